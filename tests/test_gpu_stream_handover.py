"""The hand-over of a library call onto torch's current stream (device_batch._on_torch_stream) keeps torch's ORDER, not only
the results: a torch op queued just before the call writes the inputs' final values, a torch copy queued just after it reads the
outputs, nothing synchronises the host in between, and the copy must hold what a fully synchronised run computes -- from torch's
default stream (handle 0: forked to and joined from the side stream) and from an explicit stream (handed over as it is)."""
import numpy as np
import pytest

from putslam_amd import synth
from putslam_amd._abi import EST_FIXED, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config

pytestmark = pytest.mark.gpu

CAP, NK = 64, [40, 64]


@pytest.fixture(params=["default", "side"])
def ordered(request, ctx):
    """ordered(inputs, finals, call, outputs) -> clones of outputs(), taken on the stream under test behind call(), which runs
    behind the copies finals -> inputs; the stream is busy before them, so that they are still pending when call() is made."""
    import torch
    stream = torch.cuda.Stream() if request.param == "side" else torch.cuda.default_stream()
    ballast = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")

    def run(inputs, finals, call, outputs):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(4):
                ballast.fill_(1)
            for t, f in zip(inputs, finals):
                t.copy_(f)
            call()
            got = [t.clone() for t in outputs()]
        torch.cuda.synchronize()
        return got

    yield run
    ctx.set_stream(0)


def _stale_and_final(arrays):
    """For every host array: a device tensor of zeros (a valid, empty input) and one with the final values."""
    import torch
    finals = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    return [torch.zeros_like(f) for f in finals], finals


def _check(got, want):
    import torch
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), k


def _kept(kept, nkept):
    """(kept, nkept) of a filter with the rows beyond each frame's count, which are not written, cleared."""
    import torch
    cols = torch.arange(kept.shape[1], device=kept.device)[None, :]
    return [torch.where(cols < nkept[:, None], kept, torch.zeros_like(kept)), nkept]


def test_run_pairs(ctx, ordered):
    import torch
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    seq = synth.make_sequence(2, CAP, config=3, index=5100)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_FIXED, 64, seed=11)
    results = lambda b: [b.matches, b.num_matches, b.mask, b.pose, b.stats]   # noqa: E731
    fs, ref = FrameSetDevice(seq["desc"], seq["pts"], NK), PairBatchDevice([[0, 1]], CAP)
    run_pairs(ctx, prm, cfg, TUM_FR1_K, fs, ref)
    torch.cuda.synchronize()
    assert 0 < ref.num_matches.item() <= 40
    late, out = FrameSetDevice(np.zeros_like(seq["desc"]), np.zeros_like(seq["pts"]), [0, 0]), PairBatchDevice([[0, 1]], CAP)
    got = ordered([late.desc, late.pts, late.nkpts], [fs.desc, fs.pts, fs.nkpts],
                  lambda: run_pairs(ctx, prm, cfg, TUM_FR1_K, late, out), lambda: results(out))
    _check(got, results(ref))


def test_dbscan_thin_device(ctx, ordered):
    import torch
    from putslam_amd.device_batch import dbscan_thin_device
    rng = np.random.default_rng(5200)
    centres = rng.uniform(40.0, 600.0, (2, 8, 2))
    xy = (centres[np.arange(2)[:, None], rng.integers(0, 8, (2, CAP))] + rng.normal(0.0, 3.0, (2, CAP, 2))).astype(np.float32)
    xy[:, ::5] = rng.uniform(0.0, 640.0, (2, len(range(0, CAP, 5)), 2))          # (and some keypoints on their own)
    octave = rng.integers(0, 4, (2, CAP)).astype(np.int32)
    stale, final = _stale_and_final([xy, np.array(NK, np.int32), octave])
    want = dbscan_thin_device(ctx, final[0], final[1], final[2])
    torch.cuda.synchronize()
    nk = want[1].cpu().numpy()
    assert (0 < nk).all() and (nk < NK).all()
    res = []
    got = ordered(stale, final, lambda: res.extend(dbscan_thin_device(ctx, *stale[:2], stale[2])), lambda: res)
    _check(_kept(*got), _kept(*want))


def test_exclude_device(ctx, ordered):
    import torch
    from putslam_amd import api
    from putslam_amd.device_batch import exclude_device
    rng = np.random.default_rng(5300)
    e3 = (rng.uniform(-1.0, 1.0, (2, CAP, 3)) + [0, 0, 3.0]).astype(np.float32)
    e2 = rng.uniform(0.0, 600.0, (2, CAP, 2)).astype(np.float32)
    c3, c2 = e3.copy(), e2.copy()                       # every candidate on an existing feature, but for every other one
    c3[:, ::2] += rng.uniform(0.5, 1.0, (2, CAP // 2, 3)).astype(np.float32)
    c2[:, ::2] += np.float32(50.0)
    counts = np.array(NK, np.int32)
    rule = api.rule_new_map_features(0.03, 2.0, 200)
    stale, final = _stale_and_final([c3, c2, counts, e3, e2, counts])
    want = exclude_device(ctx, rule, *final)
    torch.cuda.synchronize()
    nk = want[1].cpu().numpy()
    assert (0 < nk).all() and (nk < NK).all()
    res = []
    got = ordered(stale, final, lambda: res.extend(exclude_device(ctx, rule, *stale)), lambda: res)
    _check(_kept(*got), _kept(*want))


def test_run_match_xyz(ctx, ordered):
    import torch
    from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice, run_match_xyz
    seq = synth.make_sequence(1, CAP, config=3, index=5400)
    rng = np.random.default_rng(5400)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)       # the view: the frame's keypoints,
    vdesc = seq["desc"] ^ np.packbits(rng.random((1, CAP, 256)) < 0.03, axis=2)          # a centimetre off, 3 % of the bits
    level = np.zeros((1, CAP), np.int32)

    def batch(maps, frames):
        return MapBatchDevice(maps, level, frames, level, [[0, 0]], 4 * CAP)

    views, frames = FrameSetDevice(vdesc, vpos, [CAP]), FrameSetDevice(seq["desc"], seq["pts"], [CAP])
    ref = batch(views, frames)
    run_match_xyz(ctx, ref)
    torch.cuda.synchronize()
    assert ref.num_matches.item() > 0
    late = [FrameSetDevice(np.zeros_like(vdesc), np.zeros_like(vpos), [0]) for _ in range(2)]
    out = batch(*late)
    got = ordered([t for s in late for t in (s.desc, s.pts, s.nkpts)], [t for s in (views, frames) for t in (s.desc, s.pts, s.nkpts)],
                  lambda: run_match_xyz(ctx, out), lambda: [out.matches, out.num_matches])
    _check(got, [ref.matches, ref.num_matches])
