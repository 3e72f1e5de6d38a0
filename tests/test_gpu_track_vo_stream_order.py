"""ps_ransac_match_lists, ps_assemble_tracked and ps_track_vo_pairs keep the ORDER of the stream they are queued on, not only their
results: the protocol of tests/stream_order_cases.py (whose table is held to the header's ps_*_device functions; these calls have
other names) applied to the three, as tests/test_gpu_frame_assembly_stream_order.py does for the frame assembly.  The inputs hold
valid stale content (zeros: empty lists, counts 0, pairs (0, 0), no depth); the real inputs are copied in on the stream under test,
which is still busy with a ballast when the call is queued; the call runs through the device_batch wrapper from torch's default
stream and from a side stream, and directly on the context's stream; a copy queued behind it must hold what a fully synchronised
run computes."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import stream_order_cases as S  # noqa: E402
import track_vo_ref as R  # noqa: E402
from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import EST_FIXED, EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, frame_geometry, make_config, track_vo_params  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 64
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def geometry():
    return frame_geometry(R.K, R.DIST5, R.DEPTH_SCALE)


def depth_words():
    return np.stack(R.depths()).view(np.int16)


def prep_match_lists(k, ctx):
    """Two pairs of 64 points with their cross-check matches as the caller's lists"""
    import torch
    from putslam_amd import device_batch as D
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, keep = make_config(EST_FIXED, 64, seed=11 + k)
    prev, cur, lists = [], [], np.zeros((2, CAP, 4), np.int32)
    num = np.zeros(2, np.int32)
    for p in range(2):
        a, b = synth.make_pair(CAP, config=2, index=6100 + 2 * k + p)
        m = ctx.match_hamming256(a["desc"], b["desc"])
        prev.append(a["pts"])
        cur.append(b["pts"])
        lists[p, :len(m)] = m.view(np.int32).reshape(-1, 4)
        num[p] = len(m)
    final = [S._up(np.stack(prev)), S._up(np.stack(cur)), S._up(np.array([CAP, CAP], np.int32)), S._up(lists), S._up(num)]
    stale = S._stale(final)
    sets_p, sets_c = D.PointSets(stale[0], stale[2]), D.PointSets(stale[1], stale[2])
    out = D.PairResultsDevice(2, CAP, S.DEV)

    def call(c, direct=False):
        D.ransac_match_lists(c, prm, cfg, TUM_FR1_K, sets_p, sets_c, stale[3], stale[4], out=out, use_torch_stream=not direct)
    num_in = lambda: out.stats[:, :4].contiguous().view(torch.int32).reshape(-1)   # noqa: E731  (PsRansacStats::numMatchesIn)
    return S.Case(stale, final, call, lambda: [out.mask, out.pose, out.stats], num_in, keep=keep)


def tracked_outputs(rows):
    return [rows.counts, rows.xy, rows.xy_undist, rows.pts, rows.angle, rows.response, rows.octave, rows.det_dist]


def tracked_norm(got):
    return [got[0]] + [S.mask_rows(g, got[0]) for g in got[1:]]


def prep_assemble_tracked(k, ctx):
    from putslam_amd import device_batch as D
    rng = np.random.RandomState(70 + k)
    pts = (rng.rand(2, CAP, 2) * [R.COLS, R.ROWS]).astype(np.float32)
    idx = np.stack([rng.permutation(CAP) for _ in range(2)]).astype(np.int32)
    final = [S._up(pts), S._up(idx), S._up(np.array([CAP - 3 - k, 17 + k], np.int32)), S._up(np.array([1 + k, 3], np.int32)),
             S._up(depth_words()), S._up(rng.rand(2, CAP).astype(np.float32)), S._up(rng.rand(2, CAP).astype(np.float32)),
             S._up(rng.randint(0, 8, size=(2, CAP)).astype(np.int32)), S._up(rng.rand(2, CAP))]
    stale = S._stale(final)
    prev = D.TrackedRows(2, CAP, S.DEV)
    prev.angle, prev.response, prev.octave, prev.det_dist = stale[5], stale[6], stale[7], stale[8]
    out = D.TrackedRows(2, CAP, S.DEV)
    geo = geometry()

    def call(c, direct=False):
        D.assemble_tracked(c, geo, stale[4], stale[3], stale[0], stale[1], stale[2], prev, out, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: tracked_outputs(out), lambda: out.counts, tracked_norm)


def prep_track_vo(k, ctx):
    """Two pairs of the scene of tests/track_vo_ref.py from hand-built rows; the pyramids were built, synchronised, in prep."""
    import torch
    from oracle import oracle_py
    from putslam_amd import device_batch as D
    oracle_py.build()
    imgs = np.stack(R.images(1))[..., 0]
    pyr = D.KltPyramids(ctx, R.ROWS, R.COLS, 1, len(imgs), R.WIN, R.LEVELS)
    pyr.build(S._up(imgs))
    torch.cuda.synchronize()
    pairs = np.array([[k, k + 1], [k + 1, k + 2]], np.int32)
    first = [R.first_rows(oracle_py, CAP, 30 + 2 * k + p, int(pairs[p, 0])) for p in range(2)]
    stack = lambda n: np.stack([r[n] for r in first])   # noqa: E731
    final = [S._up(pairs), S._up(stack("xy")), S._up(stack("pts")), S._up(np.array([CAP, CAP - 5], np.int32)), S._up(depth_words()),
             S._up(stack("angle")), S._up(stack("response")), S._up(stack("octave")), S._up(stack("det_dist"))]
    stale = S._stale(final)
    rows = D.TrackedRows(2, CAP, S.DEV)
    rows.xy, rows.pts, rows.counts = stale[1], stale[2], stale[3]
    rows.angle, rows.response, rows.octave, rows.det_dist = stale[5], stale[6], stale[7], stale[8]
    out = D.TrackVoDevice(2, CAP, S.DEV)
    prm, geo, tp = R.params(), geometry(), track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST)
    cfg, keep = make_config(EST_RANSAC, R.HYP, seed=R.SEED + k)

    def call(c, direct=False):
        D.track_vo_pairs(c, pyr, stale[4], geo, stale[0], rows, prm, cfg, tp, out=out, use_torch_stream=not direct)

    def outputs():
        return [out.num_matches, rows.counts, out.next_pts, out.status, out.err, out.matches, out.kept_idx, out.mask, out.pose,
                out.stats] + tracked_outputs(out.rows)

    def norm(got):
        n, prevn = got[0], got[1]
        return ([n] + [S.mask_rows(g, prevn) for g in got[2:5]] + [S.mask_rows(g, n) for g in got[5:8]] + got[8:10]
                + tracked_norm(got[10:]))
    return S.Case(stale, final, call, outputs, lambda: out.num_matches, norm, pyr=pyr, keep=keep)


PREPS = {"match_lists": prep_match_lists, "assemble_tracked": prep_assemble_tracked, "track_vo": prep_track_vo}
_WANT = {}


def want(ctx, what, k):
    """What a fully synchronised run of case k computes (computed once)."""
    import torch
    if (what, k) not in _WANT:
        case = PREPS[what](k, ctx)
        for t, f in zip(case.inputs, case.finals):
            t.copy_(f)
        torch.cuda.synchronize()
        case.call(ctx)
        torch.cuda.synchronize()
        assert bool((case.counts() > 0).all()), case.counts()
        _WANT[what, k] = case.norm([t.clone() for t in case.outputs()])
        torch.cuda.synchronize()
        ctx.set_stream(0)
    return _WANT[what, k]


def busy(ballast):
    import torch
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first.record()
    for _ in range(BALLAST_FILLS):
        ballast.fill_(1)
    last.record()
    return last, first


@pytest.mark.parametrize("how", ["default", "side", "direct"])
@pytest.mark.parametrize("what", list(PREPS))
def test_call_keeps_the_order_of_its_stream(ctx, ballast, what, how):
    import torch
    expect = want(ctx, what, 0)
    other = want(ctx, what, 1)
    assert any(not torch.equal(a, b) for a, b in zip(expect, other))      # the two seeds differ: stale inputs would show
    case = PREPS[what](0, ctx)
    torch.cuda.synchronize()
    stream = torch.cuda.default_stream() if how == "default" else torch.cuda.Stream()
    if how == "direct":
        ctx.set_stream(stream.cuda_stream)
    with S.quiet_collector(), torch.cuda.stream(stream):     # (no handle of an earlier test is destroyed inside the timed call)
        last, first = busy(ballast)
        for t, f in zip(case.inputs, case.finals):
            t.copy_(f)
        t0 = time.perf_counter()
        case.call(ctx, direct=(how == "direct"))
        t1 = time.perf_counter()
        drained = last.query()
        got = [t.clone() for t in case.outputs()]
    torch.cuda.synchronize()
    ctx.set_stream(0)
    print("%s %s: queued in %.3f ms on the host, ballast %.3f ms" % (what, how, (t1 - t0) * 1e3, first.elapsed_time(last)))
    assert not drained, "ballast too short (or the call synchronised the host): the stream was idle when the call was queued"
    for k, (g, w) in enumerate(zip(case.norm(got), expect)):
        assert torch.equal(g, w), (what, k)
