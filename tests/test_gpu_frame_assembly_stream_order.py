"""ps_gather_keypoints, ps_assemble_frames and ps_front_end_frames keep the ORDER of the stream they are queued on, not only their
results: the protocol of tests/stream_order_cases.py (whose table is held to the header's ps_*_device functions; these calls have
other names) applied to the three.  The inputs hold valid stale content (zeros: empty lists, black images, no depth); the real
inputs are copied in on the stream under test, which is still busy with a ballast when the call is queued; the call runs through
the device_batch wrapper from torch's default stream and from a side stream, and directly on the context's stream; a copy queued
behind it must hold what a fully synchronised run computes."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import frame_assembly_ref as A  # noqa: E402
import stream_order_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 64
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)
NAME, PARAMS, LEVELS = "grid1x2", A.D.params(40, 1.2, 8, 20, 1, 2, CAP), 2


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def geometry():
    from putslam_amd._abi import frame_geometry
    return frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)


def depth_words(k):
    d = A.depths()
    return np.stack([d[k], d[2]]).view(np.int16)


def rows_of(k, rng):
    """Two frames of CAP key points, index lists over them and their counts"""
    xy = (rng.rand(2, CAP, 2) * [A.COLS, A.ROWS]).astype(np.float32)
    idx = np.stack([rng.permutation(CAP) for _ in range(2)]).astype(np.int32)
    return xy, idx, np.array([CAP - 3 - k, 17 + k], np.int32)


def prep_gather(k, ctx):
    from putslam_amd import device_batch as D
    rng = np.random.RandomState(40 + k)
    xy, idx, n = rows_of(k, rng)
    final = [S._up(idx), S._up(n), S._up(xy), S._up(rng.rand(2, CAP).astype(np.float32)), S._up(rng.rand(2, CAP).astype(np.float32)),
             S._up(rng.randint(0, 8, size=(2, CAP)).astype(np.int32))]
    stale = S._stale(final)
    res = []

    def call(c, direct=False):
        del res[:]
        res.extend(D.gather_keypoints(c, *stale, use_torch_stream=not direct))
    return S.Case(stale, final, call, lambda: list(res), lambda: res[4], lambda got: [S.mask_rows(g, got[4]) for g in got[:4]] + [got[4]])


def rows_outputs(out):
    return [out.pts, out.nkpts, out.xy, out.xy_undist, out.angle, out.response, out.octave, out.src_idx, out.det_dist]


def rows_norm(got):
    return [S.mask_rows(g, got[1]) if i != 1 else g for i, g in enumerate(got)]


def prep_assemble(k, ctx):
    from putslam_amd import device_batch as D
    rng = np.random.RandomState(50 + k)
    xy, idx, n = rows_of(k, rng)
    final = [S._up(xy), S._up(idx), S._up(n), S._up(depth_words(k)), S._up(rng.rand(2, CAP).astype(np.float32)),
             S._up(rng.rand(2, CAP).astype(np.float32)), S._up(rng.randint(0, 8, size=(2, CAP)).astype(np.int32))]
    stale = S._stale(final)
    out = D.FrameRowsDevice(2, CAP, S.DEV)
    geo = geometry()

    def call(c, direct=False):
        D.assemble_frames(c, geo, stale[3], stale[0], stale[1], stale[2], stale[4], stale[5], stale[6], out=out, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: rows_outputs(out), lambda: out.nkpts, rows_norm)


def fe_params():
    from putslam_amd._abi import front_end_params, orb_detect_params, orb_params
    p = PARAMS
    det = orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])
    return front_end_params(det, orb_params(p["scale_factor"], LEVELS), A.DBSCAN_EPS)


def images(k):
    im = A.images(1)
    return np.stack([im[k], im[2]])


def prep_front_end(k, ctx):
    """Two frames through a 1 x 2 grid; the handle has run once, synchronised, on the other images."""
    import torch
    from putslam_amd import device_batch as D
    final = [S._up(images(k)), S._up(depth_words(k))]
    stale = S._stale(final)
    out = D.FrameRowsDevice(2, CAP, S.DEV)
    geo = geometry()
    fe = D.FrontEnd(ctx, A.ROWS, A.COLS, 1, 2, fe_params())
    D.front_end_frames_batch(ctx, fe, S._up(images(1 - k)), S._up(depth_words(1 - k)), geo, CAP)
    torch.cuda.synchronize()

    def call(c, direct=False):
        D.front_end_frames_batch(c, fe, stale[0], stale[1], geo, CAP, out=out, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: [out.desc] + rows_outputs(out), lambda: out.nkpts,
                  lambda got: [S.mask_rows(got[0], got[2])] + rows_norm(got[1:]), fe=fe)


PREPS = {"gather": prep_gather, "assemble": prep_assemble, "front_end": prep_front_end}
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


def test_synchronised_front_end_equals_the_reference_chain(ctx):
    from oracle import oracle_py
    oracle_py.build()
    got = want(ctx, "front_end", 0)
    d = A.depths()
    frames, counts = A.chain(oracle_py, list(images(0)), [d[0], d[2]], PARAMS, LEVELS)
    assert got[2].cpu().numpy().tolist() == [len(f["pts"]) for f in frames] and all(c[2] > 0 for c in counts)
    for f, fr in enumerate(frames):
        n = len(fr["pts"])
        assert got[0][f, :n].cpu().numpy().tobytes() == fr["desc"].tobytes() and got[1][f, :n].cpu().numpy().tobytes() == fr["pts"].tobytes()


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
