"""ps_track_candidates and ps_track_close_pairs keep the ORDER of the stream they are queued on, not only their results: the protocol
of tests/stream_order_cases.py (whose table is held to the header's ps_*_device functions; these calls have other names) applied to
the two, as tests/test_gpu_track_vo_stream_order.py does for the first half of the step.  The inputs hold valid stale content (zeros:
counts 0, frame and slot 0, black images, no depth); the real inputs are copied in on the stream under test, which is still busy
with a ballast when the call is queued; the call runs through the device_batch wrapper from torch's default stream and from a side
stream, and directly on the context's stream; a copy queued behind it must hold what a fully synchronised run computes.  (The
level rule's table is uploaded at a context's first use of it, which waits: the synchronised runs come first.)"""
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
import track_close_ref as C  # noqa: E402
from putslam_amd._abi import frame_geometry, front_end_params, orb_detect_params, orb_params, track_close_params  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, CCAP = 24, 64
MINIMAL, DIST = 20, 5.0
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)
NAMES = tuple(n for n, _, _ in C.COLUMNS)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def block(rows_list, cap):
    """[the columns as (P, cap, ...) arrays, zero beyond every count] + [counts]"""
    out = []
    for n, dt, tail in C.COLUMNS:
        a = np.zeros((len(rows_list), cap) + tail, dt)
        for p, r in enumerate(rows_list):
            a[p, :len(r["xy"])] = r[n]
        out.append(a)
    return out + [np.array([len(r["xy"]) for r in rows_list], np.int32)]


def closed_outputs(out):
    return [out.rows.counts, out.refill, out.desc, out.src_idx] + [getattr(out.rows, n) for n in NAMES]


def closed_norm(got):
    return got[:2] + [S.mask_rows(g, got[0]) for g in got[2:]]


def prep_close(k, ctx):
    """Two due pairs (15 + k and 17 tracked rows) with 40 and 64 candidates; the pyramids were built, synchronised, in prep."""
    import torch
    from putslam_amd import device_batch as D
    tracked = [C.random_rows(15 + k, 40 + k), C.random_rows(17, 50 + k)]
    cand = [C.near_and_far_candidates(tracked[0], 40, 60 + k, DIST), C.near_and_far_candidates(tracked[1], CCAP, 70 + k, DIST)]
    final = [S._up(a) for a in block(tracked, CAP) + block(cand, CCAP)] + [S._up(np.array([1, 0], np.int32)), S._up(np.array([k, 1 - k], np.int32))]
    stale = S._stale(final)
    rows = D.TrackedRows(2, CAP, S.DEV)
    frames = D.FrameRowsDevice(2, CCAP, S.DEV)
    for i, n in enumerate(NAMES):
        setattr(rows, n, stale[i])
        setattr(frames, n, stale[8 + i])
    rows.counts, frames.nkpts = stale[7], stale[15]
    pyr = D.OrbPyramids(ctx, A.ROWS, A.COLS, 1, 2)
    pyr.build(S._up(np.stack(A.images(1)[:2])))
    tc = D.TrackClose(ctx, 2, CAP + CCAP)
    out = D.ClosedRows(2, CAP + CCAP, S.DEV)
    tp = track_close_params(MINIMAL, DIST)
    torch.cuda.synchronize()

    def call(c, direct=False):
        D.track_close_pairs(c, tc, pyr, stale[17], rows, frames, stale[16], tp, out=out, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: closed_outputs(out), lambda: out.rows.counts, closed_norm, pyr=pyr, tc=tc)


def fe_params():
    name, p, levels = A.CASES[1]
    det = orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])
    return front_end_params(det, orb_params(p["scale_factor"], levels), A.DBSCAN_EPS)


def prep_candidates(k, ctx):
    """Two frames through a 1 x 2 grid; the handle has run once, synchronised, on the other images."""
    import torch
    from putslam_amd import device_batch as D
    im, d = A.images(1), A.depths()
    pick = lambda j: (np.stack([im[j], im[2]]), np.stack([d[j], d[2]]).view(np.int16))   # noqa: E731
    final = [S._up(a) for a in pick(k)]
    stale = S._stale(final)
    out = D.FrameRowsDevice(2, A.CAPACITY, S.DEV)
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    fe = D.FrontEnd(ctx, A.ROWS, A.COLS, 1, 2, fe_params())
    D.track_candidates(ctx, fe, *[S._up(a) for a in pick(1 - k)], geo, A.CAPACITY)
    torch.cuda.synchronize()

    def call(c, direct=False):
        D.track_candidates(c, fe, stale[0], stale[1], geo, A.CAPACITY, out=out, use_torch_stream=not direct)

    def outputs():
        return [out.nkpts, out.src_idx] + [getattr(out, n) for n in NAMES]
    return S.Case(stale, final, call, outputs, lambda: out.nkpts, lambda got: got[:1] + [S.mask_rows(g, got[0]) for g in got[1:]], fe=fe)


PREPS = {"candidates": prep_candidates, "close": prep_close}
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
    assert any(not torch.equal(a, b) for a, b in zip(expect, other))      # the two cases differ: stale inputs would show
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
