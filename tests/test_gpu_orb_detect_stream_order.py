"""ps_orb_detect_frames keeps the ORDER of the stream it is queued on, not only its results: the protocol of
tests/stream_order_cases.py (whose table is held to the header's ps_*_device functions; this call has another name) applied to the
ORB detector.  The inputs hold valid stale content (zero images); the real images are copied in on the stream under test, which is
still busy with a ballast when the call is queued; the call runs through the device_batch wrapper from torch's default stream and
from a side stream, and directly on the context's stream; a copy queued behind it must hold what a fully synchronised run
computes."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_detect_ref as R  # noqa: E402
import stream_order_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, CAP = 96, 128, 32
PARAMS = R.params(24, 1.2, 3, 20, 1, 2, CAP)
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def prm():
    from putslam_amd._abi import orb_detect_params
    p = PARAMS
    return orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])


def images(k):
    return np.stack([R.image("texture", ROWS, COLS), R.image("noise256" if k == 0 else "noise4", ROWS, COLS)])


def prep(k, ctx):
    """A Case of stream_order_cases: two frames through a 1 x 2 grid; the detector has run once, synchronised, on other images, so
    its ROI lists have the size this call needs and nothing allocates."""
    import torch
    from putslam_amd import device_batch as D
    final = [S._up(images(k))]
    stale = S._stale(final)
    out = [S._zeros((2, CAP, 2), torch.float32), S._zeros((2, CAP), torch.float32), S._zeros((2, CAP), torch.float32),
           S._zeros((2, CAP), torch.int32), S._zeros((2,), torch.int32)]
    det = D.OrbDetector(ctx, ROWS, COLS, 1, 2, prm())
    D.detect_features_orb_batch(ctx, det, S._up(images(1 - k)), prm(), CAP)
    torch.cuda.synchronize()
    return S.Case(stale, final, lambda c, direct=False: D.detect_features_orb_batch(c, det, stale[0], prm(), CAP, *out, use_torch_stream=not direct),
                  lambda: list(out), lambda: out[4],
                  lambda got: [S.mask_rows(got[0], got[4]), S.mask_rows(got[1], got[4]), S.mask_rows(got[2], got[4]), S.mask_rows(got[3], got[4]), got[4]],
                  det=det)


def want(ctx, k):
    import torch
    case = prep(k, ctx)
    for t, f in zip(case.inputs, case.finals):
        t.copy_(f)
    torch.cuda.synchronize()
    case.call(ctx)
    torch.cuda.synchronize()
    assert bool((case.counts() > 0).all()), case.counts()
    out = case.norm([t.clone() for t in case.outputs()])
    torch.cuda.synchronize()
    ctx.set_stream(0)
    return out


def busy(ballast):
    import torch
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first.record()
    for _ in range(BALLAST_FILLS):
        ballast.fill_(1)
    last.record()
    return last, first


def test_synchronised_run_equals_the_restatement(ctx):
    got = want(ctx, 0)
    n = got[4].cpu().numpy()
    for f, img in enumerate(images(0)):
        w = R.detect_closed(img, PARAMS)
        assert int(n[f]) == len(w[1]) > 0
        assert got[1][f, :len(w[1])].cpu().numpy().tobytes() == w[1].tobytes() and got[0][f, :len(w[1])].cpu().numpy().tobytes() == w[0].tobytes()


@pytest.mark.parametrize("how", ["default", "side", "direct"])
def test_call_keeps_the_order_of_its_stream(ctx, ballast, how):
    import torch
    expect = want(ctx, 0)
    other = want(ctx, 1)
    assert any(not torch.equal(a, b) for a, b in zip(expect, other))      # the two seeds differ: stale inputs would show
    case = prep(0, ctx)
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
    print("%s: queued in %.3f ms on the host, ballast %.3f ms" % (how, (t1 - t0) * 1e3, first.elapsed_time(last)))
    assert not drained, "ballast too short (or the call synchronised the host): the stream was idle when the call was queued"
    for k, (g, w) in enumerate(zip(case.norm(got), expect)):
        assert torch.equal(g, w), k
