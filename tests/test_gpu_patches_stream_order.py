"""ps_patch_models and ps_patch_align keep the ORDER of the stream they are queued on, not only their results: the protocol of
tests/stream_order_cases.py (whose table is held to the header's ps_*_device functions; these calls have other names) applied to
the two, as tests/test_gpu_track_vo_stream_order.py does for its three.  The inputs hold valid stale content (zeros: black images,
counts 0, slots 0); the real inputs are copied in on the stream under test, which is still busy with a ballast when the call is
queued; the call runs through the device_batch wrapper from torch's default stream and from a side stream, and directly on the
context's stream; a copy queued behind it must hold what a fully synchronised run computes."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import patches_ref as R  # noqa: E402
import stream_order_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, ROWS, COLS, PS = 64, 48, 64, 13
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def inputs(k):
    """two frames, two sets of points with their starts"""
    imgs = np.stack([R.smooth_texture(ROWS, COLS, 40 + k), R.smooth_texture(ROWS, COLS, 40 + k, shift=(1, -1))])
    pts = np.stack([R.drawn_points(np.random.default_rng(50 + 2 * k + p), CAP, ROWS, COLS, R.half(PS)) for p in range(2)])
    return imgs, np.ascontiguousarray(pts[..., :2]), np.ascontiguousarray(pts[..., 2:]), np.array([CAP - 3 - k, 17 + k], np.int32)


def model_outputs(m):
    return [m.patch, m.gx, m.gy, m.inv]


def prep_models(k, ctx):
    from putslam_amd import device_batch as D
    from putslam_amd._abi import patch_params
    imgs, old, _, counts = inputs(k)
    final = [S._up(imgs), S._up(np.array([0, 1], np.int32)), S._up(old), S._up(counts)]
    stale = S._stale(final)
    model = D.PatchModels(2, CAP, PS, S.DEV)
    status = S._zeros((2, CAP), stale[0].dtype)

    def call(c, direct=False):
        D.patch_models(c, stale[0], stale[1], stale[2], stale[3], patch_params(PS), model, status, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: [stale[3], status] + model_outputs(model), lambda: stale[3],
                  lambda got: [got[0]] + [S.mask_rows(g, got[0]) for g in got[1:]])


def prep_align(k, ctx):
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import patch_params
    imgs, old, new, counts = inputs(k)
    final = [S._up(imgs), S._up(np.array([[0, 1], [1, 0]], np.int32)), S._up(old), S._up(new), S._up(counts)]
    stale = S._stale(final)
    model = D.PatchModels(2, CAP, PS, S.DEV)
    status, iterations = S._zeros((2, CAP), torch.uint8), S._zeros((2, CAP), torch.int32)

    def call(c, direct=False):
        D.align_patches(c, stale[0], stale[1], stale[2], stale[3], stale[4], patch_params(PS), model, status=status, iterations=iterations,
                        use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: [stale[4], stale[3], status, iterations] + model_outputs(model), lambda: stale[4],
                  lambda got: [got[0]] + [S.mask_rows(g, got[0]) for g in got[1:]])


PREPS = {"patch_models": prep_models, "patch_align": prep_align}
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
    status = expect[1] if what == "patch_models" else expect[2]
    assert int((status == 1).sum()) > 20                                   # ... and the synchronised run did real work
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
        assert torch.equal(g.view(torch.uint8), w.view(torch.uint8)), (what, k)
