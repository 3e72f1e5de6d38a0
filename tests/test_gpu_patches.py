"""Sub-pixel matching on patches on the GPU (ps_patches.h): ps_patch_models, ps_patch_align, the host forms and the demo equal the
sequential restatement (tests/patches_ref.py) byte for byte -- positions as bit patterns, NaNs included; status; iterations;
every model array -- with poisoned outputs checked beyond every count and for every point that has no model."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import patches_ref as R  # noqa: E402
from image_frontend_util import upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xA5
SHIFTS = [(0, 0), (1, -1), (0, 1)]      # frame k is the texture read at this offset (rows, cols)


def block_waves(ps):
    """patch_block_waves (ps_patches_rule.h): the waves of a work-group -- as many as 64 KiB of LDS hold, four at most, at 28 bytes
    for each of a wave's E rounded up to a multiple of four elements"""
    return min(4, 65536 // (((ps * ps + 3) & ~3) * 28))



@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


_FRAMES = {}


def frames(rows, cols, cn):
    """three frames of one texture, frame 0 with a flat block (NaN inverse Hessians for the patches inside it)"""
    if (rows, cols, cn) not in _FRAMES:
        imgs = [R.smooth_texture(rows, cols, 31 + cn, cn, shift=s) for s in SHIFTS]
        imgs[0][10:30, 22:44] = 77
        _FRAMES[rows, cols, cn] = (imgs, [R.grey(i) for i in imgs])
    return _FRAMES[rows, cols, cn]


def prm(ps=13, max_iter=50, min_inc=0.04, flags=0):
    from putslam_amd._abi import patch_params
    return patch_params(ps, max_iter, min_inc, flags)


def poisoned(shape, dtype):
    import torch
    a = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype).reshape(shape)
    return torch.from_numpy(a.copy()).to("cuda:0")


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def is_poison(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


_REF = {}


def ref_point(shape, s0, s1, ps, max_iter, min_inc, old, new):
    key = (shape, s0, s1, ps, max_iter, min_inc, np.float64(old).tobytes(), np.float64(new).tobytes())
    if key not in _REF:
        g = frames(*shape)[1]
        _REF[key] = R.align(g[s0], g[s1], old[0], old[1], new[0], new[1], ps, max_iter, min_inc)
    return _REF[key]


def blocks(pts_lists, cap=None):
    """per-pair lists of (oldX, oldY, newX, newY) -> old (P, cap, 2), new (P, cap, 2), counts; rows beyond a count are poison"""
    P = len(pts_lists)
    cap = cap or max(1, max(len(p) for p in pts_lists))
    old = np.full(P * cap * 2 * 8, POISON, np.uint8).view(np.float64).reshape(P, cap, 2).copy()
    new = old.copy()
    for i, p in enumerate(pts_lists):
        if len(p):
            q = np.asarray(p, np.float64).reshape(-1, 4)
            old[i, :len(q)], new[i, :len(q)] = q[:, :2], q[:, 2:]
    return old, new, np.array([len(p) for p in pts_lists], np.int32), cap


def run_align(ctx, shape, pairs, pts_lists, params, want_model=True, counts=None, padded=True, sync=True):
    import torch
    from putslam_amd import device_batch as D
    old, new, cnt, cap = blocks(pts_lists)
    cnt = cnt if counts is None else np.asarray(counts, np.int32)
    P = len(pairs)
    imgs = upload_images(frames(*shape)[0], padded)
    model = D.PatchModels(P, cap, params.patchSize, torch.device("cuda:0")) if want_model else None
    if model:
        E = params.patchSize ** 2
        model.patch, model.gx, model.gy = poisoned((P, cap, E), np.float64), poisoned((P, cap, E), np.float32), poisoned((P, cap, E), np.float32)
        model.inv = poisoned((P, cap, 9), np.float32)
    new_t, st, it = dev(new, np.float64), poisoned((P, cap), np.uint8), poisoned((P, cap), np.int32)
    D.align_patches(ctx, imgs, dev(np.asarray(pairs, np.int32).reshape(P, 2), np.int32), dev(old, np.float64), new_t, dev(cnt, np.int32),
                    params, model, status=st, iterations=it)
    if sync:
        torch.cuda.synchronize()
    return dict(old=old, new_in=new, counts=cnt, cap=cap, new=new_t, status=st, iterations=it, model=model, images=imgs)


def host(t):
    return t.cpu().numpy()


def check_align(shape, pairs, res, params, frames_n=3):
    """every output of a fused call against the restatement, and poison wherever nothing may be written"""
    ps, E = params.patchSize, params.patchSize ** 2
    new, st, it = host(res["new"]), host(res["status"]), host(res["iterations"])
    m = res["model"]
    mp, mgx, mgy, minv = (host(m.patch), host(m.gx), host(m.gy), host(m.inv)) if m else (None,) * 4
    seen = set()
    for p, (s0, s1) in enumerate(pairs):
        n = int(res["counts"][p])
        if n < 0 or n > res["cap"]:                                  # a bad count: the pair is left alone altogether
            n = 0
        assert new[p, n:].tobytes() == res["new_in"][p, n:].tobytes() and is_poison(st[p, n:]) and is_poison(it[p, n:]), p
        if m:
            assert is_poison(mp[p, n:]) and is_poison(mgx[p, n:]) and is_poison(mgy[p, n:]) and is_poison(minv[p, n:]), p
        for k in range(n):
            if not (0 <= s0 < frames_n and 0 <= s1 < frames_n):
                want = (R.OLD_TAPS_OUTSIDE, res["new_in"][p, k, 0], res["new_in"][p, k, 1], 0, None)
            else:
                want = ref_point(shape, s0, s1, ps, params.maxIter, params.minSqrtIncrement, res["old"][p, k], res["new_in"][p, k])
            where = (shape, ps, p, k, res["old"][p, k].tolist(), res["new_in"][p, k].tolist())
            assert (int(st[p, k]), int(it[p, k])) == (want[0], want[3]), (where, st[p, k], it[p, k], want[0], want[3])
            wxy = res["new_in"][p, k] if want[3] == 0 else np.array([want[1], want[2]], np.float64)
            assert new[p, k].tobytes() == wxy.tobytes(), (where, new[p, k], wxy)
            seen.add(want[0])
            if m and want[4] is None:
                assert is_poison(mp[p, k]) and is_poison(mgx[p, k]) and is_poison(mgy[p, k]) and is_poison(minv[p, k]), where
            elif m:
                assert mp[p, k].tobytes() == want[4][0].tobytes(), where
                assert mgx[p, k].tobytes() == want[4][1].tobytes() and mgy[p, k].tobytes() == want[4][2].tobytes(), where
                assert minv[p, k].tobytes() == want[4][3].tobytes(), where
    return seen


def drawn(shape, ps, n, seed, flat=True):
    rows, cols, _ = shape
    h = R.half(ps)
    pts = R.drawn_points(np.random.default_rng(seed), max(n, 13), rows, cols, h)
    if flat and ps <= 13:
        pts[12, :2] = (33.0, 20.0)                                    # inside frame 0's flat block
    return pts[:n]


SHAPES = [(48, 64, 1), (61, 97, 3)]


@pytest.mark.parametrize("ps", [3, 5, 7, 9, 13, 15, 17, 23, 25, 27, 29, 31])
@pytest.mark.parametrize("shape", SHAPES, ids=["64x48x1", "97x61x3"])
def test_align_equals_the_specification(ctx, shape, ps):
    """P = 3 pairs -- one names a slot twice --, 65 / 2 x waves + 1 / 1 points (waves: 4 up to 23, 3 at 25 and 27, 2 from 29), fused,
    the model written: every byte"""
    pairs = [(0, 1), (1, 1), (2, 0)]
    params = prm(ps, 50, 0.04 if ps >= 13 else 5e-7)
    lists = [drawn(shape, ps, 65, 10 * ps), drawn(shape, ps, 2 * block_waves(ps) + 1, 10 * ps + 1, flat=False), drawn(shape, ps, 13, 10 * ps + 2)[11:12]]
    res = run_align(ctx, shape, pairs, lists, params)
    seen = check_align(shape, pairs, res, params)
    assert {R.CONVERGED, R.OUT_OF_IMAGE, R.OLD_TAPS_OUTSIDE, R.NEW_TAPS_OUTSIDE} <= seen, seen
    if ps <= 13:
        assert R.NAN_HESSIAN in seen


@pytest.mark.parametrize("P", [1, 6])
def test_counts_around_the_wave_and_the_work_group(ctx, P):
    shape, params = SHAPES[0], prm(13, 50, 0.04)
    ns = [64] if P == 1 else [0, 1, 63, 64, 65, 2 * block_waves(13) + 1]
    lists = [drawn(shape, 13, n, 300 + n) for n in ns]
    pairs = [(k % 3, (k + 1) % 3) for k in range(P)]
    res = run_align(ctx, shape, pairs, lists, params, padded=(P == 1))
    check_align(shape, pairs, res, params)


def test_bad_counts_leave_the_pair_alone_and_bad_slots_fail_its_points(ctx):
    shape, params = SHAPES[0], prm(13, 50, 0.04)
    lists = [drawn(shape, 13, 8, 400 + k) for k in range(6)]
    pairs = [(0, 1), (0, 1), (1, 2), (3, 0), (0, -1), (2, 2)]
    res = run_align(ctx, shape, pairs, lists, params, counts=[-1, 9, 8, 8, 8, 8])           # capacity is 8
    check_align(shape, pairs, res, params)
    st = host(res["status"])
    assert is_poison(st[0]) and is_poison(st[1]) and (st[3] == 5).all() and (st[4] == 5).all() and not is_poison(st[2]) and not is_poison(st[5])


@pytest.mark.parametrize("max_iter", [0, 1, 50])
def test_iteration_limits(ctx, max_iter):
    shape, params = SHAPES[1], prm(5, max_iter, 5e-7)
    lists = [drawn(shape, 5, 20, 500)]
    res = run_align(ctx, shape, [(0, 1)], lists, params)
    seen = check_align(shape, [(0, 1)], res, params)
    it = host(res["iterations"])[0]
    assert it.max() == max_iter if max_iter < 50 else it.max() > 1
    if max_iter == 0:
        assert seen <= {R.MAX_ITERATIONS, R.NAN_HESSIAN, R.OLD_TAPS_OUTSIDE}
        assert host(res["new"]).tobytes() == res["new_in"].tobytes()


def test_every_status_value(ctx):
    shape = SHAPES[0]
    a = [(50.0, 40.0, 50.0, 40.0), (33.0, 20.0, 33.0, 20.0), (50.0, 40.0, 0.5, 40.0), (1.5, 40.0, 50.0, 40.0), (50.0, 40.0, 62.5, 40.0)]
    res = run_align(ctx, shape, [(0, 0)], [a], prm(3, 50, 0.04))
    seen = check_align(shape, [(0, 0)], res, prm(3, 50, 0.04))
    assert host(res["status"])[0].tolist() == [1, 2, 3, 5, 6]
    res = run_align(ctx, shape, [(0, 0)], [[(20.0, 40.0, 23.0, 40.0)]], prm(3, 50, 1e9))       # any first step stops; this one is long
    seen |= check_align(shape, [(0, 0)], res, prm(3, 50, 1e9))
    res = run_align(ctx, shape, [(0, 1)], [[(50.0, 40.0, 50.5, 40.0)]], prm(3, 1, 0.0))
    seen |= check_align(shape, [(0, 1)], res, prm(3, 1, 0.0))
    assert seen == set(range(7)), seen


@pytest.mark.parametrize("ps", [5, 17])
def test_model_pass_and_given_model_equal_the_fused_call(ctx, ps):
    import torch
    from putslam_amd import device_batch as D
    shape, params = SHAPES[1], prm(ps, 50, 0.04)
    pairs = [(0, 1), (2, 2), (1, 0)]
    lists = [drawn(shape, ps, n, 600 + n) for n in (20, 9, 13)]
    fused = run_align(ctx, shape, pairs, lists, params)
    check_align(shape, pairs, fused, params)
    # the model pass on the pairs' old slots: the fused call's model, status 5 / 2 / 1
    old, new, cnt, cap = blocks(lists)
    E, P = ps * ps, 3
    model = D.PatchModels(P, cap, ps, torch.device("cuda:0"))
    model.patch, model.gx, model.gy = poisoned((P, cap, E), np.float64), poisoned((P, cap, E), np.float32), poisoned((P, cap, E), np.float32)
    model.inv = poisoned((P, cap, 9), np.float32)
    st = poisoned((P, cap), np.uint8)
    slots = dev([p[0] for p in pairs], np.int32)
    D.patch_models(ctx, fused["images"], slots, dev(old, np.float64), dev(cnt, np.int32), params, model, st)
    torch.cuda.synchronize()
    for a, b in ((model.patch, fused["model"].patch), (model.gx, fused["model"].gx), (model.gy, fused["model"].gy), (model.inv, fused["model"].inv)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    fst, mst = host(fused["status"]), host(st)
    for p in range(P):
        n = cnt[p]
        assert is_poison(mst[p, n:])
        assert mst[p, :n].tolist() == [s if s in (2, 5) else 1 for s in fst[p, :n].tolist()]
    # ... and without a model block at all: the statuses alone
    st0 = poisoned((P, cap), np.uint8)
    old_t, cnt_t = dev(old, np.float64), dev(cnt, np.int32)           # (held: a tensor dropped after data_ptr() lends its block to the next one)
    ctx.patch_models(D._patch_images(fused["images"]), slots.data_ptr(), old_t.data_ptr(), cnt_t.data_ptr(), P, cap, params, None, st0.data_ptr())
    torch.cuda.synchronize()
    assert host(st0).tobytes() == mst.tobytes()
    # the alignment on the given model: the old slot (here: outside the set) and oldPts are not looked at
    new_t, gst, git = dev(new, np.float64), poisoned((P, cap), np.uint8), poisoned((P, cap), np.int32)
    given_pairs = dev([(99, p[1]) for p in pairs], np.int32)
    D.align_patches(ctx, fused["images"], given_pairs, None, new_t, dev(cnt, np.int32), params, model, given=True, status=gst, iterations=git)
    torch.cuda.synchronize()
    g_new, g_st, g_it = host(new_t), host(gst), host(git)
    ok = (np.arange(cap)[None, :] < cnt[:, None]) & (fst != 5)        # (a point without a model has nothing to be given)
    assert ok.sum() > 30 and (g_st[ok] == fst[ok]).all() and (g_it[ok] == host(fused["iterations"])[ok]).all()
    assert g_new[ok].tobytes() == host(fused["new"])[ok].tobytes()
    beyond = np.arange(cap)[None, :] >= cnt[:, None]
    assert is_poison(g_st[beyond]) and is_poison(g_it[beyond]) and g_new[beyond].tobytes() == new[beyond].tobytes()


def test_two_calls_back_to_back_on_one_stream(ctx):
    """one step, then up to fifty more from where it ended, queued without a synchronise in between, on a side stream"""
    import torch
    from putslam_amd import device_batch as D
    shape, ps = SHAPES[0], 13
    pts = drawn(shape, ps, 40, 700)
    old, new, cnt, cap = blocks([pts])
    imgs = upload_images(frames(*shape)[0], True)
    pairs = dev([(0, 1)], np.int32)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        new_t, old_t, cnt_t = dev(new, np.float64), dev(old, np.float64), dev(cnt, np.int32)
        _, st1, it1 = D.align_patches(ctx, imgs, pairs, old_t, new_t, cnt_t, prm(ps, 1, 0.04))
        _, st2, it2 = D.align_patches(ctx, imgs, pairs, old_t, new_t, cnt_t, prm(ps, 50, 0.04))
        got = [t.clone() for t in (new_t, st1, it1, st2, it2)]
    torch.cuda.synchronize()
    ctx.set_stream(0)
    g = frames(*shape)[1]
    for k in range(40):
        a = R.align(g[0], g[1], old[0, k, 0], old[0, k, 1], new[0, k, 0], new[0, k, 1], ps, 1, 0.04)
        mid = (a[1], a[2]) if a[3] else (new[0, k, 0], new[0, k, 1])
        b = R.align(g[0], g[1], old[0, k, 0], old[0, k, 1], mid[0], mid[1], ps, 50, 0.04)
        end = np.array((b[1], b[2]) if b[3] else mid, np.float64)
        assert (int(got[1][0, k]), int(got[2][0, k]), int(got[3][0, k]), int(got[4][0, k])) == (a[0], a[3], b[0], b[3]), k
        assert host(got[0])[0, k].tobytes() == end.tobytes(), k


def test_host_forms_through_the_context(ctx):
    shape, ps = SHAPES[1], 13
    imgs, g = frames(*shape)
    parent = np.full((shape[0], shape[1] + 4, 3), 0xEE, np.uint8)      # rows that lie further apart than their pixels
    parent[:, :shape[1]] = imgs[0]
    old_img, new_img = parent[:, :shape[1]], imgs[1]
    pts = drawn(shape, ps, 24, 800)
    params = prm(ps, 50, 0.04)
    want = R.align_batch(imgs[0], imgs[1], pts[:, :2], pts[:, 2:], ps, 50, 0.04)
    new, st, it = ctx.optimize_locations(old_img, new_img, pts[:, :2], pts[:, 2:], params)
    assert st.tolist() == want["status"].tolist() and it.tolist() == want["iterations"].tolist() and new.tobytes() == want["pts"].tobytes()
    patch, pst = ctx.compute_patch(old_img, pts[:, :2], params)
    gx, gy, inv, gst = ctx.compute_patch_gradient(old_img, pts[:, :2], params)
    assert pst.tolist() == gst.tolist() == [s if s in (2, 5) else 1 for s in want["status"].tolist()]
    assert patch.tobytes() == want["patch"].tobytes() and gx.tobytes() == want["gx"].tobytes() and gy.tobytes() == want["gy"].tobytes()
    assert inv.reshape(-1, 9).tobytes() == want["inv"].tobytes()
    have = pst != 5                                                     # the three-call protocol for the points that have a model
    new3, st3, it3 = ctx.optimize_location(patch[have], new_img, pts[have, 2:], gx[have], gy[have], inv[have], params, old_img=old_img)
    assert st3.tolist() == want["status"][have].tolist() and it3.tolist() == want["iterations"][have].tolist()
    assert new3.tobytes() == want["pts"][have].tobytes()
    assert ctx.optimize_locations(old_img, new_img, np.zeros((0, 2)), np.zeros((0, 2)), params)[1].shape == (0,)


def test_bad_arguments_are_refused_with_text_and_touch_nothing(ctx):
    import torch
    from putslam_amd import api, device_batch as D
    from putslam_amd._abi import PsPatchParams
    shape = SHAPES[0]
    imgs = upload_images(frames(*shape)[0], False)
    old, new, cnt, cap = blocks([drawn(shape, 13, 8, 900)])
    pairs, cnt_t, old_t = dev([(0, 1)], np.int32), dev(cnt, np.int32), dev(old, np.float64)

    def refused(params, images=imgs, **kw):
        new_t, st, it = dev(new, np.float64), poisoned((1, cap), np.uint8), poisoned((1, cap), np.int32)
        with pytest.raises(api.PsError) as e:
            D.align_patches(ctx, images, pairs, old_t, new_t, cnt_t, params, status=st, iterations=it, **kw)
        torch.cuda.synchronize()
        assert e.value.code == -1 and "ps_patch_align" in str(e.value), str(e.value)
        assert is_poison(host(st)) and is_poison(host(it)) and host(new_t).tobytes() == new.tobytes()
    for bad in (prm(12), prm(1), prm(33), prm(13, -1), prm(13, 1001), prm(13, 50, 0.04, flags=2), PsPatchParams(0.04, 13, 50, 0, 1)):
        refused(bad)
    two = torch.zeros((1, 48, 64, 2), dtype=torch.uint8, device="cuda:0")
    refused(prm(13), images=two)
    with pytest.raises(api.PsError) as e:                                # given model without the arrays
        ctx.patch_align(D._patch_images(imgs), pairs.data_ptr(), None, old_t.data_ptr(), cnt_t.data_ptr(), 1, cap, prm(13, flags=1), None,
                        old_t.data_ptr(), old_t.data_ptr())
    assert e.value.code == -1 and "model" in str(e.value)
    with pytest.raises(api.PsError) as e:
        ctx.patch_models(D._patch_images(imgs), None, old_t.data_ptr(), cnt_t.data_ptr(), 1, cap, prm(13), D.PatchModels(1, cap, 13, "cuda:0").struct(),
                         None)
    assert e.value.code == -1 and "ps_patch_models" in str(e.value)
    with pytest.raises(api.PsError):
        ctx.optimize_locations(np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.uint8), [[20, 20]], [[20, 20]], prm(14))
    # P == 0 is fine, whatever else is NULL
    ctx.patch_align(D._patch_images(imgs), None, None, None, None, 0, 0, prm(13), None, None, None)
    ctx.patch_models(D._patch_images(imgs), None, None, None, 0, 0, prm(13), D.PatchModels(1, 1, 13, "cuda:0").struct(), None)
    torch.cuda.synchronize()


def test_demo_prints_the_restatements_final():
    from demos import demo_patches as M
    run = subprocess.run([sys.executable, "-m", "demos.demo_patches"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    final = [l for l in run.stdout.splitlines() if l.startswith("FINAL: ")]
    assert len(final) == 1, run.stdout
    old, new = M.make_pair()
    st, x, y, it, _ = R.align(R.grey(old), R.grey(new), M.X, M.Y, M.NEW_X, M.NEW_Y, M.PATCH_SIZE, M.MAX_ITER, M.MIN_SQRT_INCREMENT)
    assert [float(v) for v in final[0].split()[1:]] == [float(x), float(y)]
    assert "status %d after %d iterations" % (st, it) in run.stdout
