"""Pyramidal Lucas-Kanade tracking on the GPU (ps_klt.h): the pyramid and derivative passes, ps_klt_track_device, ps_klt_select_device,
the host forms ps_calc_optical_flow_pyr_lk / ps_perform_tracking and the Python wrappers equal the sequential restatement
(tests/klt_ref.py) byte for byte -- float words compared as uint32, sentinel-filled outputs checked beyond every count."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import klt_ref as K  # noqa: E402
from image_frontend_util import u32, upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_B = np.uint8(0xA5)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def prm(win=7, max_levels=3, max_count=30, eps=0.01, flags=0, min_eig=1e-4):
    from putslam_amd._abi import klt_params
    return klt_params(win, max_levels, max_count, eps, flags, min_eig)


def images(rows, cols, cn, shifts, seed=11):
    """One texture sampled at several shifts: frame k carries the flow shifts[k] relative to frame 0."""
    return [K.smooth_texture(rows, cols, cn, seed=seed, shift=(-s[0], -s[1])) for s in shifts]


def sentinel(shape, dtype):
    import torch
    if dtype == np.uint8:
        a = np.full(shape, SENT_B, np.uint8)
    else:
        a = np.full(shape, SENT_F, np.uint32).view(np.float32)
    return torch.from_numpy(a).to("cuda:0")


def run_device(ctx, imgs, pairs, pts_lists, params, padded=False, init=None, counts=None):
    """track_klt_pairs over sentinel-filled blocks -> (nextPts, status, err) as numpy, whole blocks."""
    import torch
    from putslam_amd import device_batch
    rows, cols, cn = K.as_hwc(imgs[0]).shape
    pyr = device_batch.KltPyramids(ctx, rows, cols, cn, len(imgs), params.winSize, params.maxLevels)
    pyr.build(upload_images(imgs, padded))
    P, cap = len(pairs), max(1, max(len(p) for p in pts_lists))
    prev = np.zeros((P, cap, 2), np.float32)
    for i, p in enumerate(pts_lists):
        prev[i, :len(p)] = p
    cnt = np.array([len(p) for p in pts_lists] if counts is None else counts, np.int32)
    nxt = sentinel((P, cap, 2), np.float32)
    if init is not None:
        h = nxt.cpu().numpy()
        for i, q in enumerate(init):
            h[i, :len(q)] = q
        nxt = torch.from_numpy(h).to("cuda:0")
    st, er = sentinel((P, cap), np.uint8), sentinel((P, cap), np.float32)
    dev = torch.device("cuda:0")
    device_batch.track_klt_pairs(ctx, pyr, torch.from_numpy(np.asarray(pairs, np.int32).reshape(P, 2)).to(dev),
                                 torch.from_numpy(prev).to(dev), torch.from_numpy(cnt).to(dev), params, nxt, st, er)
    torch.cuda.synchronize()
    out = nxt.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()
    pyr.close()
    return out


def ref_track(prev, nxt, pts, params, init=None):
    return K.track(prev, nxt, pts, params.winSize, params.maxLevels, params.maxCount, params.eps, params.flags,
                   params.minEigThreshold, next_pts=init)


def assert_pair_equal(got, want, n, what=""):
    """Rows 0 .. n-1 of one pair equal the restatement's; everything beyond still holds the sentinels."""
    (gn, gs, ge), (wn, ws, we) = got, want
    bad = [i for i in range(n) if u32(gn[i]).tolist() != u32(wn[i]).tolist() or gs[i] != ws[i] or u32(ge[i:i + 1])[0] != u32(we[i:i + 1])[0]]
    assert not bad, (what, bad[:8], [(gn[i].tolist(), wn[i].tolist(), int(gs[i]), int(ws[i]), float(ge[i]), float(we[i])) for i in bad[:4]])
    assert (u32(gn[n:]) == SENT_F).all() and (gs[n:] == SENT_B).all() and (u32(ge[n:]) == SENT_F).all(), what


def test_main_scene_every_exit(ctx):
    """The 48 x 64 scene whose walks end at every exit of the tracker (tests/test_klt_ref_host.py), directed points included:
    NaN, +-inf, 1e30, the two sides of both bounds, pixel centres and .5 offsets."""
    prev, nxt, pts = K.main_scene()
    m = K.MAIN_SCENE
    p = prm(m["win"], m["max_levels"], m["max_count"], m["eps"])
    got = run_device(ctx, [prev, nxt], [(0, 1)], [pts], p)
    assert_pair_equal([g[0] for g in got], ref_track(prev, nxt, pts, p), len(pts))


# rows, cols, cn, win, maxLevels, flags, maxCount, eps, minEig, points, padded strides
CASES = [
    (48, 64, 1, 3, 3, 0, 30, 0.01, 1e-4, 63, False),
    (48, 64, 3, 7, 3, 0, 30, 0.01, 1e-4, 64, True),
    (48, 64, 1, 8, 3, 0, 30, 0.01, 1e-4, 65, True),
    (48, 64, 3, 8, 0, 0, 30, 0.0, 1e-4, 40, False),
    (37, 53, 1, 7, 3, 0, 150, 0.0, 1e-4, 65, False),       # maxCount clamped to 100, eps 0: cap and oscillation only
    (37, 53, 3, 7, 3, K.GET_MIN_EIGENVALS, 30, 0.01, 1e-4, 40, True),
    (37, 53, 1, 21, 3, 0, 30, 20.0, 1e-4, 40, False),      # eps clamped to 10: the first step ends every walk
    (96, 128, 1, 7, 3, K.USE_INITIAL_FLOW, 30, 0.01, 1e-4, 64, False),
    (96, 128, 3, 21, 3, K.USE_INITIAL_FLOW | K.GET_MIN_EIGENVALS, 1, 0.01, 1e-4, 40, True),
    (96, 128, 3, 31, 3, 0, 30, 0.01, 1e-4, 24, False),     # the largest window: 2883 elements, one wave a work-group
    (96, 128, 1, 31, 0, 0, 30, 0.01, 1e-4, 24, True),
    (48, 64, 1, 7, 3, 0, 0, 0.01, 1e-4, 40, False),        # maxCount 0: no step is taken
    (48, 64, 1, 7, 3, 0, 1, 0.01, 1e-4, 40, False),
    (48, 64, 3, 7, 3, 0, 30, 0.01, 5.0, 64, False),        # a minEig threshold most points fail
    (48, 64, 1, 7, 3, K.GET_MIN_EIGENVALS, 30, 0.01, 5.0, 40, True),
]


@pytest.mark.parametrize("rows,cols,cn,win,levels,flags,count,eps,min_eig,n,padded", CASES)
def test_track_equals_restatement(ctx, rows, cols, cn, win, levels, flags, count, eps, min_eig, n, padded):
    prev, nxt = images(rows, cols, cn, [(0, 0), (2.3, -1.6)], seed=rows + cn)
    pts = np.concatenate([K.random_points(rows, cols, n - 8, win * 7 + n), K.directed_points(win, rows, cols)[[0, 5, 7, 10, 15, 17, 18, 20]]])
    init = None
    if flags & K.USE_INITIAL_FLOW:
        rng = np.random.default_rng(3)
        init = (pts + rng.uniform(-3, 3, pts.shape)).astype(np.float32)
        init[1] = (np.nan, 4.0)
    p = prm(win, levels, count, eps, flags, min_eig)
    got = run_device(ctx, [prev, nxt], [(0, 1)], [pts], p, padded, None if init is None else [init])
    want = ref_track(prev, nxt, pts, p, init)
    assert_pair_equal([g[0] for g in got], want, n, (rows, cols, cn, win))
    if min_eig > 1.0:
        assert want[1].sum() < n // 2


def test_batch_of_ragged_pairs_and_count_edges(ctx):
    """P = 5 with counts [0, 1, 64, 65, 300] over 6 slots, one pair naming the same slot twice; then the same batch with a count of
    -1 and one of capacity + 1: those pairs are left alone altogether, and the selection reports -1 for them."""
    import torch
    from putslam_amd import device_batch
    rows, cols = 48, 64
    imgs = images(rows, cols, 1, [(0, 0), (1.5, 0.5), (-2.0, 1.0), (0.7, -2.2), (3.0, 3.0), (-1.0, -1.0)])
    pairs = [(0, 1), (2, 2), (1, 3), (5, 4), (3, 0)]
    counts = [0, 1, 64, 65, 300]
    pts = [K.random_points(rows, cols, c, 40 + c) for c in counts]
    p = prm()
    nxt, st, er = run_device(ctx, imgs, pairs, pts, p)
    want = [ref_track(imgs[a], imgs[b], q, p) for (a, b), q in zip(pairs, pts)]
    for i, c in enumerate(counts):
        assert_pair_equal((nxt[i], st[i], er[i]), want[i], c, i)
    assert want[1][1][0] == 1 and want[1][2][0] == 0          # (the same slot twice: the point stays, error 0)
    bad_counts = [300, -1, 64, 301, 0]
    q = pts[4]
    nxt2, st2, er2 = run_device(ctx, imgs, pairs, [q, q[:0], q[:64], q, q[:0]], p, counts=bad_counts)
    for i in (1, 3):
        assert (u32(nxt2[i]) == SENT_F).all() and (st2[i] == SENT_B).all() and (u32(er2[i]) == SENT_F).all()
    w0 = ref_track(imgs[0], imgs[1], pts[4], p)
    assert_pair_equal((nxt2[0], st2[0], er2[0]), w0, 300)
    dev = torch.device("cuda:0")
    sel = device_batch.select_tracked(ctx, torch.from_numpy(nxt2).to(dev), torch.from_numpy(st2).to(dev), torch.from_numpy(er2).to(dev),
                                      torch.tensor(bad_counts, dtype=torch.int32, device=dev), 4.0, 1.5)
    torch.cuda.synchronize()
    num = sel[1].cpu().numpy()
    assert num[1] == -1 and num[3] == -1 and num[4] == 0
    kept, _ = K.select_pairwise(w0[0], w0[1], w0[2], 4.0, 1.5)
    assert num[0] == len(kept) and np.array_equal(sel[3].cpu().numpy()[0, :len(kept)], kept)


def test_bad_slot_fails_the_pair_and_bad_arguments_are_rejected(ctx):
    """A pair that names a slot outside the set has its points failed (status 0, err 0, nextPts untouched), as the header says;
    shapes and parameters outside their range are rejected with PS_ERR_BAD_ARG before anything is launched."""
    from putslam_amd import api, device_batch
    rows, cols = 48, 64
    imgs = images(rows, cols, 1, [(0, 0), (1.0, 1.0)])
    pts = K.random_points(rows, cols, 20, 1)
    p = prm()
    nxt, st, er = run_device(ctx, imgs, [(0, 2), (-1, 0), (0, 1)], [pts, pts, pts], p)
    for i in (0, 1):
        assert (u32(nxt[i]) == SENT_F).all() and not st[i].any() and not u32(er[i]).any()
    assert_pair_equal((nxt[2], st[2], er[2]), ref_track(imgs[0], imgs[1], pts, p), 20)
    for shape in ((7, 64), (48, 7), (5, 5)):                      # rows <= W or cols <= W
        with pytest.raises(api.PsError) as e:
            device_batch.KltPyramids(ctx, shape[0], shape[1], 1, 2, 7, 3)
        assert e.value.code == -1
        with pytest.raises(api.PsError) as e:
            ctx.calc_optical_flow_pyr_lk(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), pts, p)
        assert e.value.code == -1
    for bad in (prm(win=2), prm(win=32), prm(max_levels=8), prm(max_levels=-1), prm(flags=1)):
        with pytest.raises(api.PsError) as e:
            ctx.calc_optical_flow_pyr_lk(imgs[0], imgs[1], pts, bad)
        assert e.value.code == -1
    with pytest.raises(api.PsError) as e:
        device_batch.KltPyramids(ctx, rows, cols, 2, 2, 7, 3)      # channels 1 or 3
    assert e.value.code == -1
    pyr = device_batch.KltPyramids(ctx, rows, cols, 1, 2, 7, 3)
    with pytest.raises(api.PsError) as e:
        pyr.build(upload_images(imgs, False), first_slot=1)        # two frames from slot 1 of two
    assert e.value.code == -1
    pyr.close()


@pytest.mark.parametrize("rows,cols,cn,win,levels,padded", [(37, 53, 3, 7, 3, True), (48, 64, 1, 7, 3, False), (96, 128, 1, 31, 7, True),
                                                             (9, 8, 3, 3, 7, False)])
def test_levels_read_back(ctx, rows, cols, cn, win, levels, padded):
    """Every stored level -- image with its REFLECT_101 border, derivative with its border of zeros -- equals the restatement,
    odd sizes and the level at which building stops included."""
    from putslam_amd import device_batch
    rng = np.random.default_rng(rows)
    imgs = [rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8), K.smooth_texture(rows, cols, cn, seed=2)]
    pyr = device_batch.KltPyramids(ctx, rows, cols, cn, 3, win, levels)
    pyr.build(upload_images(imgs, padded), first_slot=1)
    L = K.level_count(rows, cols, win, levels)
    assert pyr.num_levels == L + 1
    for slot, img in ((1, imgs[0]), (2, imgs[1])):
        ref = K.build_pyramid(img, win, levels)
        assert len(ref) == L + 1
        for l, lv in enumerate(ref):
            gi, gd, dims = pyr.level(slot, l)
            assert dims == lv.shape[:2]
            assert np.array_equal(gi, K.pad_image(lv, win)), (slot, l)
            assert np.array_equal(gd, K.pad_deriv(K.scharr(lv), win)), (slot, l)
    from putslam_amd import api
    with pytest.raises(api.PsError):
        pyr.level(1, L + 1)
    pyr.close()


def select_device(ctx, lists, thr, dist):
    """select_tracked over one batch of lists -> per list (kept, matches words, kept points)."""
    import torch
    from putslam_amd import device_batch
    P, cap = len(lists), max(1, max(len(l[0]) for l in lists))
    pts, st, er = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap), np.uint8), np.zeros((P, cap), np.float32)
    for i, (p, s, e) in enumerate(lists):
        pts[i, :len(p)], st[i, :len(p)], er[i, :len(p)] = p, s, e
    dev = torch.device("cuda:0")
    cnt = torch.tensor([len(l[0]) for l in lists], dtype=torch.int32, device=dev)
    m, num, kp, ki = device_batch.select_tracked(ctx, torch.from_numpy(pts).to(dev), torch.from_numpy(st).to(dev),
                                                 torch.from_numpy(er).to(dev), cnt, thr, dist)
    torch.cuda.synchronize()
    m, num, kp, ki = m.cpu().numpy(), num.cpu().numpy(), kp.cpu().numpy(), ki.cpu().numpy()
    return [(ki[i, :num[i]], m[i, :num[i]], kp[i, :num[i]]) for i in range(P)]


def check_selection(got, pts, status, err, thr, dist):
    kept, matches = K.select_pairwise(pts, status, err, thr, dist) if len(pts) <= 400 else K.select_vectorised(pts, status, err, thr, dist)
    gk, gm, gp = got
    assert np.array_equal(gk, kept)
    assert np.array_equal(gm[:, :3], matches) and not gm[:, 3].any()          # (i, j, 0) and the bits of 0.f
    assert u32(gp).tolist() == u32(pts[kept]).tolist()


def test_selection_equals_restatement(ctx):
    """The lists of the host test one by one, then all lists that share a rule as one batch: batched == per pair."""
    cases = K.selection_lists()
    for name, pts, status, err, thr, dist in cases:
        check_selection(select_device(ctx, [(pts, status, err)], thr, dist)[0], pts, status, err, thr, dist)
    same = [c for c in cases if (c[4], c[5]) == (10.0, 1.2)] + [c for c in cases if c[0] in ("random", "empty")]
    got = select_device(ctx, [(c[1], c[2], c[3]) for c in same], 2.5, 4.0)
    for g, c in zip(got, same):
        check_selection(g, c[1], c[2], c[3], 2.5, 4.0)


def test_selection_of_2000_points(ctx):
    rng = np.random.default_rng(21)
    pts = rng.uniform(0, 300, (2000, 2)).astype(np.float32)
    pts[100:140] = pts[60:100]                                                 # exact duplicates
    pts[7] = (np.nan, 3.0)
    err = rng.uniform(0, 4, 2000).astype(np.float32)
    err[200:260] = err[300:360]
    err[11] = np.nan
    status = (rng.uniform(size=2000) < 0.85).astype(np.uint8)
    got = select_device(ctx, [(pts, status, err), (pts[:1025], status[:1025], err[:1025])], 3.0, 6.0)
    check_selection(got[0], pts, status, err, 3.0, 6.0)
    check_selection(got[1], pts[:1025], status[:1025], err[:1025], 3.0, 6.0)


@pytest.mark.parametrize("cn", [1, 3])
def test_host_forms_and_wrappers_equal_the_device_forms(ctx, cn):
    """ps_calc_optical_flow_pyr_lk and ps_perform_tracking (api.Context) on numpy arrays -- one of them a region of a larger image
    -- against ps_klt_track_device + ps_klt_select_device and the restatement."""
    prev, nxt, pts = K.main_scene(cn)
    m = K.MAIN_SCENE
    p = prm(m["win"], m["max_levels"], m["max_count"], m["eps"])
    dn, ds, de = [g[0] for g in run_device(ctx, [prev, nxt], [(0, 1)], [pts], p)]
    big = np.full((prev.shape[0] + 4, prev.shape[1] + 6, cn), 7, np.uint8)
    big[2:-2, 3:-3] = prev
    region = big[2:-2, 3:-3] if cn == 3 else big[2:-2, 3:-3, 0]
    hn, hs, he = ctx.calc_optical_flow_pyr_lk(region, nxt if cn == 3 else nxt[:, :, 0], pts, p)
    assert u32(hn).tolist() == u32(dn).tolist() and np.array_equal(hs, ds) and u32(he).tolist() == u32(de).tolist()
    thr, dist = 3.0, 2.5
    r = ctx.perform_tracking(prev, nxt, pts, thr, dist, p)
    assert u32(r["next_pts"]).tolist() == u32(dn).tolist() and np.array_equal(r["status"], ds) and u32(r["err"]).tolist() == u32(de).tolist()
    got = select_device(ctx, [(dn, ds, de)], thr, dist)[0]
    assert np.array_equal(r["kept_idx"], got[0]) and u32(r["kept_pts"]).tolist() == u32(got[2]).tolist()
    assert np.array_equal(r["matches"]["queryIdx"], got[0]) and np.array_equal(r["matches"]["trainIdx"], np.arange(len(got[0])))
    assert not r["matches"]["imgIdx"].any() and not r["matches"]["distance"].view(np.uint32).any()
    wn, ws, we = ref_track(prev, nxt, pts, p)
    kept, _ = K.select_pairwise(wn, ws, we, thr, dist)
    assert np.array_equal(r["kept_idx"], kept) and 0 < len(kept) < int(ws.sum())
    # under USE_INITIAL_FLOW the host form reads nextPts; no points: nothing to do
    p2 = prm(m["win"], m["max_levels"], m["max_count"], m["eps"], K.USE_INITIAL_FLOW)
    init = (pts + 1.0).astype(np.float32)
    hn2, hs2, he2 = ctx.calc_optical_flow_pyr_lk(prev, nxt, pts, p2, next_pts=init)
    wn2, ws2, we2 = ref_track(prev, nxt, pts, p2, init)
    assert u32(hn2).tolist() == u32(wn2).tolist() and np.array_equal(hs2, ws2) and u32(he2).tolist() == u32(we2).tolist()
    e = ctx.perform_tracking(prev, nxt, np.zeros((0, 2), np.float32), thr, dist, p)
    assert len(e["matches"]) == 0 and len(e["next_pts"]) == 0
