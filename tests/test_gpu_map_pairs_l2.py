"""Guided map matching for float descriptors (ps_match_xyz_l2_f32 / ps_match_xyz_l2_device / ps_map_pairs_l2_device,
Context.match_xyz_ladder_l2) against the restatement of tests/map_l2_ref.py -- its match list, then oracle.ransac_rigid3d with
seed + p per pair --, as bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_l2_ref as lref  # noqa: E402
import map_pairs_ref as mref  # noqa: E402

from putslam_amd._abi import (DMATCH_DTYPE, EST_FIXED, EST_RANSAC, EUCLIDEAN_ERROR, REPROJECTION_ERROR, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

SEED = 909
LADDER = [mref.ladder_try(0.12, 0.55, k) for k in range(1, 11)]
ESTIMATORS = [(EUCLIDEAN_ERROR, EST_RANSAC, 487), (REPROJECTION_ERROR, EST_FIXED, 256)]


def _sets(views, frames, row_floats=None):
    from putslam_amd.device_batch import FrameSetF32Device
    return (FrameSetF32Device(views["desc"], views["pos"], views["nkpts"], row_floats=row_floats),
            FrameSetF32Device(frames["desc"], frames["pos"], frames["nkpts"], row_floats=row_floats))


def _dev(views, frames, pairs, max_matches, radius=0.12, ratio=0.55, row_floats=None):
    from putslam_amd.device_batch import MapBatchF32Device
    vs, fs = _sets(views, frames, row_floats)
    return MapBatchF32Device(vs, views["level"], fs, frames["level"], pairs, max_matches, radius=radius, ratio=ratio)


def _run(ctx, prm, est, H, seed, batch):
    from putslam_amd.device_batch import run_map_pairs_l2
    cfg, _ = make_config(est, H, seed=seed)
    run_map_pairs_l2(ctx, prm, cfg, TUM_FR1_K, batch)
    return batch.download()


def _matches_only(ctx, batch):
    from putslam_amd.device_batch import run_match_xyz_l2
    run_match_xyz_l2(ctx, batch)
    return batch.download()


def _params(mode):
    prm = default_ransac_params(mode)
    prm.errorVersionMap = mode
    return prm


def _check_lists(g, ref, pairs, radius, ratio, what):
    for p, (v, f) in enumerate(pairs):
        r = radius[p] if np.ndim(radius) else radius
        a = ratio[p] if np.ndim(ratio) else ratio
        m = ref.matches(int(v), int(f), r, a)
        assert int(g["numMatches"][p]) == len(m), (what, p, int(g["numMatches"][p]), len(m))
        assert g["matches"][p, :len(m)].tobytes() == m.tobytes(), (what, p)


# ---------------------------------------------------------------- the ragged scenes: 7 views x 7 frames of maxKpts = 1088
COUNTS = [0, 1, 63, 64, 65, 300, 1025]        # (1025 crosses the sweep's tile of 1024 keypoints)
CAP = 1088


@pytest.fixture(scope="module", params=["surf", "sift"])
def ragged(request, oracle):
    kind = request.param
    rng = np.random.default_rng(20261019 + len(kind))
    frames = lref.make_frames(rng, oracle, COUNTS, CAP, kind)
    views = lref.make_views(rng, frames, [1025, 300, 65, 64, 63, 1, 0], CAP, source=[6, 5, 4, 6, 5, 6, 3], kind=kind, sigma=0.05)
    # 23 pairs: the matching ones, crossings, repeats, and one index outside each set
    pairs = [(0, 6), (1, 5), (2, 4), (3, 6), (4, 5), (5, 6), (6, 3), (0, 5), (1, 6), (2, 0), (0, 1), (3, 2), (4, 3),
             (0, 6), (1, 5), (0, 6), (7, 6), (0, 7), (2, 6), (5, 5), (1, 4), (0, 6), (3, 6)]
    assert len(pairs) == 23
    return dict(kind=kind, views=views, frames=frames, pairs=np.array(pairs, np.int32), ref=lref.Ref(oracle, views, frames))


@pytest.mark.parametrize("mode,est,H", ESTIMATORS)
def test_batches_equal_the_restatement(ctx, ragged, mode, est, H):
    """23 pairs, scalar and per-pair radius / ratio: matches, counts, mask, pose, stats."""
    prm = _params(mode)
    pairs, ref = ragged["pairs"], ragged["ref"]
    per_r = [LADDER[p % 10][0] for p in range(len(pairs))]
    per_a = [LADDER[p % 10][1] for p in range(len(pairs))]
    want_s = ref.batch(prm, est, H, SEED, TUM_FR1_K, pairs, 0.12, 0.55, 4 * CAP)
    want_p = ref.batch(prm, est, H, SEED, TUM_FR1_K, pairs, per_r, per_a, 4 * CAP)
    assert sum(w["numMatches"] > 50 for w in want_s) >= 5 and any(w["numMatches"] == 0 for w in want_s)
    assert want_s[0]["numMatches"] > 300
    for per in (False, True):
        b = _dev(ragged["views"], ragged["frames"], pairs, 4 * CAP, radius=per_r if per else 0.12, ratio=per_a if per else 0.55)
        g = _run(ctx, prm, est, H, SEED, b)
        mref.compare(g, want_p if per else want_s, what=(ragged["kind"], per))


# ---------------------------------------------------------------- other widths and layouts
def _small_scene(oracle, dim, seed=31):
    rng = np.random.default_rng(seed + dim)
    frames = lref.make_frames(rng, oracle, [130, 77], 130, dim)
    views = lref.make_views(rng, frames, [65, 40], 65, source=[0, 1], kind=dim, sigma=0.05)
    return views, frames


class _OffsetSet:
    """A FrameSetF32Device whose descriptor block starts 4 bytes into its allocation (4-byte aligned, not 16)."""

    def __init__(self, fs):
        import torch
        self.fs, self.device = fs, fs.device
        self.num_frames, self.max_kpts, self.dim, self.pts = fs.num_frames, fs.max_kpts, fs.dim, fs.pts
        flat = fs.desc.reshape(-1)
        self.block = torch.full((flat.numel() + 1,), float("nan"), dtype=torch.float32, device=fs.device)
        self.block[1:] = flat
        torch.cuda.synchronize()

    def view(self):
        v = self.fs.view()
        v.desc_ptr = self.block.data_ptr() + 4
        return v


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 7, 8, 20, 63, 64, 65, 127, 128, 129, 512])
def test_other_widths_and_layouts(ctx, oracle, dim):
    """Every width through the plain form (64 and 128 through both): dense rows, pitched rows with NaN between them (a pitch
    that keeps 16-byte alignment and one that does not), and sets whose base is offset by 4 bytes.  The same bytes."""
    from putslam_amd.device_batch import MapBatchF32Device
    views, frames = _small_scene(oracle, dim)
    ref = lref.Ref(oracle, views, frames)
    pairs = np.array([(0, 0), (1, 1), (1, 0), (0, 1)], np.int32)
    rad, rat = [0.12, 0.3, 0.3, 1.0], [0.55, 0.3, 0.1, 0.55]
    assert len(ref.matches(0, 0, 0.12, 0.55)) > 20
    for row_floats in (None, dim + 4, dim + 1):
        g = _matches_only(ctx, _dev(views, frames, pairs, 65 * 130, rad, rat, row_floats=row_floats))
        _check_lists(g, ref, pairs, rad, rat, ("pitch", dim, row_floats))
    vs, fs = _sets(views, frames)
    for ov, of in ((True, False), (False, True), (True, True)):
        b = MapBatchF32Device(_OffsetSet(vs) if ov else vs, views["level"], _OffsetSet(fs) if of else fs, frames["level"], pairs,
                              65 * 130, radius=rad, ratio=rat)
        _check_lists(_matches_only(ctx, b), ref, pairs, rad, rat, ("offset", dim, ov, of))


# ---------------------------------------------------------------- the directed row
def test_directed_row_is_summed_in_blocks_of_four(ctx):
    """[1, 2^-12, 2^-12, 2^-24, 2^-27 x 16] against a zero row as a map feature's only candidate: 0x3f800001 (a sequential
    double sum or a float sum gives 0x3f800000, tests/test_map_l2_host.py)."""
    row = np.array([1.0, 2.0 ** -12, 2.0 ** -12, 2.0 ** -24] + [2.0 ** -27] * 16, np.float32)
    pos = np.array([[0.1, 0.2, 2.0]], np.float32)
    lv = np.array([3], np.int32)
    for md, cd in ((row[None, :], np.zeros((1, 20), np.float32)), (np.zeros((1, 20), np.float32), row[None, :])):
        m = ctx.match_xyz_l2(pos, md, lv, pos, cd, lv, 0.12, 0.55)
        assert len(m) == 1 and (int(m[0]["queryIdx"]), int(m[0]["trainIdx"]), int(m[0]["imgIdx"])) == (0, 0, -1)
        assert m["distance"].view(np.uint32)[0] == 0x3F800001
        assert m.tobytes() == lref.match_xyz_l2(pos, md, lv, pos, cd, lv, 0.12, 0.55).tobytes()
    # the same sum through the group form: the row's 20 elements at the head of a 64-wide one
    wide = np.zeros((1, 64), np.float32)
    wide[0, :20] = row
    m = ctx.match_xyz_l2(pos, wide, lv, pos, np.zeros((1, 64), np.float32), lv, 0.12, 0.55)
    assert len(m) == 1 and m["distance"].view(np.uint32)[0] == 0x3F800001


# ---------------------------------------------------------------- hand-made edges
def _edge_scene(D):
    """Views / frames of capacity 8, one edge per (view v, frame v)."""
    from putslam_amd import api
    V, cap = 9, 8
    vp, fp = np.zeros((V, cap, 3), np.float32), np.zeros((V, cap, 3), np.float32)
    vd, fd = np.zeros((V, cap, D), np.float32), np.zeros((V, cap, D), np.float32)
    vl, fl = np.zeros((V, cap), np.int32), np.zeros((V, cap), np.int32)
    vn, fn = np.zeros(V, np.int32), np.zeros(V, np.int32)
    nan = np.float32(np.nan)
    # 0: keypoints one ulp inside / exactly on the sphere bound of radius 0.12 (and the mirrored points)
    B = np.float32(api.map_sphere_bound(0.12))
    pts, inside = [], 0
    for want, isin in ((B, 0), (np.nextafter(B, np.float32(-np.inf)), 1)):
        q = mref.sphere_edge_points(B, want)
        if q is not None:
            pts += [q, -q]
            inside += 2 * isin
    assert len(pts) == 4
    vn[0], fn[0] = 1, 4
    fp[0, :4] = pts
    # 1: level differences 0, 1, 2 on either side (map level 3)
    vn[1], fn[1] = 1, 5
    vp[1, 0] = fp[1, :5] = [0.1, 0.2, 1.0]
    vl[1, 0] = 3
    fl[1, :5] = [1, 2, 3, 4, 5]
    # 2: NaN at the first candidate: bestVal stays NaN, nothing is emitted
    vn[2], fn[2] = 1, 3
    vp[2, 0] = fp[2, :3] = [0.3, 0.1, 2.0]
    fd[2, 0, D - 1], fd[2, 1, 0], fd[2, 2, 0] = nan, 1.0, 2.0
    # 3: NaN at a later candidate is ignored (values 3, NaN, 4)
    vn[3], fn[3] = 1, 3
    vp[3, 0] = fp[3, :3] = [0.3, 0.1, 2.0]
    fd[3, 0, 0], fd[3, 1, D // 2], fd[3, 2, 0] = 3.0, nan, 4.0
    # 4: a difference that overflows float is +inf; as the only candidate it is emitted at ratio 0.55
    vn[4], fn[4] = 1, 1
    vp[4, 0] = fp[4, 0] = [0.0, 0.0, 3.0]
    vd[4, 0, 1], fd[4, 0, 1] = 3e38, -3e38
    # 5: ratio 0 -- 0 x inf = NaN: the +inf candidates are not emitted, the finite ones are (first candidate +inf)
    vn[5], fn[5] = 1, 4
    vp[5, 0] = fp[5, :4] = [0.0, 0.1, 3.0]
    vd[5, 0, 0] = 3e38
    fd[5, 0, 0], fd[5, 1, 0], fd[5, 2, 0], fd[5, 3, 0] = -3e38, 3e38, -3e38, 2.9e38
    # 6: equal rows: value 0, emitted (both of them)
    vn[6], fn[6] = 1, 2
    vp[6, 0] = fp[6, :2] = [0.2, 0.2, 1.0]
    vd[6, 0] = fd[6, 0] = fd[6, 1] = np.arange(D, dtype=np.float32) * np.float32(0.37)
    # 7: ratio x value == best exactly (ratio 0.5: values 4, 2 (best), 8, 4)
    vn[7], fn[7] = 1, 4
    vp[7, 0] = fp[7, :4] = [0.5, 0.5, 1.5]
    for i, x in enumerate((4.0, 2.0, 8.0, 4.0)):
        fd[7, i, (5 * i) % D] = x
    # 8: nothing on either side
    views = dict(pos=vp, desc=vd, level=vl, nkpts=vn, cap=cap)
    frames = dict(pos=fp, desc=fd, level=fl, nkpts=fn, cap=cap)
    return views, frames, inside


@pytest.mark.parametrize("D", [64, 20, 128])
def test_value_edges(ctx, oracle, D):
    views, frames, inside = _edge_scene(D)
    ref = lref.Ref(oracle, views, frames)
    pairs = np.array([(v, v) for v in range(9)] + [(8, 0), (0, 8), (5, 5)], np.int32)
    ratio = [0.55, 0.55, 0.55, 0.55, 0.55, 0.0, 0.55, 0.5, 0.55, 0.55, 0.55, 0.55]
    prm = _params(EUCLIDEAN_ERROR)
    want = ref.batch(prm, EST_RANSAC, 487, 1, TUM_FR1_K, pairs, 0.12, ratio, 64)
    # the scene does what it was made for
    trains = lambda w: [int(t) for t in w["matches"]["trainIdx"]]          # noqa: E731
    assert want[0]["numMatches"] == inside == 2
    assert trains(want[1]) == [1, 2, 3]
    assert want[2]["numMatches"] == 0
    assert trains(want[3]) == [0, 2] and want[3]["matches"]["distance"].tolist() == [3.0, 4.0]
    assert trains(want[4]) == [0] and np.isposinf(want[4]["matches"]["distance"][0])
    assert trains(want[5]) == [1, 3] and want[5]["matches"]["distance"][0] == 0.0
    assert trains(want[6]) == [0, 1] and want[6]["matches"]["distance"].tolist() == [0.0, 0.0]
    assert trains(want[7]) == [0, 1, 3] and want[7]["matches"]["distance"].tolist() == [4.0, 2.0, 4.0]
    assert trains(want[11]) == [1]              # (the same list at ratio 0.55: the first candidate is +inf, the best is 0)
    g = _run(ctx, prm, EST_RANSAC, 487, 1, _dev(views, frames, pairs, 64, ratio=ratio))
    mref.compare(g, want, what=("edges", D))


# ---------------------------------------------------------------- more candidates than the short list holds; multi-emit
@pytest.fixture(scope="module", params=["surf", "sift"])
def square(request, oracle):
    kind = request.param
    rng = np.random.default_rng(4040 + len(kind))
    frames = lref.make_frames(rng, oracle, [500], 500, kind)
    views = lref.make_views(rng, frames, [500], 500, source=[0], kind=kind, sigma=0.05)
    return dict(kind=kind, views=views, frames=frames, ref=lref.Ref(oracle, views, frames))


def _counts(s, radius, ratio):
    v, f = s["views"], s["frames"]
    return lref.match_xyz_l2(v["pos"][0], v["desc"][0], v["level"][0], f["pos"][0], f["desc"][0], f["level"][0], radius, ratio,
                             return_counts=True)


def test_more_than_16_candidates(ctx, square):
    """500 x 500 with radius 1.0, ratio 0.55: more than half of the features have more candidates than the 16 places hold
    (up to about 45) and are swept again."""
    m, cand = _counts(square, 1.0, 0.55)
    print("%s: %d of 500 features beyond 16 candidates, %d at most" % (square["kind"], int((cand > 16).sum()), int(cand.max())))
    assert (cand > 16).sum() > 200 and (cand <= 16).sum() > 50 and cand.max() > 35
    prm = _params(EUCLIDEAN_ERROR)
    pairs = np.array([(0, 0)] * 3, np.int32)
    rad, rat = [1.0, 1.0, 0.12], [0.55, 0.9, 0.55]
    want = square["ref"].batch(prm, EST_RANSAC, 487, 3, TUM_FR1_K, pairs, rad, rat, 8000)
    assert want[0]["numMatches"] == len(m)
    g = _run(ctx, prm, EST_RANSAC, 487, 3, _dev(square["views"], square["frames"], pairs, 8000, rad, rat))
    mref.compare(g, want, what=("beyond 16", square["kind"]))


@pytest.mark.parametrize("kind", ["surf", "sift", 20])
def test_one_feature_sees_a_whole_frame(ctx, oracle, kind):
    """A one-feature view with radius 10 against 1100 keypoints (across the tile of 1024), every level admitted or not; and a
    view of 70 features whose rows all equal the frame's: nmap x candidates matches of value 0."""
    rng = np.random.default_rng(8)
    frames = lref.make_frames(rng, oracle, [1100], 1100, kind)
    views = lref.make_views(rng, frames, [1, 70], 70, source=[0, 0], kind=kind)
    views["desc"][1, :70] = frames["desc"][0, 0]
    frames["desc"][0, 500:] = frames["desc"][0, 0]
    ref = lref.Ref(oracle, views, frames)
    pairs = np.array([(0, 0), (1, 0), (0, 0)], np.int32)
    rad, rat = [10.0, 10.0, 10.0], [0.1, 0.55, 1.0]
    prm = _params(EUCLIDEAN_ERROR)
    cap = 70 * 1100
    want = ref.batch(prm, EST_RANSAC, 487, 2, TUM_FR1_K, pairs, rad, rat, cap)
    assert want[0]["numMatches"] > 100 and want[1]["numMatches"] > 70 * 100
    g = _run(ctx, prm, EST_RANSAC, 487, 2, _dev(views, frames, pairs, cap, rad, rat))
    mref.compare(g, want, what=("whole frame", kind))


def test_multi_emit(ctx, square):
    """Radius 0.30, ratio 0.10: a third of the features emit more than one match."""
    m, _ = _counts(square, 0.30, 0.10)
    per = np.bincount(m["queryIdx"], minlength=500)
    print("%s: %d of 500 features with more than one match" % (square["kind"], int((per > 1).sum())))
    assert (per > 1).sum() > 100
    prm = _params(REPROJECTION_ERROR)
    pairs = np.array([(0, 0)], np.int32)
    want = square["ref"].batch(prm, EST_FIXED, 256, 5, TUM_FR1_K, pairs, 0.30, 0.10, 4000)
    g = _run(ctx, prm, EST_FIXED, 256, 5, _dev(square["views"], square["frames"], pairs, 4000, 0.30, 0.10))
    mref.compare(g, want, what=("multi-emit", square["kind"]))


# ---------------------------------------------------------------- capacity
def test_capacity(ctx, ragged):
    """maxMatches below some pairs' counts: those report -(count) and give the estimator nothing, their neighbours equal the
    restatement; a second call with the reported capacity is exact; the host call returns the needed capacity."""
    prm = _params(EUCLIDEAN_ERROR)
    views, frames, ref = ragged["views"], ragged["frames"], ragged["ref"]
    pairs = ragged["pairs"]
    r10, a10 = LADDER[9]
    cap = 300
    want = ref.batch(prm, EST_RANSAC, 487, SEED, TUM_FR1_K, pairs, r10, a10, cap)
    over = [p for p, w in enumerate(want) if w["numMatches"] < 0]
    assert 3 <= len(over) < len(pairs)
    g = _run(ctx, prm, EST_RANSAC, 487, SEED, _dev(views, frames, pairs, cap, r10, a10))
    mref.compare(g, want, what="capacity")
    for p in over:
        assert g["pose"][p].tolist() == np.eye(4, dtype=np.float32).reshape(16).tolist()
        assert g["stats"][p]["accepted"] == 0 and g["stats"][p]["numInliers"] == 0 and g["stats"][p]["numMatchesIn"] == 0
    need = int(-g["numMatches"].min())
    assert need > cap
    want2 = ref.batch(prm, EST_RANSAC, 487, SEED, TUM_FR1_K, pairs, r10, a10, need)
    assert all(w["numMatches"] >= 0 for w in want2)
    g2 = _run(ctx, prm, EST_RANSAC, 487, SEED, _dev(views, frames, pairs, need, r10, a10))
    mref.compare(g2, want2, what="second call")
    # ps_match_xyz_l2_f32 with a short cap: PS_ERR_BAD_ARG and the needed capacity
    import ctypes as C
    mp, md, ml = ref.side(views, 0)
    cp, cd, cl = ref.side(frames, 6)
    full = ref.matches(0, 6, r10, a10)
    out = np.zeros(8, DMATCH_DTYPE)
    n = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    args = (ctx._h, p(mp), p(md), md.shape[1] * 4, p(ml), len(mp), p(cp), p(cd), cd.shape[1] * 4, p(cl), len(cp), md.shape[1],
            r10, a10)
    assert ctx._L.ps_match_xyz_l2_f32(*args, p(out), 8, C.byref(n)) == -1 and n.value == len(full) > 8
    assert ctx._L.ps_match_xyz_l2_f32(*args, None, 0, C.byref(n)) == -1 and n.value == len(full)
    big = np.zeros(len(full), DMATCH_DTYPE)
    assert ctx._L.ps_match_xyz_l2_f32(*args, p(big), len(big), C.byref(n)) == 0 and n.value == len(full)
    assert big.tobytes() == full.tobytes()


# ---------------------------------------------------------------- the three forms agree
def test_forms_agree(ctx, ragged):
    """ps_match_xyz_l2_device alone equals ps_match_xyz_l2_f32 per pair; match_xyz_l2 + ransac_rigid3d one by one equal the
    batch; frame sets with pitched rows (a packed stride) give the same batch."""
    prm = _params(EUCLIDEAN_ERROR)
    views, frames, ref = ragged["views"], ragged["frames"], ragged["ref"]
    pairs = ragged["pairs"]
    inside = [p for p, (v, f) in enumerate(pairs) if v < 7 and f < 7]
    alone = _matches_only(ctx, _dev(views, frames, pairs, 4 * CAP, 0.16, 0.45))
    g = _run(ctx, prm, EST_RANSAC, 487, SEED, _dev(views, frames, pairs, 4 * CAP, 0.16, 0.45))
    D = views["desc"].shape[2]
    packed = _run(ctx, prm, EST_RANSAC, 487, SEED, _dev(views, frames, pairs, 4 * CAP, 0.16, 0.45, row_floats=D + 12))
    for k in ("numMatches", "pose", "stats"):
        assert packed[k].tobytes() == g[k].tobytes(), k
    assert alone["numMatches"].tobytes() == g["numMatches"].tobytes()
    for p in range(len(pairs)):
        n = int(g["numMatches"][p])
        assert alone["matches"][p, :n].tobytes() == g["matches"][p, :n].tobytes(), p
        assert packed["matches"][p, :n].tobytes() == g["matches"][p, :n].tobytes(), p
        assert packed["inlierMask"][p, :n].tobytes() == g["inlierMask"][p, :n].tobytes(), p
    for p in inside:
        v, f = pairs[p]
        mp, md, ml = ref.side(views, v)
        cp, cd, cl = ref.side(frames, f)
        m = ctx.match_xyz_l2(mp, md, ml, cp, cd, cl, 0.16, 0.45)
        assert m.tobytes() == ref.matches(int(v), int(f), 0.16, 0.45).tobytes(), p
        cfg, _ = make_config(EST_RANSAC, 487, seed=SEED + p)
        r = ctx.ransac_rigid3d(prm, cfg, TUM_FR1_K, mp, cp, m)
        one = dict(numMatches=len(m), matches=m, mask=r["mask"][:len(m)], pose=np.ascontiguousarray(r["pose"].T).reshape(16),
                   stats=r["stats"])
        mref.compare(g, [one], lo=p, what="one by one")
    # a sub-batch [a, b) seeded seed + a equals its slice of the whole batch
    a, b = 5, 16
    s = _run(ctx, prm, EST_RANSAC, 487, SEED + a, _dev(views, frames, pairs[a:b], 4 * CAP, 0.16, 0.45))
    for k in ("numMatches", "pose", "stats"):
        assert s[k].tobytes() == g[k][a:b].tobytes(), k


# ---------------------------------------------------------------- the retry ladder
@pytest.mark.parametrize("shift,sigma,later", [(0.15, 0.01, True), (0.0, 0.02, False), (40.0, 0.02, None)])
def test_ladder_python(ctx, oracle, shift, sigma, later):
    """Context.match_xyz_ladder_l2 against ten restated tries (tests/map_l2_ref.py + the oracle's estimator, seed S + k - 1):
    a displaced scene takes a later try, an undisplaced one the first, a scene 40 m away the tenth."""
    rng = np.random.default_rng(11)
    frames = lref.make_frames(rng, oracle, [900], 900, "surf")
    views = lref.make_views(rng, frames, [800], 800, source=[0], kind="surf", sigma=sigma, shift=shift)
    ref = lref.Ref(oracle, views, frames)
    prm = _params(EUCLIDEAN_ERROR)
    S = 4242
    cfg, _ = make_config(EST_RANSAC, 487, seed=S)
    tries = [ref.pair(prm, EST_RANSAC, 487, S + k, TUM_FR1_K, 0, 0, LADDER[k][0], LADDER[k][1], 1 << 20) for k in range(10)]
    ratios = [float(t["stats"]["pointInlierRatio"]) for t in tries]
    k = mref.ladder_pick(ratios)
    if later is True:
        assert 0 < k
    elif later is False:
        assert k == 0
    else:
        assert k == 9 and all((-1.0 if r != r else r) < 0.1 for r in ratios)
    args = (views["pos"][0], views["desc"][0], views["level"][0], frames["pos"][0], frames["desc"][0], frames["level"][0], prm, cfg,
            TUM_FR1_K)
    got = ctx.match_xyz_ladder_l2(*args, radius=0.12, ratio=0.55, max_matches=16 * 800)
    assert got["try_used"] == k + 1, (got["try_used"], ratios)
    assert got["matches"].tobytes() == tries[k]["matches"].tobytes()
    assert got["mask"].tobytes() == tries[k]["mask"].tobytes()
    assert np.ascontiguousarray(got["pose"].T).reshape(16).astype(np.float32).tobytes() == tries[k]["pose"].astype(np.float32).tobytes()
    assert mref.canon_stats(got["stats"]) == mref.canon_stats(tries[k]["stats"])
    assert got["inlier_ratio"] == (-1.0 if ratios[k] != ratios[k] else ratios[k])
    # rows too small for the tries: the call runs again with the reported capacity and returns the same try
    small = ctx.match_xyz_ladder_l2(*args, radius=0.12, ratio=0.55, max_matches=16)
    assert small["try_used"] == got["try_used"] and small["num_matches"] == got["num_matches"]
    assert small["matches"].tobytes() == got["matches"].tobytes() and small["mask"].tobytes() == got["mask"].tobytes()
    assert small["pose"].tobytes() == got["pose"].tobytes() and mref.canon_stats(small["stats"]) == mref.canon_stats(got["stats"])


# ---------------------------------------------------------------- one context, the binary call around the float call
def test_sharing_a_context_with_the_binary_call(ctx, oracle, ragged):
    from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice, run_map_pairs
    prm = _params(EUCLIDEAN_ERROR)
    rng = np.random.default_rng(5)
    bframes = mref.make_frames(rng, oracle, [700, 333], 700)
    bviews = mref.make_views(rng, bframes, [600, 300], 700, source=[0, 1])
    bpairs = np.array([(0, 0), (1, 1), (0, 1), (1, 0)] * 4, np.int32)
    cfg, _ = make_config(EST_RANSAC, 487, seed=77)

    def binary():
        vs = FrameSetDevice(bviews["desc"], bviews["pos"], bviews["nkpts"])
        fs = FrameSetDevice(bframes["desc"], bframes["pos"], bframes["nkpts"])
        b = MapBatchDevice(vs, bviews["level"], fs, bframes["level"], bpairs, 2800)
        run_map_pairs(ctx, prm, cfg, TUM_FR1_K, b)
        return b.download()

    first = binary()
    assert int(first["numMatches"][0]) > 100
    pairs = ragged["pairs"]
    want = ragged["ref"].batch(prm, EST_RANSAC, 487, SEED, TUM_FR1_K, pairs, 0.12, 0.55, 4 * CAP)
    g = _run(ctx, prm, EST_RANSAC, 487, SEED, _dev(ragged["views"], ragged["frames"], pairs, 4 * CAP))
    mref.compare(g, want, what="between binary calls")
    second = binary()
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    assert ctx.debug_keys_clean() == 0


# ---------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_outputs_alone(ctx, ragged):
    import torch
    from putslam_amd import api
    prm = _params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    b = _dev(ragged["views"], ragged["frames"], ragged["pairs"][:4], 64)
    D = ragged["views"]["desc"].shape[2]
    for t in (b.matches, b.mask, b.stats):
        t.fill_(0xA5)
    b.num_matches.fill_(-77)
    b.pose.fill_(3.5)
    torch.cuda.synchronize()

    def expect(code, mutate):
        bv, out = b.batch_view(), b.view()
        mutate(bv, out)
        with pytest.raises(api.PsError) as e:
            ctx.map_pairs_l2_device(prm, cfg, TUM_FR1_K, bv, out)
        assert e.value.code == code, (e.value, code)
        assert len(str(e.value)) > 25
        with pytest.raises(api.PsError) as e2:
            ctx.match_xyz_l2_device(bv, out.matches_ptr, out.num_matches_ptr)
        assert e2.value.code == code

    BAD, UNSUP = -1, -5
    expect(BAD, lambda bv, o: setattr(bv, "P", -1))
    expect(BAD, lambda bv, o: setattr(bv, "max_matches", 0))
    expect(UNSUP, lambda bv, o: setattr(bv, "max_matches", (1 << 22) + 1))
    expect(BAD, lambda bv, o: setattr(bv, "pairs_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv, "map_level_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv, "cur_level_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv.maps, "dim", 0))
    expect(BAD, lambda bv, o: setattr(bv.frames, "dim", 0))
    expect(UNSUP, lambda bv, o: setattr(bv.maps, "dim", 513))
    expect(UNSUP, lambda bv, o: setattr(bv.frames, "dim", 513))
    expect(BAD, lambda bv, o: (setattr(bv.maps, "dim", D // 2), setattr(bv.maps, "row_stride", D * 4)))       # unequal dims
    expect(UNSUP, lambda bv, o: setattr(bv.maps, "max_kpts", 16385))
    expect(UNSUP, lambda bv, o: setattr(bv.frames, "max_kpts", 16385))
    expect(BAD, lambda bv, o: setattr(bv.frames, "row_stride", D * 4 - 4))
    expect(BAD, lambda bv, o: setattr(bv.frames, "row_stride", D * 4 + 2))
    expect(BAD, lambda bv, o: setattr(bv.maps, "desc_stride", CAP * D * 4 - 4))
    expect(BAD, lambda bv, o: setattr(bv.maps, "pts_stride", CAP * 12 - 4))
    expect(BAD, lambda bv, o: setattr(bv.maps, "desc_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv.maps, "pts_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv.frames, "pts_ptr", None))
    expect(BAD, lambda bv, o: setattr(bv.frames, "nkpts_ptr", None))
    expect(BAD, lambda bv, o: setattr(o, "matches_ptr", None))
    with pytest.raises(api.PsError) as e:        # outputs of the RANSAC half, explicit sample streams, a null batch
        o = b.view()
        o.pose_ptr = None
        ctx.map_pairs_l2_device(prm, cfg, TUM_FR1_K, b.batch_view(), o)
    assert e.value.code == BAD
    cfg2, keep = make_config(EST_RANSAC, 487, seed=1, sample_idx=np.zeros((487, 3), np.uint32))
    with pytest.raises(api.PsError) as e:
        ctx.map_pairs_l2_device(prm, cfg2, TUM_FR1_K, b.batch_view(), b.view())
    assert e.value.code == BAD
    assert ctx._L.ps_match_xyz_l2_device(ctx._h, None, None, None) == BAD
    assert ctx._L.ps_map_pairs_l2_device(ctx._h, None, None, None, None, None) == BAD
    # P == 0 is fine and does nothing
    bv = b.batch_view()
    bv.P = 0
    ctx.map_pairs_l2_device(prm, cfg, TUM_FR1_K, bv, b.view())
    ctx.match_xyz_l2_device(bv, b.matches.data_ptr(), b.num_matches.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((b.matches == 0xA5).all()) and bool((b.mask == 0xA5).all()) and bool((b.stats == 0xA5).all())
    assert bool((b.num_matches == -77).all()) and bool((b.pose == 3.5).all())
    # the host call's arguments
    import ctypes as C
    n = C.c_int(5)
    z = np.zeros((4, 8), np.float32)
    zi = np.zeros(4, np.int32)
    out = np.zeros(16, DMATCH_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def host(dim, step=32, mpos=z, nout=n):
        return ctx._L.ps_match_xyz_l2_f32(ctx._h, p(mpos) if mpos is not None else None, p(z), step, p(zi), 4, p(z), p(z), step, p(zi), 4,
                                          dim, 0.12, 0.55, p(out), 16, C.byref(nout) if nout is not None else None)

    assert host(0) == BAD and n.value == 0
    assert host(513, 513 * 4) == UNSUP
    assert host(8, 28) == BAD
    assert host(8, mpos=None) == BAD
    assert host(8, nout=None) == BAD
    assert host(8) == 0 and n.value == 16         # (zero positions, levels and rows: every row is a candidate of every row)

    # ... and the binary host call's (ps_match_xyz, the same host form): more than PS_MAX_KPTS rows on a side; a capacity that
    # is too small reports the needed one and leaves `out` alone
    def host_bin(nmap, ncur, cap, outbuf):
        zp, zd, zl = np.zeros((max(nmap, ncur), 3), np.float32), np.zeros((max(nmap, ncur), 32), np.uint8), np.zeros(max(nmap, ncur), np.int32)
        return ctx._L.ps_match_xyz(ctx._h, p(zp), p(zd), 32, p(zl), nmap, p(zp), p(zd), 32, p(zl), ncur, C.c_double(0.12), C.c_double(0.55),
                                   p(outbuf), cap, C.byref(n))

    n.value = 5
    assert host_bin(16385, 1, 16, out) == UNSUP and n.value == 0
    assert host_bin(1, 16385, 16, out) == UNSUP and n.value == 0
    kept = np.full(16 * DMATCH_DTYPE.itemsize, 0xA5, np.uint8).view(DMATCH_DTYPE)
    before = kept.tobytes()
    assert host_bin(2, 2, 0, kept) == BAD and n.value == 4  # (every row is a candidate of every row)
    assert kept.tobytes() == before
