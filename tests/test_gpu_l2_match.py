"""The float-descriptor cross-check matcher (ps_match_l2_f32 / ps_match_l2_device / ps_vo_pairs_l2_device) against the restatement of
tests/l2_match_ref.py, as bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l2_match_ref as ref  # noqa: E402

from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import (ADAPTIVE_ERROR, DMATCH_DTYPE, EST_FIXED, EST_RANSAC, EUCLIDEAN_ERROR, REPROJECTION_ERROR, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

f32 = np.float32
STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers",
               "accepted", "bestInlierRatio", "pointInlierRatio")
SIZES = [(0, 5), (5, 0), (1, 1), (31, 33), (32, 32), (33, 31), (64, 65), (65, 64), (129, 257), (257, 129), (513, 513)]


def _pitched(rows, extra=3):
    """The same rows at a pitch of (D + extra) floats, NaN between them."""
    wide = np.full((rows.shape[0], rows.shape[1] + extra), np.nan, f32)
    wide[:, :rows.shape[1]] = rows
    return wide[:, :rows.shape[1]]


def _same(got, want, what=None):
    assert got.dtype == DMATCH_DTYPE and len(got) == len(want), (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), what


def _forms(ctx, q, t, want, what=None):
    """Prefilter + exact (option "matcher_l2" = 1, the default) and the exact sweep (0): the restatement's bytes from both."""
    try:
        for form in (1, 0):
            ctx.set_option("matcher_l2", form)
            _same(ctx.match_l2(q, t), want, (what, form))
            if len(q) and len(t):
                assert ctx.get_option("matcher_l2_used") == (form if q.shape[1] in (64, 128) else 0)
    finally:
        ctx.set_option("matcher_l2", 1)


# ---------------------------------------------------------------- the exact sweep: every dim's tail, ragged sizes, pitched rows
@pytest.mark.parametrize("D", [1, 3, 4, 7, 8, 9, 12, 13, 64, 65, 128, 131, 512])
def test_sweep_equals_the_restatement(ctx, D):
    rng = np.random.default_rng(4000 + D)
    for nq, nt in SIZES:
        q = rng.standard_normal((nq, D)).astype(f32)
        t = rng.standard_normal((nt, D)).astype(f32)
        k = min(nq, nt) // 2
        if k:                                   # near copies: real matches, not only chance ones
            t[:k] = q[rng.permutation(nq)[:k]] + (0.05 * rng.standard_normal((k, D))).astype(f32)
        want = ref.match_l2(q, t)
        _forms(ctx, _pitched(q), _pitched(t, 5), want, (D, nq, nt))
        if (nq, nt) == (129, 257):
            _same(ctx.match_l2(q, t), want, (D, "dense"))


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for kind, make in (("surf", ref.surf_scene), ("sift", ref.sift_scene)):
        q, t = make(513, 511, index=1)
        out[kind] = (q, t, ref.match_l2(q, t))
    return out


@pytest.mark.parametrize("kind", ["surf", "sift"])
def test_scenes_under_every_query_split(ctx, scenes, kind):
    q, t, want = scenes[kind]
    assert len(want) > 250
    try:
        for split in (0, 1, 7, 64):
            ctx.set_option("debug.qsplit", split)
            _forms(ctx, q, t, want, (kind, split))
    finally:
        ctx.set_option("debug.qsplit", 0)


# ---------------------------------------------------------------- directed attacks
def _background(rng, n, D):
    x = rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)


def test_near_ties_at_tile_edges(ctx):
    """Query rows 31 / 32 / 33 and 63 / 64 / 65 are copies of one row with last-ulp perturbations: the least distance, and the
    lowest index among equal ones, must win for every train row."""
    rng = np.random.default_rng(11)
    for D in (64, 128):
        q = _background(rng, 130, D)
        base = _background(rng, 1, D)[0]
        for i, row in enumerate((31, 32, 33, 63, 64, 65)):
            v = base.copy()
            for k in range(i):                  # i elements one ulp up
                v[(7 * k + i) % D] = np.nextafter(v[(7 * k + i) % D], f32(2))
            q[row] = v
        t = _background(rng, 70, D)
        for i in range(40):                     # train rows around the copies, an ulp or a few apart
            v = base.copy()
            for k in rng.integers(0, D, i % 5):
                v[k] = np.nextafter(v[k], f32(2 if i % 2 else -2))
            t[i] = v
        _forms(ctx, q, t, ref.match_l2(q, t), D)


def _sqrt_tie_cases(D, seeds=40):
    """Per seed: a train row t and a query row A; one element of A is nudged towards t an ulp at a time until the restated sum
    drops.  Kept if the dropped sum has the same square-rooted distance: (A, B, t) with L2sqr(t, A) > L2sqr(t, B), equal roots."""
    cases = []
    for seed in range(seeds):
        rng = np.random.default_rng(9000 + seed)
        t = _background(rng, 1, D)[0]
        a = (t + f32(0.3) * _background(rng, 1, D)[0]).astype(f32)
        j = int(rng.integers(0, D))
        steps = np.empty((2048, D), f32)
        v = a.copy()
        for k in range(2048):
            v[j] = np.nextafter(v[j], t[j])
            steps[k] = v
        sums = ref.l2sqr_matrix(t[None, :], steps)[0]
        s0 = ref.l2sqr(t, a)
        drop = np.nonzero(sums < s0)[0]
        if drop.size and np.sqrt(sums[drop[0]]) == np.sqrt(s0):
            cases.append((a, steps[drop[0]].copy(), t))
    return cases


def test_square_root_ties_go_to_the_lower_index(ctx):
    for D in (64, 128):
        cases = _sqrt_tie_cases(D)
        assert len(cases) >= 8, len(cases)
        rng = np.random.default_rng(12)
        for a, b, t in cases:
            # the row with the LARGER sum at the lower index: equal distances, so it must win (a squared-domain minimum takes b)
            q = np.concatenate([_background(rng, 3, D), a[None], _background(rng, 2, D), b[None]])
            tr = np.concatenate([_background(rng, 2, D), t[None]])
            q[[0, 1, 2, 4, 5]] += 1                 # (the background keeps its distance)
            want = ref.match_l2(q, tr)
            assert ref.l2sqr(t, a) > ref.l2sqr(t, b)
            assert (3, 2) in [(int(m["queryIdx"]), int(m["trainIdx"])) for m in want]
            _forms(ctx, q, tr, want)


def test_cancellation(ctx):
    """Norms near 1e3, distances near 1e-3: the Gram form would lose every digit."""
    rng = np.random.default_rng(13)
    for D in (64, 128):
        q, t = _cancellation(rng, D, 200, 190)
        _forms(ctx, q, t, ref.match_l2(q, t), D)


def test_identical_queries_and_degenerate_rows(ctx):
    rng = np.random.default_rng(14)
    for D in (64, 128, 9):
        # 257 identical query rows: every train row takes index 0
        q = np.repeat(_background(rng, 1, D), 257, axis=0)
        t = _background(rng, 40, D)
        want = ref.match_l2(q, t)
        assert len(want) == 1 and want["queryIdx"][0] == 0
        _forms(ctx, q, t, want, D)
        # all-zero and subnormal rows
        q = _background(rng, 70, D)
        t = _background(rng, 66, D)
        q[5] = 0
        t[7] = 0
        q[9] = f32(1e-42) * rng.integers(1, 9, D).astype(f32)
        t[11] = f32(1e-42) * rng.integers(1, 9, D).astype(f32)
        q[13] = f32(3e-23) * rng.integers(1, 9, D).astype(f32)      # squares are subnormal
        t[15] = f32(3e-23) * rng.integers(1, 9, D).astype(f32)
        _forms(ctx, q, t, ref.match_l2(q, t), (D, "zero"))
        # NaN / inf elements, norms that overflow, a train row with no admissible query
        q = _background(rng, 70, D)
        t = _background(rng, 66, D)
        q[3, 0] = np.nan
        q[4, D - 1] = np.inf
        q[6] = f32(3e38)
        q[8] = f32(2e19)
        t[2, 1 % D] = np.nan
        t[5] = f32(-3e38)
        t[9] = f32(2e19)
        t[10, 0] = -np.inf
        t[12] = np.nan
        _forms(ctx, q, t, ref.match_l2(q, t), (D, "nonfinite"))
        q[:] = np.nan
        assert len(ctx.match_l2(q, t)) == 0


# ---------------------------------------------------------------- the prefilter's band and what it hands on
def _cancellation(rng, D, nq, nt):
    c = (rng.standard_normal(D) * 1e3 / np.sqrt(D)).astype(f32)
    q = (c[None, :] + 1e-3 / np.sqrt(D) * rng.standard_normal((nq, D))).astype(f32)
    t = (c[None, :] + 1e-3 / np.sqrt(D) * rng.standard_normal((nt, D))).astype(f32)
    return q, t


@pytest.mark.parametrize("case", ["surf", "sift", "cancel64", "cancel128"])
def test_band_holds(ctx, case):
    """|s~ - S| <= E and |L2sqr - S| <= E for the real-number S (float64 on float32 inputs: its own error, 1e-16 relative, is
    nothing beside E >= 1e-5 relative) on 1024 x 1024 = 2^20 (t, q) per case."""
    if case in ("surf", "sift"):
        q, t = (ref.surf_scene if case == "surf" else ref.sift_scene)(1024, 1024, index=2)
    else:
        q, t = _cancellation(np.random.default_rng(16), int(case[6:]), 1024, 1024)
    st, E = ctx.debug_l2_band(q, t)
    S = np.zeros((1024, 1024))
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    for k in range(q.shape[1]):
        S += (t64[:, k][:, None] - q64[:, k][None, :]) ** 2
    L = ref.l2sqr_matrix(t, q).astype(np.float64)
    E = E.astype(np.float64)
    assert np.all(np.isfinite(st)) and np.all(E > 0)
    w1, w2 = np.abs(st - S) / E, np.abs(L - S) / E
    print(case, "max |s~ - S| / E = %.4f, max |L2sqr - S| / E = %.5f, median E / S = %.3g" % (w1.max(), w2.max(), np.median(E / np.maximum(S, 1e-300))))
    assert w1.max() <= 1.0 and w2.max() <= 1.0


@pytest.mark.parametrize("kind", ["surf", "sift"])
def test_prefilter_filters(ctx, kind):
    """512 x 512: candidate evaluations + nq x (rows swept exactly) <= nq nt / 16, and at least one row takes the prefilter."""
    q, t = (ref.surf_scene if kind == "surf" else ref.sift_scene)(512, 512, index=4)
    ctx.set_option("l2_stats", 1)
    try:
        got = ctx.match_l2(q, t)
        swept, evals, over = ctx.l2_stats()
    finally:
        ctx.set_option("l2_stats", 0)
    assert ctx.get_option("matcher_l2_used") == 1
    _same(got, ref.match_l2(q, t), kind)
    print(kind, "rows swept", swept, "candidate evaluations", evals, "overflowed rows", over)
    assert evals + 512 * swept <= 512 * 512 // 16 and swept < 512 and evals >= 512 - swept


def test_overflowed_lists_are_swept(ctx):
    """257 identical query rows: every list overflows, every row is swept, the answer is index 0."""
    rng = np.random.default_rng(17)
    q = np.repeat(_background(rng, 1, 64), 257, axis=0)
    t = _background(rng, 40, 64)
    ctx.set_option("l2_stats", 1)
    try:
        got = ctx.match_l2(q, t)
        swept, evals, over = ctx.l2_stats()
    finally:
        ctx.set_option("l2_stats", 0)
    _same(got, ref.match_l2(q, t))
    assert (swept, over) == (40, 40) and got["queryIdx"].tolist() == [0]


# ---------------------------------------------------------------- device-resident batches
@pytest.fixture(scope="module")
def ragged():
    """Eight frames of capacity 300, D = 64, linked along a chain; counts include 0, 1 and the capacity."""
    rng = np.random.default_rng(15)
    counts = [300, 0, 1, 63, 65, 300, 257, 129]
    cap, D = 300, 64
    desc = np.full((8, cap, D), np.nan, f32)      # rows beyond a frame's count are never read
    rows = synth.float_rows(rng, cap, "surf")
    for f, n in enumerate(counts):
        truth = np.where(rng.random(cap) < 0.3, -1, rng.permutation(cap))
        rows = synth.float_rows_linked(rng, rows, truth, "surf")
        desc[f, :n] = rows[:n]
    return dict(desc=desc, nkpts=np.array(counts, np.int32), cap=cap, D=D)


def _pairs(P):
    allp = [(a, b) for a in range(8) for b in range(8)]          # includes (f, f) and the empty frame
    extra = [(0, 8), (-1, 0), (9, 9), (5, 100)]                  # frames outside the set: no matches
    return np.array((extra + allp)[:P] if P > 3 else [(0, 5), (3, 3), (6, 8)][:P], np.int32)


def _want(ragged, pair, cache={}):
    a, b = int(pair[0]), int(pair[1])
    if not (0 <= a < 8 and 0 <= b < 8):
        return np.zeros(0, DMATCH_DTYPE)
    if (a, b) not in cache:
        n = ragged["nkpts"]
        cache[(a, b)] = ref.match_l2(ragged["desc"][a, :n[a]], ragged["desc"][b, :n[b]])
    return cache[(a, b)]


@pytest.mark.parametrize("P", [1, 3, 64])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("form", [1, 0])
def test_batches(ctx, ragged, P, strided, form):
    from putslam_amd.device_batch import FrameSetF32Device, PairBatchDevice, run_match_l2
    ctx.set_option("matcher_l2", form)
    fs = FrameSetF32Device(ragged["desc"], None, ragged["nkpts"], row_floats=ragged["D"] + 5 if strided else None)
    pairs = _pairs(P)
    batch = PairBatchDevice(pairs, ragged["cap"])
    for _ in range(2):                                           # twice in a row on one context
        batch.matches.fill_(0xAB)
        batch.num_matches.fill_(-7)
        run_match_l2(ctx, fs, batch)
        g = batch.download()
        for p in range(P):
            want = _want(ragged, pairs[p])
            n = int(g["numMatches"][p])
            assert n == len(want) and g["matches"][p, :n].tobytes() == want.tobytes(), (p, pairs[p])
    ctx.set_option("matcher_l2", 1)
    assert sum(int(x) for x in g["numMatches"]) > 0


@pytest.mark.parametrize("mode,est,H", [(EUCLIDEAN_ERROR, EST_RANSAC, 487), (REPROJECTION_ERROR, EST_FIXED, 1024)])
@pytest.mark.parametrize("kind", ["surf", "sift"])
@pytest.mark.parametrize("form", [1, 0])
def test_vo_pairs(ctx, oracle, mode, est, H, kind, form):
    """ps_vo_pairs_l2_device = the restated matches, then oracle.ransac_rigid3d with seed + p: masks, poses and stats as bytes."""
    from putslam_amd.device_batch import FrameSetF32Device, PairBatchDevice, run_vo_pairs_l2
    seq = synth.make_float_sequence(5, 400, kind=kind, index=21)
    nk = np.array([400, 400, 333, 400, 0], np.int32)
    fs = FrameSetF32Device(seq["fdesc"], seq["pts"], nk)
    pairs = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (1, 1), (0, 7)], np.int32)
    batch = PairBatchDevice(pairs, 400)
    prm = default_ransac_params(mode)
    seed = 4242
    cfg, _ = make_config(est, H, seed=seed)
    ctx.set_option("matcher_l2", form)
    run_vo_pairs_l2(ctx, prm, cfg, TUM_FR1_K, fs, batch)
    ctx.set_option("matcher_l2", 1)
    g = batch.download()
    assert ctx.get_option("matcher_l2_used") == form
    accepted = 0
    for p, (a, b) in enumerate(pairs):
        inside = 0 <= a < 5 and 0 <= b < 5
        m = ref.match_l2(seq["fdesc"][a, :nk[a]], seq["fdesc"][b, :nk[b]]) if inside else np.zeros(0, DMATCH_DTYPE)
        n = int(g["numMatches"][p])
        assert n == len(m) and g["matches"][p, :n].tobytes() == m.tobytes(), p
        cfgp, _ = make_config(est, H, seed=seed + p)
        a_, b_ = (a, b) if inside else (0, 0)
        c = oracle.ransac_rigid3d(prm, cfgp, TUM_FR1_K, seq["pts"][a_], seq["pts"][b_], m)
        assert np.array_equal(c["mask"], g["inlierMask"][p, :n]), p
        assert c["pose"].T.astype(f32).tobytes() == g["pose"][p].tobytes(), p
        for fld in STAT_FIELDS:
            x, y = g["stats"][p][fld], c["stats"][fld]
            assert x == y or (np.isnan(x) and np.isnan(y)), (p, fld, x, y)
        accepted += int(g["stats"][p]["accepted"])
    assert accepted >= 3


@pytest.mark.parametrize("P", [1, 17])
@pytest.mark.parametrize("mode,prune", [(EUCLIDEAN_ERROR, 0), (ADAPTIVE_ERROR, 2), (REPROJECTION_ERROR, 0), (REPROJECTION_ERROR, 2)])
def test_vo_pairs_record_stage_at_its_edges(oracle, mode, prune, P):
    """The record stage of ps_l2_crosscheck for both of its work-group sizes (at most 16 pairs: 1024 threads, more: 256) on frames
    of 1100 key points, so that either size makes more than one trip: an odd number of depth-valid matches under both Euclidean
    error versions, depth-invalid matches on both sides of every tile seam, a pair without a depth-valid match, both record forms
    of the reprojection kernels (complete scoring of a small batch, staged scoring), the staged scoring's counters cleared for
    call after call on one context.  Against the restated matches and oracle.ransac_rigid3d with seed + p."""
    from putslam_amd import api
    from putslam_amd.device_batch import FrameSetF32Device, PairBatchDevice, run_vo_pairs_l2
    seq = synth.make_float_sequence(2, 1100, kind="surf", index=31)
    fdesc, pts = np.concatenate([seq["fdesc"], seq["fdesc"][:1]]), np.concatenate([seq["pts"], seq["pts"][:1]])
    pts[2, :, 2] = 0                                              # frame 2: frame 0 with every depth missing
    fs = FrameSetF32Device(fdesc, pts, np.full(3, 1100, np.int32))
    three = [(0, 1), (2, 1), (1, 0)]
    want = {pr: ref.match_l2(fdesc[pr[0]], fdesc[pr[1]]) for pr in three}
    prm = default_ransac_params(mode)
    seed = 3
    cfg, _ = make_config(EST_FIXED, 1024, seed=seed)
    c2 = api.Context(0)
    c2.set_option("prune", prune)                                 # 2: the staged form whatever the batch size; 0: complete scoring
    valid = {}
    for pairs in ([[pr] for pr in three] if P == 1 else [(three * 6)[:P]] * 2):   # three calls in a row, or the batch twice
        batch = PairBatchDevice(np.array(pairs, np.int32), 1100)
        run_vo_pairs_l2(c2, prm, cfg, TUM_FR1_K, fs, batch)
        g = batch.download()
        if pairs[0][0] != 2:
            assert (c2.get_option("last_staged_pairs") > 0) == (prune == 2)
        for p, (a, b) in enumerate(pairs):
            m, n = want[(a, b)], int(g["numMatches"][p])
            assert n == len(m) and g["matches"][p, :n].tobytes() == m.tobytes(), p
            cfgp, _ = make_config(EST_FIXED, 1024, seed=seed + p)
            c = oracle.ransac_rigid3d(prm, cfgp, TUM_FR1_K, pts[a], pts[b], m)
            assert np.array_equal(c["mask"], g["inlierMask"][p, :n]), p
            assert c["pose"].T.astype(f32).tobytes() == g["pose"][p].tobytes(), p
            for fld in STAT_FIELDS:
                x, y = g["stats"][p][fld], c["stats"][fld]
                assert x == y or (np.isnan(x) and np.isnan(y)), (p, fld, x, y)
            valid[(a, b)] = (int(c["stats"]["numMatchesValid"]), int(c["stats"]["accepted"]))
    c2.close()
    for (a, b), m in want.items():                                # what the inputs are meant to hold
        z0, z1 = pts[a][m["queryIdx"], 2], pts[b][m["trainIdx"], 2]
        bad = ~((z0 >= 0.1) & (z0 <= 6) & (z1 >= 0.1) & (z1 <= 6))
        for seam in (256, 512, 768, 1024):
            assert (bad & (m["queryIdx"] >= seam - 256) & (m["queryIdx"] < seam)).any() and (bad & (m["queryIdx"] >= seam)).any()
    assert valid[(2, 1)] == (0, 0) and any(v % 2 == 1 and ok for v, ok in valid.values())


# ---------------------------------------------------------------- argument errors leave the outputs untouched
def test_argument_errors(ctx, ragged):
    import torch
    from putslam_amd.device_batch import FrameSetF32Device, PairBatchDevice
    L, h = ctx._L, ctx._h
    q = np.zeros((4, 8), f32)
    out = np.full(4, 0x55, np.uint8).repeat(16).view(DMATCH_DTYPE)
    keep = out.tobytes()
    n = C.c_int(9)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def host(nq, qs, nt, ts, dim, o=out, qq=q, tt=q):
        n.value = 9
        return L.ps_match_l2_f32(h, None if qq is None else vp(qq), nq, qs, None if tt is None else vp(tt), nt, ts, dim,
                                 None if o is None else vp(o), C.byref(n))

    for args, code in (((4, 32, 4, 32, 0), -1), ((4, 32, 4, 32, -3), -1), ((-1, 32, 4, 32, 8), -1), ((4, 28, 4, 32, 8), -1),
                       ((4, 32, 4, 16, 8), -1), ((4, 2052, 4, 2052, 513), -5), ((16385, 32, 4, 32, 8), -5)):
        assert host(*args) == code and n.value == 0 and out.tobytes() == keep, args
    assert host(4, 32, 4, 32, 8, qq=None) == -1 and host(4, 32, 4, 32, 8, tt=None) == -1 and host(4, 32, 4, 32, 8, o=None) == -1
    assert host(0, 32, 4, 32, 8) == 0 and n.value == 0 and out.tobytes() == keep

    fs = FrameSetF32Device(ragged["desc"], np.zeros((8, ragged["cap"], 3), f32), ragged["nkpts"])
    batch = PairBatchDevice(_pairs(3), ragged["cap"])
    batch.matches.fill_(0xAB)
    batch.num_matches.fill_(-7)
    batch.pose.fill_(5)
    torch.cuda.synchronize()
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    K = np.ascontiguousarray(TUM_FR1_K, f32)
    res = batch.view().struct()
    D, cap = ragged["D"], ragged["cap"]

    def both(fsx, pairs_ptr, P, code, m_ptr=batch.matches.data_ptr(), n_ptr=batch.num_matches.data_ptr()):
        fsp = None if fsx is None else C.byref(fsx)
        assert L.ps_match_l2_device(h, fsp, C.c_void_p(pairs_ptr), P, C.c_void_p(m_ptr), C.c_void_p(n_ptr)) == code
        assert L.ps_vo_pairs_l2_device(h, C.byref(prm), C.byref(cfg), vp(K), fsp, C.c_void_p(pairs_ptr), P, C.byref(res)) == code
        assert ctx._L.ps_last_error(h) if code else True

    def variant(**kw):
        s = fs.view().struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    pp = batch.pairs.data_ptr()
    both(None, pp, 3, -1)
    both(variant(), pp, -1, -1)
    both(variant(), None, 3, -1)
    both(variant(desc=None), pp, 3, -1)
    both(variant(nkpts=None), pp, 3, -1)
    both(variant(dim=0), pp, 3, -1)
    both(variant(numFrames=0), pp, 3, -1)
    both(variant(maxKpts=0), pp, 3, -1)
    both(variant(descRowStride=D * 4 - 4), pp, 3, -1)
    both(variant(descRowStride=D * 4 + 2), pp, 3, -1)
    both(variant(descFrameStride=cap * D * 4 - 4), pp, 3, -1)
    both(variant(dim=513), pp, 3, -5)
    both(variant(maxKpts=16385), pp, 3, -5)
    both(variant(), pp, 0, 0)
    assert L.ps_match_l2_device(h, C.byref(variant()), C.c_void_p(pp), 3, None, C.c_void_p(batch.num_matches.data_ptr())) == -1
    assert L.ps_vo_pairs_l2_device(h, C.byref(prm), C.byref(cfg), vp(K), C.byref(variant(pts=None)), C.c_void_p(pp), 3, C.byref(res)) == -1
    assert L.ps_vo_pairs_l2_device(h, C.byref(prm), C.byref(cfg), vp(K), C.byref(variant(ptsFrameStride=cap * 12 - 4)), C.c_void_p(pp), 3,
                                   C.byref(res)) == -1
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((batch.matches == 0xAB).all()) and bool((batch.num_matches == -7).all()) and bool((batch.pose == 5).all())
