"""The guided map matching kernels held directly to the independent float64 model of tests/match_xyz_model_f64.py (written from
matcher.cpp alone; the oracle and tests/map_l2_ref.py are not consulted here) through its shared check: the host-array entries
(ps_match_xyz, ps_match_xyz_l2_f32), the device batches (ps_match_xyz_device, ps_match_xyz_l2_device) at every number of map
features per wave, and the match rows of ps_map_pairs_device / ps_map_pairs_l2_device."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_xyz_model_f64 as model  # noqa: E402

from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["binary", 64, 128, 20, 65]          # float widths 64 and 128: the group form; 20 and 65: the plain form
LADDER = {k: model.ladder(model.RADIUS, model.RATIO, k) for k in model.TRIES}


def _host(ctx, s, radius, ratio):
    call = ctx.match_xyz if s["map_desc"].dtype == np.uint8 else ctx.match_xyz_l2
    return call(*model.args(s), radius, ratio)


def _host_pitched(ctx, s, radius, ratio, extra):
    """The same call on rows that lie `extra` elements further apart than they are wide (what lies between is never read)."""
    binary = s["map_desc"].dtype == np.uint8
    dim = s["map_desc"].shape[1]

    def wide(d):
        w = np.full((max(len(d), 1), dim + extra), 0xA5 if binary else np.nan, d.dtype)
        w[:len(d), :dim] = d
        return w

    md, cd = wide(s["map_desc"]), wide(s["cur_desc"])
    mp, cp = np.ascontiguousarray(s["map_pos"], np.float32), np.ascontiguousarray(s["cur_pos"], np.float32)
    ml, cl = np.ascontiguousarray(s["map_level"], np.int32), np.ascontiguousarray(s["cur_level"], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    step = md.strides[0]
    cap = 16 * max(len(mp), 1)
    out = np.zeros(cap, DMATCH_DTYPE)
    n = C.c_int(0)
    if binary:
        rc = ctx._L.ps_match_xyz(ctx._h, p(mp), p(md), step, p(ml), len(mp), p(cp), p(cd), step, p(cl), len(cp), radius, ratio, p(out),
                                 cap, C.byref(n))
    else:
        rc = ctx._L.ps_match_xyz_l2_f32(ctx._h, p(mp), p(md), step, p(ml), len(mp), p(cp), p(cd), step, p(cl), len(cp), dim, radius,
                                        ratio, p(out), cap, C.byref(n))
    assert rc == 0 and n.value <= cap
    return out[:n.value].copy()


def _scene(shape, kind):
    """A random scene of the shape; (1, 1): the first seed whose feature has its keypoint as a candidate at try 1."""
    for seed in range(3000 + 7 * shape[0], 3400 + 7 * shape[0]):
        s = model.scene(np.random.default_rng(seed), *shape, kind)
        if shape != (1, 1) or model.match_xyz(*model.args(s), *LADDER[1]).exact:
            return s
    raise AssertionError("no seed gives the single feature a candidate")


# ---------------------------------------------------------------- the host-array entries
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1), (65, 63), (257, 1025)], ids=lambda s: "%dx%d" % s)
def test_host_entries_against_the_model(ctx, shape, kind):
    """ctx.match_xyz / ctx.match_xyz_l2 at tries 1, 5 and 10 of the ladder; try 5 once more with pitched rows."""
    s = _scene(shape, kind)
    total = 0
    for k in model.TRIES:
        r, a = LADDER[k]
        ans = model.match_xyz(*model.args(s), r, a)
        got = _host(ctx, s, r, a)
        rep = model.check(got, ans, (kind, shape, k))
        total += len(got)
        if k == 5:
            again = _host_pitched(ctx, s, r, a, 3)
            model.check(again, ans, (kind, shape, "pitched"))
            assert again.tobytes() == got.tobytes()
        print("%s %s try %d: %d matches, %d / %d ambiguous, worst distance %.2f u" % (kind, shape, k, len(got), rep.ambiguous,
                                                                                    rep.with_candidates, rep.worst_u))
    assert total >= 3 * min(shape) // 2       # (the scenes match: a check of empty lists would say nothing)


@pytest.mark.parametrize("kind", KINDS)
def test_host_entries_on_the_directed_scenes(ctx, kind):
    """15 / 16 / 17 candidates around the stash of 16, candidates at keypoints 1023 and 1024 of 1025 only, a first candidate
    that is not the least, and (binary) ratio x value == bestVal exactly."""
    for name, s, r, a in model.directed(np.random.default_rng(31), kind):
        ans = model.match_xyz(*model.args(s), r, a)
        assert ans.exact and not ans.ambiguous, name
        for got in (_host(ctx, s, r, a), _host_pitched(ctx, s, r, a, 5)):
            model.check(got, ans, (kind, name))
            assert [(int(q), int(t)) for q, t in zip(got["queryIdx"], got["trainIdx"])] == ans.pairs(), (kind, name)


# ---------------------------------------------------------------- device batches
P = 64
FRAME_CAP = 300


def _batch_scene(view_cap, kind):
    """4 views x 4 frames, ragged counts with 0, 1 and the capacity on both sides, 64 pairs of which two name a view / a frame
    outside its set, per-pair radius and ratio from tries 1, 5 and 10 of the ladder."""
    rng = np.random.default_rng(500 + view_cap)
    vcounts = [view_cap, 1, 0, int(0.6 * view_cap)]
    fcounts = [FRAME_CAP, 217, 1, 0]
    source = [0, 1, 0, 1]
    views, frames = model.sets(rng, vcounts, fcounts, view_cap, FRAME_CAP, source, kind)
    pairs = [(v, f) for v in range(4) for f in range(4)] * 4
    pairs[37], pairs[50] = (4, 0), (0, -1)
    tries = [model.TRIES[(p // 16 + p) % 3] for p in range(P)]
    # (pairs (0, 0), (3, 1) and (0, 1) at all three tries)
    for p, (pr, k) in enumerate((((0, 0), 1), ((0, 0), 5), ((0, 0), 10), ((3, 1), 1), ((3, 1), 5), ((3, 1), 10), ((0, 1), 10))):
        pairs[20 + p], tries[20 + p] = pr, k
    return dict(views=views, frames=frames, pairs=np.array(pairs, np.int32), tries=tries,
                radius=[LADDER[k][0] for k in tries], ratio=[LADDER[k][1] for k in tries])


def _device_batch(b, kind, max_matches, pitched=False):
    from putslam_amd.device_batch import FrameSetDevice, FrameSetF32Device, MapBatchDevice, MapBatchF32Device
    v, f = b["views"], b["frames"]
    if kind == "binary":
        vs, fs = FrameSetDevice(v["desc"], v["pos"], v["nkpts"]), FrameSetDevice(f["desc"], f["pos"], f["nkpts"])
        return MapBatchDevice(vs, v["level"], fs, f["level"], b["pairs"], max_matches, radius=b["radius"], ratio=b["ratio"])
    rf = kind + 4 if pitched else None
    vs = FrameSetF32Device(v["desc"], v["pos"], v["nkpts"], row_floats=rf)
    fs = FrameSetF32Device(f["desc"], f["pos"], f["nkpts"], row_floats=rf)
    return MapBatchF32Device(vs, v["level"], fs, f["level"], b["pairs"], max_matches, radius=b["radius"], ratio=b["ratio"])


def _check_batch(b, g, what):
    """Every pair's rows against the model, computed once per distinct (view, frame, try); the cap on ambiguous features over the
    batch's distinct scenes."""
    v, f = b["views"], b["frames"]
    done, amb, cand, total = {}, 0, 0, 0
    for p, (vi, fi) in enumerate(b["pairs"]):
        n = int(g["numMatches"][p])
        if not (0 <= vi < 4 and 0 <= fi < 4):
            assert n == 0, (what, p, n)
            continue
        key = (int(vi), int(fi), b["tries"][p])
        if key not in done:
            done[key] = model.match_xyz(*model.side(v, vi), *model.side(f, fi), b["radius"][p], b["ratio"][p])
            amb, cand = amb + len(done[key].ambiguous), cand + done[key].with_candidates
        ans = done[key]
        assert n >= 0, (what, p, n)
        rep = model.compare(g["matches"][p, :n], ans)
        rep.ambiguous = rep.with_candidates = 0          # (counted per distinct scene, above)
        assert not rep.failures(), (what, p, key, rep.failures())
        if not ans.ambiguous:
            assert n == len(ans.pairs()), (what, p, n)
        total += n
    assert amb <= model.AMBIGUOUS_CAP * cand, (what, amb, cand)
    return total, amb, cand


@pytest.mark.parametrize("kind", ["binary", 64, 20])
@pytest.mark.parametrize("view_cap", [100, 130, 260, 520])
def test_device_batches_against_the_model(ctx, view_cap, kind):
    """run_match_xyz / run_match_xyz_l2 on 64 pairs; the view capacities 100, 130, 260 and 520 select 1, 2, 4 and 8 map features
    per wave (map_features_per_wave: the largest F of 8, 4, 2 with 64 x ceil(capacity / (4 F)) >= 1024)."""
    from putslam_amd.device_batch import run_match_xyz, run_match_xyz_l2
    waves = 4
    F = next((f for f in (8, 4, 2) if P * ((view_cap + waves * f - 1) // (waves * f)) >= 1024), 1)
    assert F == {100: 1, 130: 2, 260: 4, 520: 8}[view_cap]
    b = _batch_scene(view_cap, kind)
    dev = _device_batch(b, kind, 8 * view_cap, pitched=view_cap == 130)
    (run_match_xyz if kind == "binary" else run_match_xyz_l2)(ctx, dev)
    total, amb, cand = _check_batch(b, dev.download(), (kind, view_cap))
    print("%s capacity %d (F = %d): %d matches over 64 pairs, %d / %d features ambiguous" % (kind, view_cap, F, total, amb, cand))
    assert total > 5 * view_cap          # (a check of empty rows would say nothing)


STASH_ORDERS = ((0, 1, 2), (2, 0, 1))          # 15, 16, 17 candidates (model.scene_stash); 17, 15, 16


@functools.lru_cache(maxsize=None)
def _stash_scene(kind):
    """model.scene_stash and, per (order, ratio), the model's answer for its three features in that order."""
    s = model.scene_stash(np.random.default_rng(77), kind)
    answers = {}
    for v, order in enumerate(STASH_ORDERS):
        o = list(order)
        for ratio in (model.RATIO, 0.1):
            answers[v, ratio] = model.match_xyz(s["map_pos"][o], s["map_desc"][o], s["map_level"][o], s["cur_pos"], s["cur_desc"],
                                                s["cur_level"], model.RADIUS, ratio)
    return s, answers


@pytest.mark.parametrize("ratio", [model.RATIO, 0.1])
@pytest.mark.parametrize("kind", ["binary", 64, 20])
@pytest.mark.parametrize("view_cap", [130, 260, 520])
def test_device_batches_sweep_again_beside_stashed_features(ctx, view_cap, kind, ratio):
    """A feature with more candidates than the stash holds (17: swept again from global memory) beside stashed ones (15, 16) in
    ONE wave's chain of output offsets and in the offset of the wave behind it, at 2, 4 and 8 map features per wave: 64 identical
    pairs over one frame of 84 keypoints, the three features in the order 15, 16, 17 and in the order 17, 15, 16."""
    from putslam_amd.device_batch import run_match_xyz, run_match_xyz_l2
    s, answers = _stash_scene(kind)
    ncur = len(s["cur_pos"])
    assert ncur == 84
    views = dict(pos=np.zeros((2, view_cap, 3), np.float32), desc=np.zeros((2, view_cap) + s["map_desc"].shape[1:], s["map_desc"].dtype),
                 level=np.zeros((2, view_cap), np.int32), nkpts=np.array([3, 3], np.int32))
    for v, order in enumerate(STASH_ORDERS):
        o = list(order)
        views["pos"][v, :3], views["desc"][v, :3], views["level"][v, :3] = s["map_pos"][o], s["map_desc"][o], s["map_level"][o]
    frames = dict(pos=s["cur_pos"][None], desc=s["cur_desc"][None], level=s["cur_level"][None], nkpts=np.array([ncur], np.int32))
    for v in range(2):
        ans = answers[v, ratio]
        assert ans.exact and not ans.ambiguous
        want = ans.pairs()
        assert len(want) == (47 if kind == 20 and ratio == model.RATIO else 48)
        b = dict(views=views, frames=frames, pairs=np.tile(np.array([v, 0], np.int32), (P, 1)), radius=[model.RADIUS] * P,
                 ratio=[ratio] * P)
        dev = _device_batch(b, kind, 64)
        (run_match_xyz if kind == "binary" else run_match_xyz_l2)(ctx, dev)
        g = dev.download()
        for p in range(P):
            n = int(g["numMatches"][p])
            assert n == len(want), (kind, view_cap, v, p, n)
            rows = g["matches"][p, :n]
            model.check(rows, ans, (kind, view_cap, v, p))
            assert [(int(q), int(t)) for q, t in zip(rows["queryIdx"], rows["trainIdx"])] == want, (kind, view_cap, v, p)


@pytest.mark.parametrize("kind", ["binary", 64])
def test_map_pairs_match_rows_against_the_model(ctx, kind):
    """run_map_pairs / run_map_pairs_l2: the match rows in front of RANSAC (masks, poses and stats are held by
    tests/test_gpu_map_pairs.py and tests/test_gpu_map_pairs_l2.py)."""
    from putslam_amd.device_batch import run_map_pairs, run_map_pairs_l2
    b = _batch_scene(260, kind)
    dev = _device_batch(b, kind, 8 * 260)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    prm.errorVersionMap = EUCLIDEAN_ERROR
    cfg, _ = make_config(EST_RANSAC, 487, seed=9)
    (run_map_pairs if kind == "binary" else run_map_pairs_l2)(ctx, prm, cfg, TUM_FR1_K, dev)
    total, _, _ = _check_batch(b, dev.download(), ("map pairs", kind))
    assert total > 5 * 260
