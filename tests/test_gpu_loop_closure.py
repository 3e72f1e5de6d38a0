"""Loop-closure candidates verified in one batch from the resident store (ps_pose_sets_device, ps_loop_pairs_device,
Context.verify_loop_closures) against the sequential restatement of tests/loop_closure_ref.py and the CPU oracle, byte for
byte: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_ref as lref  # noqa: E402

from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, PS_SET_INVALID, REPROJECTION_ERROR, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

SENTINEL = (0x5A, -123.0)
H_LC = 1157          # the loop-closure config's cap on the hypotheses


def _build(ctx, store, p3d, poses, cap, packed=None, side=True, fill=False, sd=None):
    from putslam_amd.device_batch import PoseSetsDevice, build_pose_sets
    sd = lref.store_device(store) if sd is None else sd
    out = None
    if fill:
        out = PoseSetsDevice(len(poses), cap, sd.device, packed, side)
        for t in ((out.blocks,) if packed else (out.desc,)) + ((out.feat_idx, out.obs_idx) if side else ()):
            t.fill_(SENTINEL[0])
        if not packed:
            out.pts.fill_(SENTINEL[1])
        out.set_count.fill_(77)
        out.nkpts.fill_(77)
    return build_pose_sets(ctx, sd, p3d, poses, cap, packed_stride=packed, side_arrays=side, out=out)


# ---------------------------------------------------------------- pose sets
@pytest.mark.parametrize("F,N,max_obs,packed", [(2000, 40, 12, False), (1500, 30, 8, True), (257, 5, 5, False), (90, 3, 3, True)])
def test_random_stores_equal_the_restatement(ctx, F, N, max_obs, packed):
    rng = np.random.default_rng(F * 31 + N)
    store, p3d = lref.make_scene(rng, F, N, max_obs=max_obs)
    poses = rng.permutation(N).astype(np.int32)
    want = lref.pose_sets(store, p3d, poses, F)
    counts = [w["setCount"] for w in want]
    assert max(counts) > F // 8 and len(set(counts)) > 1, counts
    stride = (F * 44 + 15) // 16 * 16 + 256 if packed else None
    got = _build(ctx, store, p3d, poses, F, packed=stride, fill=not packed).download()
    lref.compare_sets(got, want, sentinel=None if packed else SENTINEL, what=(F, N))


def _edge_scene():
    """Member counts of 0, 1, 255, 256, 257 and 513 on poses nobody else observed from: one short of a chunk, a chunk whose 256
    features all belong to one set, one more than a chunk (across a chunk edge), two chunks and one (across three)."""
    rng = np.random.default_rng(513)
    store, p3d = lref.make_scene(rng, 1100, 4, max_obs=3, extra_poses=8)
    feats = lref.unpack(store, p3d)
    lref.observe(rng, feats, 5, [1099])
    lref.observe(rng, feats, 6, range(0, 255))
    lref.observe(rng, feats, 7, range(256, 512))
    lref.observe(rng, feats, 8, range(255, 512))
    lref.observe(rng, feats, 9, range(300, 813))
    store, p3d = lref.pack(store, feats)
    return store, p3d, np.array([4, 5, 6, 7, 8, 9, 1, 7], np.int32)


def test_chunk_and_wave_edges_overflow_and_untouched_rows(ctx):
    store, p3d, poses = _edge_scene()
    want = lref.pose_sets(store, p3d, poses, 1100)
    assert [w["setCount"] for w in want][:6] == [0, 1, 255, 256, 257, 513]
    assert (want[3]["rows"]["featIdx"] == np.arange(256, 512)).all() and lref.sets_equal(want[3], want[7])     # (pose 7 twice)
    lref.compare_sets(_build(ctx, store, p3d, poses, 1100, fill=True).download(), want, SENTINEL, "edges")
    # capacity 256: the sets of 257 and 513 report -(count), their rows and everybody else's rows beyond the count stay untouched
    want = lref.pose_sets(store, p3d, poses, 256)
    assert [w["setCount"] for w in want][:6] == [0, 1, 255, 256, -257, -513]
    lref.compare_sets(_build(ctx, store, p3d, poses, 256, fill=True).download(), want, SENTINEL, "overflow")
    lref.compare_sets(_build(ctx, store, p3d, poses, 256, side=False, fill=True).download(), want, SENTINEL, "no side arrays")


def test_one_chunk_touching_a_hundred_sets_and_the_set_limits(ctx):
    from putslam_amd import api
    rng = np.random.default_rng(64)
    store, p3d = lref.make_scene(rng, 600, 100, max_obs=12)
    poses = np.arange(100, dtype=np.int32)
    want = lref.pose_sets(store, p3d, poses, 600)
    assert sum(w["nkpts"] > 0 and (w["rows"]["featIdx"] < 256).any() for w in want) > 64
    sd = lref.store_device(store)
    lref.compare_sets(_build(ctx, store, p3d, poses, 600, sd=sd).download(), want, what="100 sets")
    # S = 1, S = PS_LOOP_MAX_SETS (every pose listed ten times: chains), S + 1 refused with nothing written
    lref.compare_sets(_build(ctx, store, p3d, poses[17:18], 600, sd=sd, fill=True).download(), want[17:18], SENTINEL, "S = 1")
    many = (np.arange(1024) % 100).astype(np.int32)
    lref.compare_sets(_build(ctx, store, p3d, many, 200, sd=sd).download(), lref.pose_sets(store, p3d, many, 200), what="S = 1024")
    with pytest.raises(api.PsError) as e:
        _build(ctx, store, p3d, np.zeros(1025, np.int32), 8, sd=sd)
    assert e.value.code == -5
    from putslam_amd.device_batch import PoseSetsDevice
    for cap in (16385, 0):                                         # PS_MAX_KPTS + 1: unsupported; no capacity: a bad argument
        small = PoseSetsDevice(1, 8, sd.device)
        small.max_kpts = cap
        with pytest.raises(api.PsError) as e:
            _build_into(ctx, sd, p3d, poses[:1], small)
        assert e.value.code == (-5 if cap else -1)
    short = PoseSetsDevice(1, 8, sd.device)
    short.num_frames = 1                                           # numFrames < S + 1
    with pytest.raises(api.PsError) as e:
        _build_into(ctx, sd, p3d, poses[:1], short)
    assert e.value.code == -1


def _build_into(ctx, sd, p3d, poses, out):
    from putslam_amd.device_batch import build_pose_sets
    return build_pose_sets(ctx, sd, p3d, poses, out.max_kpts, out=out)


def test_bad_pose_ids_foreign_observations_and_a_malformed_index(ctx):
    rng = np.random.default_rng(99)
    store, p3d = lref.make_scene(rng, 700, 12, max_obs=6, extra_poses=1)          # pose 12: no observation
    store["obs_pose"][rng.choice(len(store["obs_pose"]), 40, replace=False)] = np.tile([13, -2, 2 ** 30, -2 ** 31], 10)
    f = int(np.nonzero(np.diff(store["obs_start"]) >= 3)[0][5])
    o = int(store["obs_start"][f])
    store["obs_pose"][o:o + 3] = [4, 4, 4]                                        # malformed: the first observation is taken
    poses = np.array([3, 3, 12, -1, 13, 4, -2 ** 31, 2 ** 31 - 1, 0], np.int32)
    want = lref.pose_sets(store, p3d, poses, 700)
    assert [w["setCount"] for w in want][2:5] == [0, PS_SET_INVALID, PS_SET_INVALID] and want[0]["nkpts"] > 50
    k = int(np.nonzero(want[5]["rows"]["featIdx"] == f)[0][0])
    assert want[5]["rows"]["obsIdx"][k] == o
    lref.compare_sets(_build(ctx, store, p3d, poses, 700, fill=True).download(), want, SENTINEL, "ids")
    # THE RULE for a malformed obsStart: every set is invalid, nothing is written
    for at, val in ((0, -1), (300, int(store["obs_start"][299]) - 1), (700, len(store["obs_pose"]) + 1)):
        bad = dict(store)
        bad["obs_start"] = store["obs_start"].copy()
        bad["obs_start"][at] = val
        want = lref.pose_sets(bad, p3d, poses, 700)
        assert all(w["setCount"] == PS_SET_INVALID for w in want)
        lref.compare_sets(_build(ctx, bad, p3d, poses, 700, fill=True).download(), want, SENTINEL, ("obsStart", at))


def test_an_empty_store_and_no_sets(ctx):
    store = dict(pos=np.zeros((0, 3)), obs_start=np.zeros(1, np.int32), obs_pose=np.zeros(0, np.int32),
                 obs_desc=np.zeros((0, 32), np.uint8), obs_octave=np.zeros(0, np.int32), obs_det_dist=np.zeros(0), num_poses=5)
    p3d, poses = np.zeros((0, 3)), np.array([0, 4, 5], np.int32)
    want = lref.pose_sets(store, p3d, poses, 16)
    assert [w["setCount"] for w in want] == [0, 0, PS_SET_INVALID]
    lref.compare_sets(_build(ctx, store, p3d, poses, 16, fill=True).download(), want, SENTINEL, "empty store")
    got = _build(ctx, store, p3d, np.zeros(0, np.int32), 16, fill=True).download()        # S == 0: nkpts[0] = 0, PS_OK
    assert got["nkpts"].tolist() == [0] and (got["desc"] == SENTINEL[0]).all()


def test_twice_beside_a_busy_stream_gives_identical_bytes(ctx):
    import torch
    store, p3d, poses = _edge_scene()
    sd = lref.store_device(store)
    first = _build(ctx, store, p3d, poses, 600, sd=sd).download()
    side, x = torch.cuda.Stream(), torch.ones(1 << 24, device=sd.device)
    with torch.cuda.stream(side):
        for _ in range(100):
            x.mul_(1.0001)
    again = _build(ctx, store, p3d, poses, 600, sd=sd).download()
    side.synchronize()
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    lref.compare_sets(again, lref.pose_sets(store, p3d, poses, 600), what="busy")


# ---------------------------------------------------------------- the verifier
POSE0 = 8                 # poses 8 .. 22 of the scene are the directed ones: set index = pose id - POSE0
SIZES = {14: 35, 15: 36, 16: 9, 17: 10, 18: 11, 19: 40, 21: 5}


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(2026)
    store, p3d = lref.make_scene(rng, 1200, 8, max_obs=4, extra_poses=15)
    feats = lref.unpack(store, p3d)
    lref.plant_loop(rng, feats, 8, 9, range(0, 150))                 # a true loop
    lref.plant_loop(rng, feats, 10, 11, range(150, 450))             # a larger one (overflows a capacity of 256)
    lref.observe(rng, feats, 12, range(400, 460))                    # unrelated sets: run, rejected
    lref.observe(rng, feats, 13, range(500, 580))
    at = 600
    for q, n in SIZES.items():                                       # min, min + 1, 9, 10, 11; 40 (emptied below); 5
        lref.observe(rng, feats, q, range(at, at + n))
        at += n + 3
    store, p3d = lref.pack(store, feats)                             # (pose 20, 22: no observation)
    poses = np.arange(POSE0, 23, dtype=np.int32)
    pairs = np.array([[0, 1], [1, 0], [2, 3], [4, 5], [0, 4], [0, 5], [0, 2], [0, 0], [6, 0], [0, 6], [7, 0], [8, 0], [9, 0], [0, 9],
                      [10, 0], [11, 0], [0, 11], [12, 0], [13, 1], [4, 4], [5, 7], [-1, 0], [0, 15], [2 ** 31 - 1, -2 ** 31]], np.int32)
    return dict(store=store, p3d=p3d, poses=poses, pairs=pairs, S=len(poses))


def _emptied(sets):
    """Set 11 (40 members) with its keypoint count set to 0 behind the call: the one way to a RUN candidate without matches --
    cross-check matching of two non-empty sets always returns the closest pair --, the reference's -1.0 (matcher.cpp:838-839)."""
    sets = list(sets)
    sets[11] = dict(setCount=sets[11]["setCount"], nkpts=0, rows=None)
    return sets


def _empty_on_device(dev):
    import torch
    dev.nkpts[11] = 0
    torch.cuda.synchronize(dev.device)


def _run(ctx, sc, cap, pairs, prm, cfg, K, min_features, thr=0.4, side=True, feat=True, torch_stream=True, sd=None, sets=None):
    from putslam_amd.device_batch import LoopBatchDevice, run_loop_pairs
    if sets is None:
        sets = _build(ctx, sc["store"], sc["p3d"], sc["poses"], cap, side=side, sd=sd)
        _empty_on_device(sets)
    b = LoopBatchDevice(sets, pairs, min_features, thr, paired_feat=feat)
    for t in (b.ratio, b.closed, b.num_paired, b.paired_rows):
        t.fill_(-7)
    import torch
    torch.cuda.current_stream(b.device).synchronize()     # (the fills are done before the context's own stream writes)
    run_loop_pairs(ctx, prm, cfg, K, b, use_torch_stream=torch_stream)
    return b, sets


@pytest.mark.parametrize("min_features,mode,cap", [(35, EUCLIDEAN_ERROR, 320), (5, EUCLIDEAN_ERROR, 320), (35, REPROJECTION_ERROR, 320),
                                                   (5, EUCLIDEAN_ERROR, 256)])
def test_candidates_equal_the_restatement(ctx, oracle, scene, min_features, mode, cap):
    sc = scene
    prm = default_ransac_params(mode, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=806)
    sets = _emptied(lref.pose_sets(sc["store"], sc["p3d"], sc["poses"], cap))
    assert [s["setCount"] for s in sets[6:12]] == [35, 36, 9, 10, 11, 40] and sets[13]["setCount"] == 5
    want = lref.verify(oracle, sets, sc["pairs"], prm, cfg, TUM_FR1_K, min_features, 0.4, cap)
    st = dict(zip(map(tuple, sc["pairs"].tolist()), zip(want["state"], want["ratio"], want["closed"])))
    # what the batch contains, by the restatement's own answer
    assert st[(0, 1)][0] == lref.RUN and st[(0, 1)][2] == 1 and st[(1, 0)][2] == 1 and st[(0, 0)][2] == 1       # closed loops
    assert st[(4, 5)][0] == lref.RUN and st[(4, 5)][2] == 0 and st[(0, 4)][2] == 0                              # run, rejected
    assert st[(0, 11)][:2] == (lref.RUN, -1.0) and st[(11, 0)][:2] == (lref.RUN, -1.0)                          # no matches: -1.0
    assert st[(-1, 0)][0] == st[(0, 15)][0] == lref.INVALID_PAIR
    if min_features == 35:
        assert st[(6, 0)][0] == lref.GATED_MIN and st[(7, 0)][0] == lref.RUN                                    # 35: gated; 36: run
        assert st[(8, 0)][0] == st[(9, 0)][0] == st[(10, 0)][0] == lref.GATED_MIN
    else:
        assert st[(13, 1)][0] == lref.GATED_MIN                                                                 # 5 > 5 is false
        assert st[(8, 0)][0] == lref.GATED_10 and st[(9, 0)][0] == st[(0, 9)][0] == st[(10, 0)][0] == lref.RUN   # 9; 10, 11
    assert st[(12, 0)][0] == lref.GATED_MIN                                                                     # a pose nobody saw from
    assert st[(2, 3)][0] == (lref.INVALID_PAIR if cap == 256 else lref.RUN)                                     # 300 members each
    if cap != 256:
        assert st[(2, 3)][2] == 1 and want["numPaired"][2] > 200
    b, _ = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, min_features)
    lref.compare_verdicts(b.download(), want, what=(min_features, mode, cap))


def test_candidate_order_single_candidates_and_no_feature_indices(ctx, oracle, scene):
    from putslam_amd import api
    from putslam_amd.device_batch import LoopBatchDevice, run_loop_pairs
    sc, cap = scene, 320
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=41)
    sd = lref.store_device(sc["store"])
    b, sets = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 5, sd=sd)
    g = b.download()
    # another order: what does not depend on the draws follows its candidate; candidate l alone with seed + l is row l
    perm = np.random.default_rng(1).permutation(len(sc["pairs"]))
    gp = _run(ctx, sc, cap, sc["pairs"][perm], prm, cfg, TUM_FR1_K, 5, sets=sets)[0].download()
    for j, l in enumerate(perm):
        n = max(int(g["numMatches"][l]), 0)
        assert gp["numMatches"][j] == g["numMatches"][l] and gp["matches"][j, :n].tobytes() == g["matches"][l, :n].tobytes()
        assert (gp["numPaired"][j] == PS_SET_INVALID) == (g["numPaired"][l] == PS_SET_INVALID)
        assert (gp["ratio"][j] == 0.0) == (g["ratio"][l] == 0.0) and (gp["ratio"][j] == -1.0) == (g["ratio"][l] == -1.0)
    keys = ("numMatches", "pose", "stats", "ratio", "closed", "numPaired")
    for l in (0, 3, 7, 12, 16, 21):
        cfg_l, _ = make_config(EST_RANSAC, H_LC, seed=41 + l)
        one = _run(ctx, sc, cap, sc["pairs"][l:l + 1], prm, cfg_l, TUM_FR1_K, 5, sets=sets)[0].download()
        n = max(int(g["numPaired"][l]), 0)
        assert all(one[k][0].tobytes() == g[k][l].tobytes() for k in keys), l
        assert one["pairedRows"][0, :n].tobytes() == g["pairedRows"][l, :n].tobytes()
        assert one["pairedFeat"][0, :n].tobytes() == g["pairedFeat"][l, :n].tobytes()
    # without featIdx / pairedFeat: the same rows; pairedFeat without featIdx is refused
    sets = _emptied(lref.pose_sets(sc["store"], sc["p3d"], sc["poses"], cap))
    want = lref.verify(oracle, sets, sc["pairs"], prm, cfg, TUM_FR1_K, 5, 0.4, cap)
    lref.compare_verdicts(g, want, what="with featIdx")
    b2, bare = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 5, side=False, feat=False, sd=sd)
    lref.compare_verdicts(b2.download(), want, with_feat=False, what="without featIdx")
    with pytest.raises(api.PsError) as e:
        run_loop_pairs(ctx, prm, cfg, TUM_FR1_K, LoopBatchDevice(bare, sc["pairs"], 5, 0.4, paired_feat=True))
    assert e.value.code == -1
    # L == 0: PS_OK, nothing written; a threshold nothing passes / everything run passes
    b0 = _run(ctx, sc, cap, np.zeros((0, 2), np.int32), prm, cfg, TUM_FR1_K, 5, sets=bare, feat=False)[0]
    assert b0.download()["ratio"].shape == (0,) and (b0.ratio.cpu().numpy() == -7).all()
    hi = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 5, thr=1.0, sets=bare, feat=False)[0].download()
    lo = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 5, thr=-2.0, sets=bare, feat=False)[0].download()
    valid = g["numPaired"] != PS_SET_INVALID                          # (a candidate that names an invalid set is never closed)
    assert not hi["closed"].any() and lo["closed"][valid].all() and not lo["closed"][~valid].any() and not valid.all()
    assert hi["ratio"].tobytes() == lo["ratio"].tobytes() == g["ratio"].tobytes()


# ---------------------------------------------------------------- chain and hand-over
def test_verify_loop_closures_end_to_end_with_one_retry(ctx, oracle, scene):
    sc = scene
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=5)
    cand = np.array([[8, 9], [10, 11], [11, 10], [12, 13], [8, 12], [14, 8], [15, 8], [20, 8], [9, 9], [16, 17], [8, 13]], np.int32)
    sd = lref.store_device(sc["store"])
    for first_cap, final_cap in ((64, 300), (400, 400)):             # the largest set has 300 members: one retry / none
        r = ctx.verify_loop_closures(sd, sc["p3d"], cand, prm, cfg, TUM_FR1_K, max_kpts=first_cap)
        assert r["max_kpts"] == final_cap
        poses = np.unique(cand)
        assert (r["poses"] == poses).all() and (poses[r["pairs"]] == cand).all()
        sets = lref.pose_sets(sc["store"], sc["p3d"], poses, final_cap)
        want = lref.verify(oracle, sets, r["pairs"], prm, cfg, TUM_FR1_K, 35, 0.4, final_cap)
        assert want["closed"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0] and want["state"][5] == lref.GATED_MIN
        assert r["set_count"].tolist() == [s["setCount"] for s in sets]
        assert r["ratio"].tobytes() == want["ratio"].tobytes() and r["closed"].tolist() == [bool(c) for c in want["closed"]]
        assert r["num_paired"].tolist() == want["numPaired"].tolist()
        assert r["num_matches"].tobytes() == want["pair"]["numMatches"].tobytes()
        assert r["pose"].transpose(0, 2, 1).reshape(-1, 16).tobytes() == want["pair"]["pose"].tobytes()
        for l in range(len(cand)):
            assert r["paired_rows"][l].tobytes() == want["paired_rows"][l].tobytes()
            assert r["paired_feat"][l].tobytes() == want["paired_feat"][l].tobytes()


def test_the_same_results_on_the_contexts_stream_and_on_a_torch_stream(ctx, scene):
    import torch
    from putslam_amd.device_batch import build_pose_sets
    sc, cap = scene, 320
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=77)
    sd = lref.store_device(sc["store"])
    p3d = torch.from_numpy(sc["p3d"]).to(sd.device)
    results, side = [], torch.cuda.Stream()
    for mode in ("own", "torch", "own", "default"):
        if mode == "own":
            ctx.set_stream(0)
            sets = build_pose_sets(ctx, sd, p3d, sc["poses"], cap, use_torch_stream=False)
            b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 35, torch_stream=False, sets=sets)[0]
        elif mode == "torch":
            with torch.cuda.stream(side):
                sets = build_pose_sets(ctx, sd, p3d, sc["poses"], cap)
                b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 35, sets=sets)[0]
        else:
            sets = build_pose_sets(ctx, sd, p3d, sc["poses"], cap)
            b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, TUM_FR1_K, 35, sets=sets)[0]
        g, gs = b.download(), sets.download()
        results.append({**{k: v.tobytes() for k, v in g.items() if k not in ("matches", "inlierMask", "pairedRows", "pairedFeat")},
                        **{"set:" + k: v.tobytes() for k, v in gs.items()},
                        "rows": [g["pairedRows"][l, :max(int(n), 0)].tobytes() for l, n in enumerate(g["numPaired"])]})
    assert results[0]["ratio"] != np.zeros(len(sc["pairs"])).tobytes()
    assert all(r == results[0] for r in results[1:])
