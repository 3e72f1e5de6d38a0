"""Loop-closure candidates verified from a resident store of FLOAT descriptor rows (ps_pose_sets_l2_device,
ps_loop_pairs_l2_device, Context.verify_loop_closures_l2) against tests/map_store_f32_ref.py -- the sequential walks of
tests/loop_closure_ref.py, l2_match_ref.match_l2 and the CPU oracle's RANSAC --, byte for byte: the cases of
tests/test_gpu_loop_closure.py that concern rows and verdicts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_ref as lref  # noqa: E402
import map_store_f32_ref as fref  # noqa: E402

from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, PS_SET_INVALID, REPROJECTION_ERROR, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

H = 487
H_LC = 1157          # the loop-closure config's cap on the hypotheses


def _build(ctx, fs, p3d, poses, cap, row_floats=None, offset=0, side=True, fill=True, sd=None):
    from putslam_amd.device_batch import PoseSetsF32Device, build_pose_sets_l2
    sd = fref.store_device(fs) if sd is None else sd
    out = PoseSetsF32Device(len(poses), cap, sd.dim, sd.device, row_floats, offset, side)
    if fill:
        fref.fill_sentinels(out)
        out.set_count.fill_(77)
        out.nkpts.fill_(77)
    return build_pose_sets_l2(ctx, sd, p3d, poses, cap, out=out, side_arrays=side)


def _check(out, want, what):
    fref.compare_sets(out.download(), want, fref.SENTINEL, what)
    fref.check_untouched(out, want, what)


def _float(rng, store, dim, special=True):
    make = fref.special_rows if special else fref.unit_rows
    return fref.float_store(store, make(rng, len(store["obs_pose"]), dim))


# ---------------------------------------------------------------- pose sets
@pytest.mark.parametrize("F,N,max_obs,dim,row_floats,offset", [(2000, 40, 12, 64, None, 0), (1500, 30, 8, 128, 132, 0),
                                                               (257, 5, 5, 3, 4, 1), (90, 3, 3, 512, None, 0)])
def test_random_stores_equal_the_restatement(ctx, F, N, max_obs, dim, row_floats, offset):
    rng = np.random.default_rng(F * 31 + N)
    store, p3d = lref.make_scene(rng, F, N, max_obs=max_obs)
    fs = _float(rng, store, dim)
    poses = rng.permutation(N).astype(np.int32)
    cap = min(F, 600)
    want = fref.pose_sets(fs, p3d, poses, cap)
    counts = [w["setCount"] for w in want]
    assert max(counts) > F // 8 and len(set(counts)) > 1, counts
    _check(_build(ctx, fs, p3d, poses, cap, row_floats, offset), want, (F, N))


def _edge_scene(dim):
    """Member counts of 0, 1, 255, 256, 257 and 513 on poses nobody else observed from (tests/test_gpu_loop_closure.py's)."""
    rng = np.random.default_rng(513)
    store, p3d = lref.make_scene(rng, 1100, 4, max_obs=3, extra_poses=8)
    feats = lref.unpack(store, p3d)
    lref.observe(rng, feats, 5, [1099])
    lref.observe(rng, feats, 6, range(0, 255))
    lref.observe(rng, feats, 7, range(256, 512))
    lref.observe(rng, feats, 8, range(255, 512))
    lref.observe(rng, feats, 9, range(300, 813))
    store, p3d = lref.pack(store, feats)
    return _float(rng, store, dim), p3d, np.array([4, 5, 6, 7, 8, 9, 1, 7], np.int32)


@pytest.mark.parametrize("dim", [64, 7])
def test_chunk_and_wave_edges_overflow_and_untouched_rows(ctx, dim):
    fs, p3d, poses = _edge_scene(dim)
    want = fref.pose_sets(fs, p3d, poses, 600)
    assert [w["setCount"] for w in want][:6] == [0, 1, 255, 256, 257, 513]
    assert (want[3]["rows"]["featIdx"] == np.arange(256, 512)).all()                     # a chunk owned by one set; pose 7 twice
    assert fref.same_words(want[3]["rows"]["desc"], want[7]["rows"]["desc"])
    sd = fref.store_device(fs)
    _check(_build(ctx, fs, p3d, poses, 600, sd=sd), want, "edges")
    # capacity 256: the sets of 257 and 513 report -(count), their rows and everybody else's rows beyond the count stay untouched
    want = fref.pose_sets(fs, p3d, poses, 256)
    assert [w["setCount"] for w in want][:6] == [0, 1, 255, 256, -257, -513]
    _check(_build(ctx, fs, p3d, poses, 256, sd=sd), want, "overflow")
    _check(_build(ctx, fs, p3d, poses, 256, side=False, sd=sd), want, "no side arrays")


def test_one_chunk_touching_a_hundred_sets_and_the_set_limits(ctx):
    from putslam_amd import api
    from putslam_amd.device_batch import PoseSetsF32Device, build_pose_sets_l2
    rng = np.random.default_rng(64)
    store, p3d = lref.make_scene(rng, 600, 100, max_obs=12)
    fs = _float(rng, store, 20)
    poses = np.arange(100, dtype=np.int32)
    want = fref.pose_sets(fs, p3d, poses, 600)
    assert sum(w["nkpts"] > 0 and (w["rows"]["featIdx"] < 256).any() for w in want) > 64
    sd = fref.store_device(fs)
    _check(_build(ctx, fs, p3d, poses, 600, sd=sd), want, "100 sets")
    _check(_build(ctx, fs, p3d, poses[17:18], 600, sd=sd), want[17:18], "S = 1")
    many = (np.arange(1024) % 100).astype(np.int32)                                      # every pose listed ten times: chains
    _check(_build(ctx, fs, p3d, many, 200, sd=sd), fref.pose_sets(fs, p3d, many, 200), "S = 1024")
    with pytest.raises(api.PsError) as e:
        _build(ctx, fs, p3d, np.zeros(1025, np.int32), 8, sd=sd)
    assert e.value.code == -5

    def refused(code, mutate_store=None, **attrs):
        out = fref.fill_sentinels(PoseSetsF32Device(1, 8, 20, sd.device))
        for k, v in attrs.items():
            setattr(out, k, v)
        st = sd
        if mutate_store is not None:
            class Mutated:
                device, dim, num_obs = sd.device, sd.dim, sd.num_obs

                def view(self):
                    v = sd.view()
                    mutate_store(v)
                    return v
            st = Mutated()
        with pytest.raises(api.PsError) as e:
            build_pose_sets_l2(ctx, st, p3d, poses[:1], out.max_kpts, out=out)
        assert e.value.code == code, (e.value, attrs)
        out.max_kpts, out.num_frames, out.dim, out.row_floats = 8, 2, 20, 20
        fref.check_untouched(out, [dict(nkpts=0)], attrs)

    refused(-5, max_kpts=16385)
    refused(-1, max_kpts=0)
    refused(-1, num_frames=1)                                                            # numFrames < S + 1
    refused(-1, dim=21, row_floats=21)                                                   # sets.dim != store.dim
    refused(-1, lambda v: setattr(v, "dim", 0))
    refused(-5, lambda v: setattr(v, "dim", 513))
    refused(-1, lambda v: setattr(v, "obsDescRowStride", 76))                            # below a row of 20 floats
    refused(-1, lambda v: setattr(v, "obsDescRowStride", 82))
    refused(-1, lambda v: setattr(v, "obsDesc", v.obsDesc + 1))


def test_bad_pose_ids_foreign_observations_and_a_malformed_index(ctx):
    rng = np.random.default_rng(99)
    store, p3d = lref.make_scene(rng, 700, 12, max_obs=6, extra_poses=1)                 # pose 12: never observed from
    store["obs_pose"][rng.choice(len(store["obs_pose"]), 40, replace=False)] = np.tile([13, -2, 2 ** 30, -2 ** 31], 10)
    f = int(np.nonzero(np.diff(store["obs_start"]) >= 3)[0][5])
    o = int(store["obs_start"][f])
    store["obs_pose"][o:o + 3] = [4, 4, 4]                                               # malformed: the first observation is taken
    fs = _float(rng, store, 64)
    poses = np.array([3, 3, 12, -1, 13, 4, -2 ** 31, 2 ** 31 - 1, 0], np.int32)          # listed twice, unobserved, outside the table
    want = fref.pose_sets(fs, p3d, poses, 700)
    assert [w["setCount"] for w in want][2:5] == [0, PS_SET_INVALID, PS_SET_INVALID] and want[0]["nkpts"] > 50
    k = int(np.nonzero(want[5]["rows"]["featIdx"] == f)[0][0])
    assert want[5]["rows"]["obsIdx"][k] == o and fref.same_words(want[5]["rows"]["desc"][k], fs["rows"][o])
    _check(_build(ctx, fs, p3d, poses, 700), want, "ids")
    # THE RULE for a malformed obsStart: every set is invalid, nothing is written
    for at, val in ((0, -1), (300, int(store["obs_start"][299]) - 1), (700, len(store["obs_pose"]) + 1)):
        bad = dict(fs)
        bad["obs_start"] = fs["obs_start"].copy()
        bad["obs_start"][at] = val
        want = fref.pose_sets(bad, p3d, poses, 700)
        assert all(w["setCount"] == PS_SET_INVALID for w in want)
        _check(_build(ctx, bad, p3d, poses, 700, side=at != 300), want, ("obsStart", at))


def test_an_empty_store_and_no_sets(ctx):
    store = dict(pos=np.zeros((0, 3)), obs_start=np.zeros(1, np.int32), obs_pose=np.zeros(0, np.int32),
                 obs_desc=np.zeros((0, 32), np.uint8), obs_octave=np.zeros(0, np.int32), obs_det_dist=np.zeros(0), num_poses=5)
    fs = fref.float_store(store, np.zeros((0, 64), np.float32))
    p3d, poses = np.zeros((0, 3)), np.array([0, 4, 5], np.int32)
    want = fref.pose_sets(fs, p3d, poses, 16)
    assert [w["setCount"] for w in want] == [0, 0, PS_SET_INVALID]
    _check(_build(ctx, fs, p3d, poses, 16), want, "empty store")
    out = _build(ctx, fs, p3d, np.zeros(0, np.int32), 16)                                # S == 0: nkpts[0] = 0, PS_OK
    assert out.download()["nkpts"].tolist() == [0]
    fref.check_untouched(out, [], "S == 0")


# ---------------------------------------------------------------- the verifier
def _scene(dim, cache={}):
    if dim not in cache:
        cache[dim] = fref.loop_scene(dim)      # (built once per width, never changed)
    return cache[dim]


def _empty_on_device(dev):
    import torch
    dev.nkpts[fref.EMPTIED] = 0
    torch.cuda.synchronize(dev.device)


def _run(ctx, sc, cap, pairs, prm, cfg, min_features, thr=0.4, side=True, feat=True, torch_stream=True, sd=None, sets=None):
    import torch
    from putslam_amd.device_batch import LoopBatchF32Device, run_loop_pairs_l2
    if sets is None:
        sets = _build(ctx, sc["store"], sc["p3d"], sc["poses"], cap, side=side, fill=False, sd=sd)
        _empty_on_device(sets)
    b = LoopBatchF32Device(sets, pairs, min_features, thr, paired_feat=feat)
    for t in (b.ratio, b.closed, b.num_paired, b.paired_rows):
        t.fill_(-7)
    torch.cuda.current_stream(b.device).synchronize()     # (the fills are done before the context's own stream writes)
    run_loop_pairs_l2(ctx, prm, cfg, TUM_FR1_K, b, use_torch_stream=torch_stream)
    return b, sets


def _want(oracle, sc, cap, prm, H_, seed, min_features, pairs=None, cache={}):
    key = (sc["dim"], cap, prm.errorVersion, H_, seed, min_features, None if pairs is None else pairs.tobytes())
    if key not in cache:
        sets = fref.emptied(fref.pose_sets(sc["store"], sc["p3d"], sc["poses"], cap))
        cache[key] = fref.verify(oracle, sets, sc["pairs"] if pairs is None else pairs, prm, EST_RANSAC, H_, seed, TUM_FR1_K,
                                 min_features, 0.4, cap, sc["dim"])
    return cache[key]


CASES = [(dim, mf, EUCLIDEAN_ERROR, cap, H) for dim in (64, 128, 7) for mf, cap in ((35, 320), (5, 320), (5, 256))]
CASES += [(64, 35, EUCLIDEAN_ERROR, 320, H_LC), (64, 35, REPROJECTION_ERROR, 320, H_LC)]      # E0 and E1 at H = 1157


@pytest.mark.parametrize("dim,min_features,mode,cap,H_", CASES)
def test_candidates_equal_the_restatement_in_both_matcher_forms(ctx, oracle, dim, min_features, mode, cap, H_):
    sc = _scene(dim)
    prm = default_ransac_params(mode, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_, seed=806)
    want = _want(oracle, sc, cap, prm, H_, 806, min_features)
    states = set(want["state"])
    assert lref.RUN in states and lref.GATED_MIN in states and lref.INVALID_PAIR in states and want["closed"].sum() >= 3
    assert (want["ratio"] == -1.0).sum() == 2                                            # (tests/test_map_store_f32_host.py: the rest)
    got = []
    for form in (1, 0):
        ctx.set_option("matcher_l2", form)
        try:
            b, _ = _run(ctx, sc, cap, sc["pairs"], prm, cfg, min_features)
            g = b.download()
        finally:
            ctx.set_option("matcher_l2", 1)
        assert ctx.get_option("matcher_l2_used") == (form if sc["dim"] in (64, 128) else 0)
        fref.compare_verdicts(g, want, what=(sc["dim"], min_features, mode, cap, form))
        n = np.maximum(g["numMatches"], 0)
        got.append({**{k: g[k].tobytes() for k in ("numMatches", "pose", "stats", "ratio", "closed", "numPaired")},
                    "rows": [g["matches"][l, :n[l]].tobytes() + g["inlierMask"][l, :n[l]].tobytes() for l in range(len(n))]})
    assert got[0] == got[1]


@pytest.mark.parametrize("dim", [64, 7])
def test_candidate_order_single_candidates_and_no_feature_indices(ctx, oracle, dim):
    from putslam_amd import api
    from putslam_amd.device_batch import LoopBatchF32Device, run_loop_pairs_l2
    sc, cap = _scene(dim), 320
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H, seed=41)
    sd = fref.store_device(sc["store"])
    b, sets = _run(ctx, sc, cap, sc["pairs"], prm, cfg, 5, sd=sd)
    g = b.download()
    want = _want(oracle, sc, cap, prm, H, 41, 5)
    fref.compare_verdicts(g, want, what="with featIdx")
    # another order: what does not depend on the draws follows its candidate; candidate l alone with seed + l is row l
    perm = np.random.default_rng(1).permutation(len(sc["pairs"]))
    gp = _run(ctx, sc, cap, sc["pairs"][perm], prm, cfg, 5, sets=sets)[0].download()
    for j, l in enumerate(perm):
        n = max(int(g["numMatches"][l]), 0)
        assert gp["numMatches"][j] == g["numMatches"][l] and gp["matches"][j, :n].tobytes() == g["matches"][l, :n].tobytes()
        assert (gp["numPaired"][j] == PS_SET_INVALID) == (g["numPaired"][l] == PS_SET_INVALID)
        assert (gp["ratio"][j] == 0.0) == (g["ratio"][l] == 0.0) and (gp["ratio"][j] == -1.0) == (g["ratio"][l] == -1.0)
    keys = ("numMatches", "pose", "stats", "ratio", "closed", "numPaired")
    for l in (0, 3, 7, 12, 16, 21):
        cfg_l, _ = make_config(EST_RANSAC, H, seed=41 + l)
        one = _run(ctx, sc, cap, sc["pairs"][l:l + 1], prm, cfg_l, 5, sets=sets)[0].download()
        n = max(int(g["numPaired"][l]), 0)
        assert all(one[k][0].tobytes() == g[k][l].tobytes() for k in keys), l
        assert one["pairedRows"][0, :n].tobytes() == g["pairedRows"][l, :n].tobytes()
        assert one["pairedFeat"][0, :n].tobytes() == g["pairedFeat"][l, :n].tobytes()
    # without featIdx / pairedFeat: the same rows; pairedFeat without featIdx is refused
    b2, bare = _run(ctx, sc, cap, sc["pairs"], prm, cfg, 5, side=False, feat=False, sd=sd)
    fref.compare_verdicts(b2.download(), want, with_feat=False, what="without featIdx")
    with pytest.raises(api.PsError) as e:
        run_loop_pairs_l2(ctx, prm, cfg, TUM_FR1_K, LoopBatchF32Device(bare, sc["pairs"], 5, 0.4, paired_feat=True))
    assert e.value.code == -1
    # L == 0: PS_OK, nothing written
    b0 = _run(ctx, sc, cap, np.zeros((0, 2), np.int32), prm, cfg, 5, sets=bare, feat=False)[0]
    assert b0.download()["ratio"].shape == (0,) and (b0.ratio.cpu().numpy() == -7).all()


@pytest.mark.parametrize("dim", [64, 7])
def test_verify_loop_closures_l2_end_to_end_with_one_retry(ctx, oracle, dim):
    sc = _scene(dim)
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H, seed=5)
    cand = np.array([[8, 9], [10, 11], [11, 10], [12, 13], [8, 12], [14, 8], [15, 8], [20, 8], [9, 9], [16, 17], [8, 13]], np.int32)
    sd = fref.store_device(sc["store"])
    for first_cap, final_cap in ((64, 300), (400, 400)):             # the largest set has 300 members: one retry / none
        r = ctx.verify_loop_closures_l2(sd, sc["p3d"], cand, prm, cfg, TUM_FR1_K, max_kpts=first_cap)
        assert r["max_kpts"] == final_cap
        poses = np.unique(cand)
        assert (r["poses"] == poses).all() and (poses[r["pairs"]] == cand).all()
        sets = fref.pose_sets(sc["store"], sc["p3d"], poses, final_cap)
        want = fref.verify(oracle, sets, r["pairs"], prm, EST_RANSAC, H, 5, TUM_FR1_K, 35, 0.4, final_cap, sc["dim"])
        assert want["closed"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0] and want["state"][5] == lref.GATED_MIN
        assert r["set_count"].tolist() == [s["setCount"] for s in sets]
        assert r["ratio"].tobytes() == want["ratio"].tobytes() and r["closed"].tolist() == [bool(c) for c in want["closed"]]
        assert r["num_paired"].tolist() == want["numPaired"].tolist()
        assert r["num_matches"].tobytes() == want["pair"]["numMatches"].tobytes()
        assert r["pose"].transpose(0, 2, 1).reshape(-1, 16).tobytes() == want["pair"]["pose"].tobytes()
        for l in range(len(cand)):
            assert r["paired_rows"][l].tobytes() == want["paired_rows"][l].tobytes()
            assert r["paired_feat"][l].tobytes() == want["paired_feat"][l].tobytes()


def test_the_same_results_on_the_contexts_stream_and_on_a_torch_stream(ctx):
    import torch
    from putslam_amd.device_batch import build_pose_sets_l2
    sc, cap = _scene(64), 320
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H, seed=77)
    sd = fref.store_device(sc["store"])
    p3d = torch.from_numpy(sc["p3d"]).to(sd.device)
    results, side = [], torch.cuda.Stream()
    for mode in ("own", "torch", "own", "default"):
        if mode == "own":
            ctx.set_stream(0)
            sets = build_pose_sets_l2(ctx, sd, p3d, sc["poses"], cap, use_torch_stream=False)
            b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, 35, torch_stream=False, sets=sets)[0]
        elif mode == "torch":
            with torch.cuda.stream(side):
                sets = build_pose_sets_l2(ctx, sd, p3d, sc["poses"], cap)
                b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, 35, sets=sets)[0]
        else:
            sets = build_pose_sets_l2(ctx, sd, p3d, sc["poses"], cap)
            b = _run(ctx, sc, cap, sc["pairs"], prm, cfg, 35, sets=sets)[0]
        g, gs = b.download(), sets.download()
        results.append({**{k: v.tobytes() for k, v in g.items() if k not in ("matches", "inlierMask", "pairedRows", "pairedFeat")},
                        **{"set:" + k: v.view(np.uint32).tobytes() if v.dtype == np.float32 else v.tobytes() for k, v in gs.items()},
                        "rows": [g["pairedRows"][l, :max(int(n), 0)].tobytes() for l, n in enumerate(g["numPaired"])]})
    assert results[0]["ratio"] != np.zeros(len(sc["pairs"])).tobytes()
    assert all(r == results[0] for r in results[1:])
