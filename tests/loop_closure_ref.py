"""CPU answer and scenes for the batched loop-closure verification (ps_pose_sets_device / ps_loop_pairs_device).

`pose_sets` and `verify` are a sequential restatement of the reference's loop-closure thread, in its loop order:
FeaturesMap::loopClosure (src/Map/featuresMap.cpp:733-873) -- camTrajectory[q].featuresIds as a std::set<int> walked in
ascending order, the gate on minNumberOfFeaturesLC (:776-779), the threshold on the returned ratio (:806) -- around
Matcher::matchFeatureLoopClosure (src/Matcher/matcher.cpp:802-861): each feature's descriptor and (float) point3D as observed
from that pose (:816-824), the 10-feature gate (:830), performMatching, the -1.0 for "no matches" (:838-839), RANSAC, the repack
of the inlier matches (:853-857) and pointInlierRatio (:859).  The inner call is the CPU oracle's (oracle_py.vo_pairs: matcher +
RANSAC with seed + l for candidate l).  Like every restatement of this project it is RESTATED, not compiled against the reference.

`pose_sets_fast` is a second, brute-force formulation of the sets (a mask over all observations per pose) that
tests/test_loop_closure_host.py holds against the walk.
"""
import numpy as np

import map_view_ref as vref

from putslam_amd._abi import PS_SET_INVALID


# ---------------------------------------------------------------- the sets
def _range_ok(store):
    start, O = store["obs_start"].astype(np.int64), len(store["obs_pose"])
    return bool((start[:-1] >= 0).all() and (start[1:] >= start[:-1]).all() and (start[1:] <= O).all())


def _answer(store, p3d, feat, obs, max_kpts):
    n = len(feat)
    if n > max_kpts:
        return dict(setCount=-n, nkpts=0, rows=None)
    obs = np.asarray(obs, np.int64).reshape(n)
    rows = dict(featIdx=np.asarray(feat, np.int32).reshape(n), obsIdx=obs.astype(np.int32),
                desc=store["obs_desc"][obs].reshape(n, 32), pts=p3d[obs].reshape(n, 3).astype(np.float32))
    return dict(setCount=n, nkpts=n, rows=rows)


INVALID = dict(setCount=PS_SET_INVALID, nkpts=0, rows=None)


def pose_sets(store, p3d, poses, max_kpts):
    """One answer per entry of `poses`: dict(setCount, nkpts, rows or None).  The walk the reference's bookkeeping amounts to:
    every feature's observation map (ascending pose id) is visited once, feature f joins featuresIds of each pose it was
    observed from (the first observation with that pose id, should a malformed store hold two); a pose's set is then read in
    std::set order.  A malformed observation range anywhere in the store invalidates every set."""
    start, pose_of, N = store["obs_start"], store["obs_pose"], store["num_poses"]
    if not _range_ok(store):
        return [dict(INVALID) for _ in poses]
    ids = {}                                            # pose -> {feature: observation}
    for f in range(len(store["pos"])):
        for o in range(int(start[f]), int(start[f + 1])):
            q = int(pose_of[o])
            if 0 <= q < N:
                ids.setdefault(q, {}).setdefault(f, o)
    out = []
    for q in poses:
        q = int(q)
        if q < 0 or q >= N:
            out.append(dict(INVALID))
            continue
        members = ids.get(q, {})
        feat = sorted(members)                          # std::set<int>
        out.append(_answer(store, p3d, feat, [members[f] for f in feat], max_kpts))
    return out


def pose_sets_fast(store, p3d, poses, max_kpts):
    """The same answer, formulated differently: per pose a mask over ALL observations, the first hit of every feature."""
    if not _range_ok(store):
        return [dict(INVALID) for _ in poses]
    start, pose_of, N = store["obs_start"].astype(np.int64), store["obs_pose"], store["num_poses"]
    feat_of = np.repeat(np.arange(len(store["pos"])), np.diff(start))
    covered = np.zeros(len(pose_of), bool)
    covered[start[0]:start[-1]] = True                 # (observations outside every feature's range belong to nobody)
    out = []
    for q in poses:
        q = int(q)
        if q < 0 or q >= N:
            out.append(dict(INVALID))
            continue
        hit = np.nonzero((pose_of == q) & covered)[0]
        feat, first = np.unique(feat_of[hit - start[0]], return_index=True) if len(hit) else (np.zeros(0, int), np.zeros(0, int))
        out.append(_answer(store, p3d, feat, hit[first], max_kpts))
    return out


def sets_equal(a, b):
    if a["setCount"] != b["setCount"] or a["nkpts"] != b["nkpts"] or (a["rows"] is None) != (b["rows"] is None):
        return False
    return a["rows"] is None or all(a["rows"][k].tobytes() == b["rows"][k].tobytes() for k in a["rows"])


def compare_sets(got, want, sentinel=None, what=""):
    """got: PoseSetsDevice.download(); want: pose_sets' list.  Bytes, rows up to the count; the empty set behind them.
    sentinel = (byte, float): rows beyond every count (and every row of an overflowed or invalid set) still hold it."""
    S = len(want)
    assert len(got["setCount"]) == S and int(got["nkpts"][S]) == 0, what
    for s, w in enumerate(want):
        tag = (what, s)
        assert int(got["setCount"][s]) == w["setCount"], (tag, int(got["setCount"][s]), w["setCount"])
        assert int(got["nkpts"][s]) == w["nkpts"], tag
        n = w["nkpts"]
        for k in ("desc", "pts", "featIdx", "obsIdx"):
            if k in got and n:
                assert got[k][s, :n].tobytes() == w["rows"][k].tobytes(), (tag, k)
        if sentinel is not None:
            assert (got["desc"][s, n:] == sentinel[0]).all() and (got["pts"][s, n:] == sentinel[1]).all(), tag
            if "featIdx" in got:
                assert (got["featIdx"][s, n:] == sentinel[0]).all() and (got["obsIdx"][s, n:] == sentinel[0]).all(), tag
    if sentinel is not None:
        assert (got["desc"][S] == sentinel[0]).all() and (got["pts"][S] == sentinel[1]).all(), (what, "empty set")


def sets_as_frames(sets, max_kpts):
    """pose_sets' answers as the frame set the verifier reads: S + 1 frames, the last one empty."""
    S = len(sets)
    desc, pts = np.zeros((S + 1, max_kpts, 32), np.uint8), np.zeros((S + 1, max_kpts, 3), np.float32)
    nk, feat = np.zeros(S + 1, np.int32), np.zeros((S + 1, max_kpts), np.int32)
    for s, w in enumerate(sets):
        n = w["nkpts"]
        nk[s] = n
        if n:
            desc[s, :n], pts[s, :n], feat[s, :n] = w["rows"]["desc"], w["rows"]["pts"], w["rows"]["featIdx"]
    return desc, pts, nk, feat


# ---------------------------------------------------------------- the loop
RUN, GATED_MIN, GATED_10, INVALID_PAIR = "run", "gated: minNumberOfFeaturesLC", "gated: fewer than 10", "invalid"


def gate(sets, a, b, min_features):
    S = len(sets)
    if not (0 <= a < S and 0 <= b < S) or sets[a]["setCount"] < 0 or sets[b]["setCount"] < 0:
        return INVALID_PAIR
    na, nb = sets[a]["setCount"], sets[b]["setCount"]
    if not (na > min_features and nb > min_features):       # featuresMap.cpp:776-779
        return GATED_MIN
    if na < 10 or nb < 10:                                   # matcher.cpp:830
        return GATED_10
    return RUN


def verify(oracle, sets, pairs, params, cfg, K, min_features, threshold, max_kpts):
    """The loop over the candidates.  Returns dict(state [L], ratio, closed, numPaired, paired_rows / paired_feat (lists of
    (n, 2) int32), pair = oracle.vo_pairs' block for the effective pairs)."""
    S, L = len(sets), len(pairs)
    desc, pts, nk, feat = sets_as_frames(sets, max_kpts)
    state = [gate(sets, int(a), int(b), min_features) for a, b in pairs]
    eff = np.array([(a, b) if st == RUN else (S, S) for (a, b), st in zip(pairs, state)], np.int32).reshape(L, 2)
    vo = oracle.vo_pairs(params, cfg, K, desc, pts, nk, eff, threads=4)          # candidate l draws from seed + l
    ratio, closed, num, rows, feats = np.zeros(L), np.zeros(L, np.int32), np.zeros(L, np.int32), [], []
    for l in range(L):
        r, pr = 0.0, np.zeros((0, 2), np.int32)              # matchingRatio = 0.0 (featuresMap.cpp:764)
        if state[l] == RUN:
            n = int(vo["numMatches"][l])
            if n <= 0:
                r = -1.0                                     # matcher.cpp:838-839
            else:
                m = vo["matches"][l, :n][vo["inlierMask"][l, :n] != 0]          # inlierMatches, in match order
                pr = np.stack([m["queryIdx"], m["trainIdx"]], axis=1).astype(np.int32).reshape(-1, 2)     # :853-857
                r = float(vo["stats"][l]["pointInlierRatio"])                   # :859
        ratio[l], closed[l] = r, 1 if r > threshold and state[l] != INVALID_PAIR else 0   # featuresMap.cpp:806
        num[l] = PS_SET_INVALID if state[l] == INVALID_PAIR else len(pr)
        rows.append(pr)
        a, b = (int(x) for x in eff[l])
        feats.append(np.stack([feat[a][pr[:, 0]], feat[b][pr[:, 1]]], axis=1).astype(np.int32).reshape(-1, 2))
    return dict(state=state, ratio=ratio, closed=closed, numPaired=num, paired_rows=rows, paired_feat=feats, pair=vo, eff=eff)


STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers", "accepted",
               "bestInlierRatio", "pointInlierRatio")


def _same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def compare_verdicts(got, want, with_feat=True, what=""):
    """got: LoopBatchDevice.download(); want: verify's dict.  Byte for byte (NaN stats fields compare as NaN)."""
    L = len(want["state"])
    assert _same_bytes(got["numMatches"], want["pair"]["numMatches"]), what
    assert _same_bytes(got["pose"], want["pair"]["pose"]), what
    for l in range(L):
        tag = (what, l, want["state"][l])
        n = max(int(want["pair"]["numMatches"][l]), 0)
        assert _same_bytes(got["matches"][l, :n], want["pair"]["matches"][l, :n]), tag
        assert _same_bytes(got["inlierMask"][l, :n], want["pair"]["inlierMask"][l, :n]), tag
        for f in STAT_FIELDS:
            x, y = got["stats"][l][f], want["pair"]["stats"][l][f]
            assert _same_bytes(x, y) or (np.isnan(x) and np.isnan(y)), (tag, f, x, y)
        assert _same_bytes(np.float64(got["ratio"][l]), np.float64(want["ratio"][l])), (tag, got["ratio"][l], want["ratio"][l])
        assert int(got["closed"][l]) == int(want["closed"][l]), tag
        assert int(got["numPaired"][l]) == int(want["numPaired"][l]), (tag, int(got["numPaired"][l]))
        k = len(want["paired_rows"][l])
        assert _same_bytes(got["pairedRows"][l, :k], want["paired_rows"][l]), tag
        if with_feat:
            assert _same_bytes(got["pairedFeat"][l, :k], want["paired_feat"][l]), tag


# ---------------------------------------------------------------- scenes
def random_points3d(rng, n):
    """Local 3-D points in front of a camera, inside RANSAC's depth range."""
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), rng.uniform(1.0, 4.0, n)], axis=1)


def make_scene(rng, F, num_poses, max_obs=6, extra_poses=0):
    """(store, obs_point3d): map_view_ref.make_store's random front-end map over the first `num_poses` pose ids plus a random
    local point per observation; the pose table is `extra_poses` longer (ids nobody has observed from yet: the directed
    builders below use them)."""
    store = vref.make_store(rng, F, num_poses, max_obs=max_obs)
    store["num_poses"] = int(num_poses + extra_poses)
    return store, random_points3d(rng, len(store["obs_pose"]))


def unpack(store, p3d):
    """The store as the reference holds it: per feature a dict pose id -> observation (desc, octave, det_dist, point3D)."""
    start = store["obs_start"]
    return [{int(store["obs_pose"][o]): (store["obs_desc"][o].copy(), int(store["obs_octave"][o]), float(store["obs_det_dist"][o]),
                                         p3d[o].copy()) for o in range(int(start[f]), int(start[f + 1]))}
            for f in range(len(store["pos"]))]


def pack(store, feats):
    """(store, obs_point3d) from `unpack`'s form: every feature's observations in ascending pose id."""
    start, pose, desc, octave, det, p3d = [0], [], [], [], [], []
    for d in feats:
        for q in sorted(d):
            pose.append(q)
            desc.append(d[q][0])
            octave.append(d[q][1])
            det.append(d[q][2])
            p3d.append(d[q][3])
        start.append(len(pose))
    O = len(pose)
    out = dict(store)
    out.update(obs_start=np.array(start, np.int32), obs_pose=np.array(pose, np.int32).reshape(O),
               obs_desc=np.array(desc, np.uint8).reshape(O, 32), obs_octave=np.array(octave, np.int32).reshape(O),
               obs_det_dist=np.array(det, np.float64).reshape(O))
    return out, np.array(p3d, np.float64).reshape(O, 3)


def observe(rng, feats, q, features):
    """Pose q observes `features` (indices): a random descriptor and local point each (an existing observation stays)."""
    for f in features:
        feats[int(f)].setdefault(int(q), (rng.integers(0, 256, 32, dtype=np.uint8), int(rng.integers(0, 8)), float(rng.uniform(1, 4)),
                                          random_points3d(rng, 1)[0]))


def plant_loop(rng, feats, qa, qb, features, noise=0.003, flip=0.08, max_rot=0.2, max_shift=0.3):
    """A TRUE loop: poses qa and qb both observe `features`; the local points are consistent under one rigid motion with a few
    mm of noise, the descriptors of the two observations differ in ~8 % of their bits."""
    R = vref.rotation(rng.normal(size=3), rng.uniform(0.02, max_rot))
    t = rng.uniform(-max_shift, max_shift, 3)
    for f in features:
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        pa = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.8, 0.8), rng.uniform(1.5, 3.5)])
        pb = R @ pa + t + rng.normal(0, noise, 3)
        db = d ^ np.packbits(rng.random(256) < flip)
        feats[int(f)][int(qa)] = (d, int(rng.integers(0, 8)), float(np.linalg.norm(pa)), pa)
        feats[int(f)][int(qb)] = (db, int(rng.integers(0, 8)), float(np.linalg.norm(pb)), pb)


def store_device(store):
    from putslam_amd.device_batch import MapStoreDevice
    return MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                          store["obs_det_dist"], store["num_poses"])
