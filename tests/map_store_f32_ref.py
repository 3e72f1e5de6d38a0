"""CPU answer and scenes for the resident store with FLOAT descriptor rows (ps_map_views_l2_device / ps_pose_sets_l2_device /
ps_loop_pairs_l2_device).

The reference runs the same code for both descriptor kinds (matcher.cpp:675-679 copies whatever cv::Mat row the observation holds;
matchFeatureLoopClosure, :802-861, pushes ext.descriptor rows into a Mat and calls performMatching), so nothing is restated a
second time here: a float store is a store of tests/map_view_ref.py / tests/loop_closure_ref.py with one more array, `rows`
(O, dim) float32, and the sequential walks of those modules -- build_view's per-feature walk, pose_sets' dict of observations per
pose in std::set order -- are run as they are; their answer is extended only by "the row is the observation's dim floats", taken
through the obsIdx they return.  Loop verification is l2_match_ref.match_l2 followed by the oracle's RANSAC with seed + l, the
way tests/test_gpu_l2_match.py forms its expectation for ps_vo_pairs_l2_device.
"""
import numpy as np

import l2_match_ref as l2ref
import loop_closure_ref as lref
import map_l2_ref as mref  # noqa: F401  (the guided matcher's restatement: the chain test of the views uses it)
import map_view_ref as vref

from putslam_amd._abi import DMATCH_DTYPE, PS_SET_INVALID, STATS_DTYPE, make_config

u32 = np.uint32


# ---------------------------------------------------------------- rows
def unit_rows(rng, n, dim):
    """SURF-like rows: unit length."""
    r = rng.normal(size=(n, dim))
    return (r / np.maximum(np.linalg.norm(r, axis=1, keepdims=True), 1e-12)).astype(np.float32)


SPECIAL_WORDS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7FBFFFFF,      # quiet / signalling NaNs with payloads
                          0x80000000, 0x00000000, 0x7F800000, 0xFF800000,      # -0.0, +0.0, +inf, -inf
                          0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF], u32)  # subnormals, FLT_MAX


def special_rows(rng, n, dim):
    """Rows whose words are drawn from SPECIAL_WORDS and random bit patterns: only a word-wise copy keeps them."""
    w = rng.integers(0, 2 ** 32, (n, dim), dtype=np.uint64).astype(u32)
    pick = rng.random((n, dim)) < 0.5
    w[pick] = SPECIAL_WORDS[rng.integers(0, len(SPECIAL_WORDS), int(pick.sum()))]
    return w.view(np.float32)


def float_store(store, rows):
    """`store` (map_view_ref.make_store's dict; its 32-byte rows stay for the trusted walks, nobody compares them) + float rows."""
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.ndim == 2 and rows.shape[0] == len(store["obs_pose"])
    out = dict(store)
    out["rows"] = rows
    return out


def same_words(a, b):
    return np.ascontiguousarray(a, np.float32).view(u32).tobytes() == np.ascontiguousarray(b, np.float32).view(u32).tobytes()


# ---------------------------------------------------------------- views
def _with_rows(fstore, answers):
    for w in answers:
        if w["rows"] is not None:
            w["rows"] = dict(w["rows"])
            w["rows"]["desc"] = fstore["rows"][w["rows"]["obsIdx"].astype(np.int64)].reshape(-1, fstore["rows"].shape[1])
    return answers


def build_views(fstore, cam_inv, pose_angle, max_angle, K, image, max_kpts, cand=None, cand_counts=None, require_visible=False,
                fast=False):
    """map_view_ref.build_views, every row's desc = the chosen observation's dim floats."""
    return _with_rows(fstore, vref.build_views(fstore, cam_inv, pose_angle, max_angle, K, image, max_kpts, cand, cand_counts,
                                               require_visible, fast))


def brute_view_rows(fstore, view):
    """The brute-force formulation of the extension: a (rows x observations) one-hot mask times nothing -- each row's
    observation found by equality over ALL observations, not by indexing."""
    obs = view["rows"]["obsIdx"]
    mask = obs[:, None] == np.arange(len(fstore["rows"]))[None, :]
    assert (mask.sum(axis=1) == 1).all()
    return fstore["rows"].view(u32)[np.nonzero(mask)[1]].view(np.float32)


VIEW_KEYS = ("pts", "mapLevel", "featIdx", "obsIdx", "posCam", "uv", "angle")


def compare_views(got, want, what=""):
    """got: MapViewsF32Device.download(); want: build_views' list.  Bytes (desc as 32-bit words), rows up to the count."""
    assert len(got["viewCount"]) >= len(want)
    for v, w in enumerate(want):
        tag = (what, v)
        assert int(got["viewCount"][v]) == w["viewCount"], (tag, int(got["viewCount"][v]), w["viewCount"])
        assert int(got["nkpts"][v]) == w["nkpts"], (tag, int(got["nkpts"][v]), w["nkpts"])
        n = w["nkpts"]
        if n:
            assert same_words(got["desc"][v, :n], w["rows"]["desc"]), (tag, "desc")
            for k in VIEW_KEYS:
                if k in got:
                    assert got[k][v, :n].tobytes() == w["rows"][k].tobytes(), (tag, k)


def views_as_scene(views, cap, dim):
    """build_views' answers as the arrays a host-filled PsMapBatchF32::maps holds."""
    V = len(views)
    pos, desc, level = np.zeros((V, cap, 3), np.float32), np.zeros((V, cap, dim), np.float32), np.zeros((V, cap), np.int32)
    for v, w in enumerate(views):
        n = w["nkpts"]
        if n:
            pos[v, :n], desc[v, :n], level[v, :n] = w["rows"]["pts"], w["rows"]["desc"], w["rows"]["mapLevel"]
    return dict(pos=pos, desc=desc, level=level, nkpts=np.array([w["nkpts"] for w in views], np.int32), cap=cap)


def kept_features(fstore, cam_inv, pose_angle, max_angle, K, image, require_visible=False):
    """Per view the features the whole store would emit (index order), by the fast formulation."""
    F = len(fstore["pos"])
    out = []
    for w in vref.build_views(fstore, cam_inv, pose_angle, max_angle, K, image, F, None, None, require_visible, fast=True):
        assert w["rows"] is not None
        out.append(w["rows"]["featIdx"].astype(np.int64))
    return out


def candidates_with_counts(rng, fstore, kept, counts, capacity):
    """(cand, cand_counts): view v's list holds exactly counts[v] features that are emitted, with features that are dropped
    mixed in between (ascending ids), so that view v's count is counts[v]."""
    F, V = len(fstore["pos"]), len(counts)
    cand, cc = np.full((V, capacity), -7, np.int32), np.zeros(V, np.int32)
    for v, n in enumerate(counts):
        assert len(kept[v]) >= n, (v, len(kept[v]), n)
        take = rng.choice(kept[v], n, replace=False)
        rest = np.setdiff1d(np.arange(F), kept[v])
        extra = rng.choice(rest, min(len(rest), capacity - n, 40 + n // 3), replace=False)
        c = np.sort(np.concatenate([take, extra]))
        cc[v] = len(c)
        cand[v, :len(c)] = c
    return cand, cc


SENTINEL = (0x5A5A5A5A, -123.0)     # (int32 / uint32 word, float)


def fill_sentinels(out):
    """Every array the library may write of a MapViewsF32Device / PoseSetsF32Device holds SENTINEL before the call."""
    import torch
    out.desc_flat.view(torch.int32).fill_(SENTINEL[0])
    out.pts.fill_(SENTINEL[1])
    for name in ("map_level", "feat_idx", "obs_idx"):
        t = getattr(out, name, None)
        if t is not None:
            t.fill_(SENTINEL[0])
    for name in ("pos_cam", "uv", "angle"):
        t = getattr(out, name, None)
        if t is not None:
            t.fill_(SENTINEL[1])
    torch.cuda.current_stream(out.device).synchronize()
    return out


def check_untouched(out, answers, what=""):
    """The WHOLE descriptor allocation of `out`, word for word: the rows of `answers` where they belong, SENTINEL everywhere else
    -- in front of an offset base, between the rows of a pitched set, in rows beyond the count and in every row of an overflowed
    or invalid set; the same for the points and the int32 side arrays."""
    import torch
    torch.cuda.synchronize(out.device)
    flat = out.desc_flat.view(torch.int32).cpu().numpy().view(u32)
    want = np.full(flat.shape, SENTINEL[0], u32)
    n_alloc, cap = out.desc.shape[0], out.max_kpts
    rows = want[out.offset_floats:].reshape(n_alloc, cap, out.row_floats)
    pts = np.full((n_alloc, cap, 3), SENTINEL[1], np.float32)
    for v, w in enumerate(answers):
        n = w["nkpts"]
        if n:
            rows[v, :n, :out.dim] = np.ascontiguousarray(w["rows"]["desc"], np.float32).view(u32)
            pts[v, :n] = w["rows"]["pts"]
    bad = np.nonzero(flat != want)[0]
    assert len(bad) == 0, (what, "descriptor words", len(bad), bad[:8])
    assert out.pts.cpu().numpy().tobytes() == pts.tobytes(), (what, "pts")
    for name, key in (("map_level", "mapLevel"), ("feat_idx", "featIdx"), ("obs_idx", "obsIdx")):
        t = getattr(out, name, None)
        if t is None:
            continue
        side = np.full((n_alloc, cap), SENTINEL[0], np.int32)
        for v, w in enumerate(answers):
            if w["nkpts"]:
                side[v, :w["nkpts"]] = w["rows"][key]
        assert t.cpu().numpy().tobytes() == side.tobytes(), (what, name)


# ---------------------------------------------------------------- pose sets
def pose_sets(fstore, p3d, poses, max_kpts, fast=False):
    """loop_closure_ref.pose_sets (fast: its brute-force mask formulation), every row's desc = that observation's dim floats."""
    return _with_rows(fstore, (lref.pose_sets_fast if fast else lref.pose_sets)(fstore, p3d, poses, max_kpts))


def compare_sets(got, want, sentinel=None, what=""):
    """got: PoseSetsF32Device.download(); want: pose_sets' list.  sentinel = (int32 word, float): rows beyond every count, every
    row of an overflowed / invalid set and the empty set still hold it."""
    S = len(want)
    assert len(got["setCount"]) == S and int(got["nkpts"][S]) == 0, what
    for s, w in enumerate(want):
        tag = (what, s)
        assert int(got["setCount"][s]) == w["setCount"], (tag, int(got["setCount"][s]), w["setCount"])
        assert int(got["nkpts"][s]) == w["nkpts"], tag
        n = w["nkpts"]
        if n:
            assert same_words(got["desc"][s, :n], w["rows"]["desc"]), (tag, "desc")
            for k in ("pts", "featIdx", "obsIdx"):
                if k in got:
                    assert got[k][s, :n].tobytes() == w["rows"][k].tobytes(), (tag, k)
        if sentinel is not None:
            assert (got["desc"][s, n:].view(u32) == sentinel[0]).all() and (got["pts"][s, n:] == sentinel[1]).all(), tag
            if "featIdx" in got:
                assert (got["featIdx"][s, n:] == sentinel[0]).all() and (got["obsIdx"][s, n:] == sentinel[0]).all(), tag
    if sentinel is not None:
        assert (got["desc"][S].view(u32) == sentinel[0]).all() and (got["pts"][S] == sentinel[1]).all(), (what, "empty set")


def sets_as_frames(sets, max_kpts, dim):
    S = len(sets)
    desc, pts = np.zeros((S + 1, max_kpts, dim), np.float32), np.zeros((S + 1, max_kpts, 3), np.float32)
    nk, feat = np.zeros(S + 1, np.int32), np.zeros((S + 1, max_kpts), np.int32)
    for s, w in enumerate(sets):
        n = w["nkpts"]
        nk[s] = n
        if n:
            desc[s, :n], pts[s, :n], feat[s, :n] = w["rows"]["desc"], w["rows"]["pts"], w["rows"]["featIdx"]
    return desc, pts, nk, feat


# ---------------------------------------------------------------- the loop
def verify(oracle, sets, pairs, params, est, H, seed, K, min_features, threshold, max_kpts, dim):
    """loop_closure_ref.verify with the float matcher: the gate is that module's, candidate l's matches are
    l2_match_ref.match_l2 on its effective pair (the empty set for a gated or invalid one) and its estimate is the oracle's RANSAC
    with seed + l.  The same dict; pair = dict(numMatches, matches / inlierMask (lists), pose (L, 16) float32, stats)."""
    S, L = len(sets), len(pairs)
    desc, pts, nk, feat = sets_as_frames(sets, max_kpts, dim)
    state = [lref.gate(sets, int(a), int(b), min_features) for a, b in pairs]
    eff = np.array([(a, b) if st == lref.RUN else (S, S) for (a, b), st in zip(pairs, state)], np.int32).reshape(L, 2)
    ratio, closed, num, rows, feats = np.zeros(L), np.zeros(L, np.int32), np.zeros(L, np.int32), [], []
    pair = dict(numMatches=np.zeros(L, np.int32), matches=[], inlierMask=[], pose=np.zeros((L, 16), np.float32),
                stats=np.zeros(L, STATS_DTYPE))
    cache = {}
    for l in range(L):
        a, b = (int(x) for x in eff[l])
        if (a, b) not in cache:
            cache[(a, b)] = l2ref.match_l2(desc[a, :nk[a]], desc[b, :nk[b]])
        m = cache[(a, b)]
        cfg, _keep = make_config(est, H, seed=seed + l)
        c = oracle.ransac_rigid3d(params, cfg, K, pts[a], pts[b], m)
        pair["numMatches"][l] = len(m)
        pair["matches"].append(m)
        pair["inlierMask"].append(np.asarray(c["mask"], np.uint8))
        pair["pose"][l] = c["pose"].T.astype(np.float32).reshape(16)
        for f in lref.STAT_FIELDS:
            pair["stats"][l][f] = c["stats"][f]
        r, pr = 0.0, np.zeros((0, 2), np.int32)
        if state[l] == lref.RUN:
            if len(m) == 0:
                r = -1.0                                     # matcher.cpp:838-839
            else:
                mi = m[np.asarray(c["mask"]) != 0]
                pr = np.stack([mi["queryIdx"], mi["trainIdx"]], axis=1).astype(np.int32).reshape(-1, 2)
                r = float(pair["stats"][l]["pointInlierRatio"])
        ratio[l], closed[l] = r, 1 if r > threshold and state[l] != lref.INVALID_PAIR else 0
        num[l] = PS_SET_INVALID if state[l] == lref.INVALID_PAIR else len(pr)
        rows.append(pr)
        feats.append(np.stack([feat[a][pr[:, 0]], feat[b][pr[:, 1]]], axis=1).astype(np.int32).reshape(-1, 2))
    return dict(state=state, ratio=ratio, closed=closed, numPaired=num, paired_rows=rows, paired_feat=feats, pair=pair, eff=eff)


def compare_verdicts(got, want, with_feat=True, what=""):
    """got: LoopBatchF32Device.download(); want: verify's dict.  Byte for byte (NaN stats fields compare as NaN)."""
    same = lambda a, b: np.asarray(a).tobytes() == np.asarray(b).tobytes()   # noqa: E731
    L = len(want["state"])
    assert same(got["numMatches"], want["pair"]["numMatches"]), (what, got["numMatches"], want["pair"]["numMatches"])
    assert same(got["pose"], want["pair"]["pose"]), what
    for l in range(L):
        tag = (what, l, want["state"][l])
        n = int(want["pair"]["numMatches"][l])
        assert same(got["matches"][l, :n], want["pair"]["matches"][l]), tag
        assert same(got["inlierMask"][l, :n], want["pair"]["inlierMask"][l]), tag
        for f in lref.STAT_FIELDS:
            x, y = got["stats"][l][f], want["pair"]["stats"][l][f]
            assert same(x, y) or (np.isnan(x) and np.isnan(y)), (tag, f, x, y)
        assert same(np.float64(got["ratio"][l]), np.float64(want["ratio"][l])), (tag, got["ratio"][l], want["ratio"][l])
        assert int(got["closed"][l]) == int(want["closed"][l]), tag
        assert int(got["numPaired"][l]) == int(want["numPaired"][l]), (tag, int(got["numPaired"][l]))
        k = len(want["paired_rows"][l])
        assert same(got["pairedRows"][l, :k], want["paired_rows"][l]), tag
        if with_feat:
            assert same(got["pairedFeat"][l, :k], want["paired_feat"][l]), tag


# ---------------------------------------------------------------- the loop scene
POSE0 = 8                 # poses 8 .. 22 of the scene are the directed ones: set index = pose id - POSE0
SIZES = {14: 35, 15: 36, 16: 9, 17: 10, 18: 11, 19: 40, 21: 5}
EMPTIED = 11              # the set (pose 19, 40 members) whose keypoint count is set to 0 behind the call: a RUN candidate
                          # without matches, the reference's -1.0 (cross-check matching of two non-empty sets always matches)
PAIRS = np.array([[0, 1], [1, 0], [2, 3], [4, 5], [0, 4], [0, 5], [0, 2], [0, 0], [6, 0], [0, 6], [7, 0], [8, 0], [9, 0], [0, 9],
                  [10, 0], [11, 0], [0, 11], [12, 0], [13, 1], [4, 4], [5, 7], [-1, 0], [0, 15], [2 ** 31 - 1, -2 ** 31]], np.int32)


def plant_loop(rng, feats, side, qa, qb, features, dim, sigma=0.02):
    """A TRUE loop: loop_closure_ref.plant_loop's geometry (one rigid motion, 3 mm of noise on the local points); the two
    observations of every shared feature carry its base row plus small Gaussian noise on each side."""
    lref.plant_loop(rng, feats, qa, qb, features, noise=0.003)
    base = unit_rows(rng, len(features), dim)
    for i, f in enumerate(features):
        side[(int(f), int(qa))] = (base[i] + rng.normal(0, sigma / np.sqrt(dim), dim)).astype(np.float32)
        side[(int(f), int(qb))] = (base[i] + rng.normal(0, sigma / np.sqrt(dim), dim)).astype(np.float32)


def loop_scene(dim, seed=2026):
    """tests/test_gpu_loop_closure.py's scene with float rows: two planted loops (150 and 300 shared features; the second
    overflows a capacity of 256), unrelated sets, sets of 35 / 36 / 9 / 10 / 11 / 40 / 5 members around the two gates, poses
    nobody observed from.  Returns dict(store (a float store), p3d, poses, pairs, S)."""
    rng = np.random.default_rng(seed)
    store, p3d = lref.make_scene(rng, 1200, 8, max_obs=4, extra_poses=15)
    feats, side = lref.unpack(store, p3d), {}
    plant_loop(rng, feats, side, 8, 9, range(0, 150), dim)
    plant_loop(rng, feats, side, 10, 11, range(150, 450), dim)
    lref.observe(rng, feats, 12, range(400, 460))
    lref.observe(rng, feats, 13, range(500, 580))
    at = 600
    for q, n in SIZES.items():
        lref.observe(rng, feats, q, range(at, at + n))
        at += n + 3
    store, p3d = lref.pack(store, feats)
    rows = unit_rows(rng, len(store["obs_pose"]), dim)
    start = store["obs_start"]
    for f in range(len(store["pos"])):
        for o in range(int(start[f]), int(start[f + 1])):
            r = side.get((f, int(store["obs_pose"][o])))
            if r is not None:
                rows[o] = r
    return dict(store=float_store(store, rows), p3d=p3d, poses=np.arange(POSE0, 23, dtype=np.int32), pairs=PAIRS.copy(),
                S=23 - POSE0, dim=dim)


def emptied(sets):
    sets = list(sets)
    sets[EMPTIED] = dict(setCount=sets[EMPTIED]["setCount"], nkpts=0, rows=None)
    return sets


def store_device(fstore, **kw):
    from putslam_amd.device_batch import MapStoreF32Device
    return MapStoreF32Device(fstore["pos"], fstore["obs_start"], fstore["obs_pose"], fstore["rows"], fstore["obs_octave"],
                             fstore["obs_det_dist"], fstore["num_poses"], **kw)
