"""The second half of Matcher::trackKLT (reference src/Matcher/matcher.cpp:213-381) on the CPU, one pair at a time, in the
reference's order, from pieces the project already has: the sandbox of :218-246 (orb_detect_ref, dbscan_ref_py, the oracle's
remove_image_distortion / keypoints2Dto3D and the detection distance of frame_assembly_ref), mergeTrackedFeatures
(exclusion_ref_py.merge_tracked_features: the real square root against the threshold itself, no squared bound), the predicted level
(:281-301, ps_predicted_level: the host's libm, no thresholds, no tables), the level buckets of :302-331, orb_ref.describe on key
points that carry the level as octave, and the position-matching walk of :359-375 done LITERALLY -- it does not go through the
description's keptIdx, so that "the walk selects exactly keptIdx" is a claim tests/test_track_close_ref_host.py can hold.  What
ps_track_candidates and ps_track_close_pairs (putslam_amd/csrc/ps_track_close.h) must equal byte for byte.

Three things the reference does not define are stated here as the library documents them: a pair that is due without candidates
closes without the refill (refill = 2); a quotient of the level rule that is not finite (curDist 0) gives level 0 -- the x86 cast
of NaN / inf to int is INT_MIN, which :297 clamps to 0 --; an octave outside PS_LEVEL_OCTAVE_MIN .. MAX gives level -1 and the row
is dropped with the rows the description drops (the reference would index keyPointsLevel[-1])."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dbscan_ref_py as DB  # noqa: E402
import exclusion_ref_py as X  # noqa: E402
import frame_assembly_ref as A  # noqa: E402
import orb_detect_ref as D  # noqa: E402
import orb_ref as O  # noqa: E402
from putslam_amd._abi import PS_LEVEL_OCTAVE_MAX, PS_LEVEL_OCTAVE_MIN  # noqa: E402

f32 = np.float32
COLUMNS = (("xy", f32, (2,)), ("xy_undist", f32, (2,)), ("pts", f32, (3,)), ("angle", f32, ()), ("response", f32, ()),
           ("octave", np.int32, ()), ("det_dist", np.float64, ()))
SCALE_FACTOR, N_LEVELS = 1.2, 8          # Matcher's constants (matcher.h:26-28)
MINIMAL_TRACKED, MIN_DIST = 150, 3.0     # the shipped minimalTrackedFeatures / minimalReprojDistanceNewTrackingFeatures


def empty_rows():
    return {n: np.zeros((0,) + tail, dt) for n, dt, tail in COLUMNS}


def take(rows, idx):
    idx = np.asarray(idx, np.int64)
    return {n: np.ascontiguousarray(np.asarray(rows[n], dt).reshape((-1,) + tail)[idx]) for n, dt, tail in COLUMNS}


def candidates(oracle, img, depth, p, eps, K=A.K, dist5=A.DIST5, scale=A.DEPTH_SCALE):
    """:218-246 for one frame: detectFeatures, DBScan::run, removeImageDistortion, keypoints2Dto3D and the detection distances.
    Nothing is described.  Returns the sandbox rows (COLUMNS)."""
    xy, resp, ang, octv = D.detect_closed(img, p)
    keep = DB.dbscan_keep(xy, octv, eps, 2, 1)
    r = A.assemble(oracle, xy, keep, depth, K, dist5, scale, angle=ang, response=resp, octave=octv)
    return {n: r[n] for n, _, _ in COLUMNS}


def cur_dist(pts):
    """:287-290 as the compiler sees it: float products, float sums left to right, the float root, widened"""
    return A.det_dist(pts)


def predicted_levels(octave, det_dist, pts):
    """:283-299 per row; -1 for an octave outside the level table, 0 for a quotient that is not finite"""
    from putslam_amd import _lib
    L = _lib.load()
    cur = cur_dist(pts)
    out = np.zeros(len(cur), np.int32)
    for i, (o, dd, cd) in enumerate(zip(np.asarray(octave, np.int32), np.asarray(det_dist, np.float64), cur)):
        if not PS_LEVEL_OCTAVE_MIN <= int(o) <= PS_LEVEL_OCTAVE_MAX:
            out[i] = -1
            continue
        with np.errstate(all="ignore"):
            x = np.float64(math.pow(SCALE_FACTOR, int(o))) * np.float64(dd) / np.float64(cd)
        out[i] = int(L.ps_predicted_level(int(o), float(dd), float(cd))) if np.isfinite(x) else 0
    return out


def close(tracked, cand, pyr, capacity, minimal=MINIMAL_TRACKED, min_dist=MIN_DIST):
    """matcher.cpp:213-381 for one pair.  tracked / cand: rows (COLUMNS; cand None = no candidates given), pyr: orb_ref.pyramid of
    the current image, capacity: the tracked block's (srcIdx of candidate i is capacity + i).  Returns dict(desc (k, 32), the rows'
    COLUMNS (k rows), src_idx (k,), refill, and for the host test: level (of every merged row), merged_src, walk (the merged
    rows the walk of :359-375 selected), kept (the merged rows the description kept, in described order))."""
    rows = take(tracked, np.arange(len(tracked["xy"])))
    n = len(rows["xy"])
    src = np.arange(n, dtype=np.int64)
    refill = 0
    if n < minimal:                                                                           # :214-215
        if cand is None:
            refill = 2
        else:
            refill = 1
            acc = X.merge_tracked_features(rows["xy_undist"], cand["xy_undist"], min_dist)     # :251-260
            add = take(cand, acc)
            rows = {k: np.concatenate([rows[k], add[k]]) for k in rows}
            src = np.concatenate([src, capacity + acc.astype(np.int64)])
    level = predicted_levels(rows["octave"], rows["det_dist"], rows["pts"])                   # :281-301
    # :302-331: keyPointsLevel[level] buckets, every column reordered -- descKeyPoints is NOT (ORB::compute orders it itself)
    order = [i for l in range(N_LEVELS) for i in range(len(level)) if level[i] == l]
    have = np.nonzero(level >= 0)[0]                                                          # (the extension: level -1 is no key point)
    desc, kept = O.describe(pyr, rows["xy"][have], rows["angle"][have], level[have])          # :338
    desc_pts = rows["xy"][have][kept]                                                         # descKeyPoints[j].pt after compute
    walk = order
    if len(desc_pts) != len(order):                                                           # :343
        walk, j = [], 0
        for i in order:                                                                       # :359-375
            if j == len(desc_pts):
                break
            with np.errstate(invalid="ignore"):
                if X._norm2_f64(rows["xy"][i], desc_pts[j]) < 0.0001:
                    walk.append(i)
                    j += 1
    walk = np.asarray(walk, np.int64)
    out = take(rows, walk)
    out.update(desc=desc, src_idx=src[walk].astype(np.int32), refill=refill, level=level, merged_src=src, walk=walk,
               kept=have[kept].astype(np.int64))
    return out


# ---- inputs shared by the host and the device tests ----
def random_rows(n, seed, rows=A.ROWS, cols=A.COLS, octaves=(0, 8)):
    """n rows whose positions cover the image, the 31-pixel border included, whose undistorted positions lie half a pixel off and
    whose detection distances put the predicted level up to three levels either side of the detection octave"""
    rng = np.random.RandomState(seed)
    xy = (rng.rand(n, 2) * [cols, rows]).astype(f32)
    pts = np.stack([rng.randn(n), rng.randn(n), 0.5 + 3.5 * rng.rand(n)], axis=1).astype(f32)
    return dict(xy=xy, xy_undist=(xy + 0.5 * rng.randn(n, 2)).astype(f32), pts=pts, angle=(rng.rand(n) * 360).astype(f32),
                response=rng.randn(n).astype(f32), octave=rng.randint(octaves[0], octaves[1], size=n).astype(np.int32),
                det_dist=cur_dist(pts) * (0.6 + 1.1 * rng.rand(n)))


def rows_at(und, seed=0, xy=None):
    """rows with the given undistorted positions (and xy: default the same), everything else random but describable"""
    und = np.asarray(und, f32).reshape(-1, 2)
    r = random_rows(len(und), seed)
    r["xy_undist"] = und
    r["xy"] = und.copy() if xy is None else np.asarray(xy, f32).reshape(-1, 2)
    return r


def near_and_far_candidates(tracked, n, seed, min_dist=MIN_DIST):
    """n candidates: every other one a pixel from a tracked row (rejected), the rest random (most accepted, some near each other)"""
    c = random_rows(n, seed)
    k = len(tracked["xy"])
    if k:
        for i in range(0, n, 2):
            c["xy_undist"][i] = tracked["xy_undist"][i % k] + f32(1.0)
    return c


def move_copies(cand, src, dst, step=(1.0, 0.0)):
    """Candidates dst become candidates src moved by `step` pixels (image and undistorted position; every other column copied).
    A copy is rejected because of its original where the original was accepted, and may be accepted where it was itself rejected."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    for n, _, _ in COLUMNS:
        cand[n][dst] = cand[n][src]
    cand["xy"][dst] += np.asarray(step, f32)
    cand["xy_undist"][dst] += np.asarray(step, f32)
    return cand


# The seams of the merge (ps_track_merge_rows passes candidates, and stages what it sweeps them against, MERGE_TILE at a time):
# tracked rows that need a second and a third trip, candidates that fill a third and a fifth tile, more than a tile of accepted
# candidates before the last one, and copies in the third tile of candidates of the first.
MERGE_TILE = 256
SEAM_CAP, SEAM_CCAP = 520, 1100                 # the capacities of the seam cases' own blocks
SEAM_TRACKED, SEAM_CANDIDATES = (255, 256, 257, 513), (513, 1100)
SEAM_MINIMAL = max(SEAM_TRACKED) + 1            # every case is due
SEAM_COPIES = (512, 601)                        # candidates 512 .. 600 are candidates 0 .. 88 moved by one pixel
# The distance of the seam cases.  near_and_far_candidates puts every other candidate at (1, 1) from a tracked row: 1.41 px, rejected;
# its copy lies at (2, 1), 2.24 px: free of that row, accepted unless something else is near.  The copy of an accepted candidate lies
# 1 px from it: rejected because of a candidate two tiles earlier.
SEAM_MIN_DIST = 2.0


def seam_case(n_tracked, n_cand):
    """(tracked rows, candidates) of one seam case"""
    tracked = random_rows(n_tracked, 50 + n_tracked)
    cand = near_and_far_candidates(tracked, n_cand, 60 + n_tracked + n_cand)
    dst = np.arange(SEAM_COPIES[0], min(SEAM_COPIES[1], n_cand))
    return tracked, move_copies(cand, dst - SEAM_COPIES[0], dst)


def merge_seams(tracked, cand, min_dist=MIN_DIST):
    """What mergeTrackedFeatures goes through on these rows, from the restatement alone: dict(accepted -- the candidates merged --,
    before_last -- how many of them lie before the last tile --, earlier_only -- the rejected candidates near no tracked row and
    near no accepted candidate of their own tile: rejected only because of a candidate accepted in an EARLIER tile --,
    second_trip_only -- those of them near none of the first MERGE_TILE accepted candidates either: a sweep that stops after one
    trip over the accepted candidates would accept them)."""
    und_t, und_c = np.asarray(tracked["xy_undist"], f32).reshape(-1, 2), np.asarray(cand["xy_undist"], f32).reshape(-1, 2)
    nc = len(und_c)
    acc = np.asarray(X.merge_tracked_features(und_t, und_c, min_dist), np.int64)
    accepted = set(acc.tolist())
    earlier_only, second_trip_only = [], []
    for i in range(MERGE_TILE, nc):
        if i in accepted or X.near_merge(und_t, und_c[i], min_dist).any():
            continue
        t0 = i // MERGE_TILE * MERGE_TILE
        own = acc[(acc >= t0) & (acc < i)]
        if len(own) and X.near_merge(und_c[own], und_c[i], min_dist).any():
            continue
        earlier_only.append(i)
        first_trip = acc[acc < t0][:MERGE_TILE]
        if not X.near_merge(und_c[first_trip], und_c[i], min_dist).any():
            second_trip_only.append(i)
    last = (nc - 1) // MERGE_TILE * MERGE_TILE if nc else 0
    return dict(accepted=acc, before_last=int((acc < last).sum()), earlier_only=earlier_only, second_trip_only=second_trip_only)


# ---- the whole tracked frame: matcher.cpp:147-381, and sequences of them ----
def track_step(oracle, img_prev, img_cur, depth_cur, rows, seed, prm=None, K=A.K, dist5=A.DIST5, scale=A.DEPTH_SCALE):
    """:147-211 on any pair of images (track_vo_ref.step on its own scene): dict(rows -- the tracked rows, COLUMNS --, pose (4, 4),
    mask, stats, matches).  RANSAC draws from `seed`."""
    import klt_ref as T
    import track_vo_ref as V
    from putslam_amd._abi import EST_RANSAC, make_config
    prm = prm or V.params()
    n = len(rows["xy"])
    nxt, status, err = (T.track(img_prev, img_cur, rows["xy"], V.WIN, V.LEVELS, V.MAX_COUNT, V.EPS) if n
                        else (np.zeros((0, 2), f32), np.zeros(0, np.uint8), np.zeros(0, f32)))
    kept, m3 = T.select_pairwise(nxt, status, err, V.ERR_THRESHOLD, MIN_DIST)
    kept = np.asarray(kept, np.int32)
    r = A.assemble(oracle, nxt, kept, depth_cur, K, dist5, scale)
    new = dict(xy=r["xy"], xy_undist=r["xy_undist"], pts=r["pts"])
    for name in V.CARRIED:
        new[name] = np.asarray(rows[name])[kept]
    cfg, _ = make_config(EST_RANSAC, V.HYP, seed=seed)
    res = V.ransac_list(oracle, prm, cfg, K, np.asarray(rows["pts"], f32).reshape(-1, 3), new["pts"], V.dmatches(m3))
    return dict(rows=new, pose=res["pose"], mask=res["mask"], stats=res["stats"], matches=V.dmatches(m3))


def tracked_vo(oracle, imgs, deps, frames, rows0, capacity, cand_capacity, p, eps, minimal, seed, describe_levels=N_LEVELS):
    """S sequences of K tracked frames (frames (S, K + 1) indices into imgs / deps) from the rows rows0[s]: per step :147-211, the
    sandbox where the refill is due, and :213-381.  Pair s of step k draws from seed + s.  The tracked block of step k holds
    capacity + k x cand_capacity rows (srcIdx of candidate i is that + i).  Returns [[dict(step, closed)] per step] per sequence."""
    out = []
    for s, fr in enumerate(frames):
        rows, seq = rows0[s], []
        for k in range(len(fr) - 1):
            a, b = int(fr[k]), int(fr[k + 1])
            st = track_step(oracle, imgs[a], imgs[b], deps[b], rows, seed + s)
            due = len(st["rows"]["xy"]) < minimal
            cand = candidates(oracle, imgs[b], deps[b], p, eps) if due else None
            closed = close(st["rows"], cand, O.pyramid(imgs[b], p["scale_factor"], describe_levels), capacity + k * cand_capacity, minimal)
            seq.append(dict(step=st, closed=closed))
            rows = closed
        out.append(seq)
    return out
