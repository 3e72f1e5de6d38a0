"""The tracking VO step, Matcher::trackKLT (reference src/Matcher/matcher.cpp:147-211), on the CPU, from pieces the project already
has: klt_ref.track and klt_ref.select_pairwise, the oracle's remove_image_distortion and keypoints2Dto3D under the dense-image depth
rule (frame_assembly_ref.assemble), the previous rows' columns carried by index, and the oracle's ransac_rigid3d on (previous points,
new points, the selection's matches) with seed + p -- behind the filter that states what ps_ransac_match_lists decides for lists the
host form cannot meet.  What ps_ransac_match_lists, ps_assemble_tracked and ps_track_vo_pairs (putslam_amd/csrc/ps_track_vo.h) must
equal byte for byte.

The scene: four 96 x 128 frames of one smooth texture, each moved against the one before, with a uint16 depth plane (scale 5000)
moved with the texture; the plane has a block of zeros (no depth) and a block beyond 6 m (RANSAC's depth gate).  A fifth frame is an
unrelated texture.  The previous points of frame 0 are klt_ref.random_points: some lie outside the image, and their rows are built
by hand (undistort, back-project, invented key point columns)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import frame_assembly_ref as A  # noqa: E402
import klt_ref as T  # noqa: E402
from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, STATS_DTYPE, default_ransac_params, make_config  # noqa: E402

f32 = np.float32
ROWS, COLS = 96, 128
WIN, LEVELS, MAX_COUNT, EPS = 7, 3, 30, 0.01
K = np.array([70.0, 0, 63.5, 0, 69.0, 47.5, 0, 0, 1], f32)       # a wide camera whose image is 128 x 96
DIST5 = (-0.0410, 0.3286, 0.0087, 0.0051, -0.5643)               # TUM fr1 (resources/datasetConfig/freiburg1_desk.xml:7)
DEPTH_SCALE = 5000.0
SHIFTS = ((1.3, -0.7), (0.8, 1.1), (-1.2, 0.6))                  # (x, y) flow of frame k -> k + 1
ERR_THRESHOLD, MIN_DIST = 25.0, 3.0                              # the shipped trackingErrorThreshold / minimalReprojDistance...
MINIMAL_TRACKED = 150                                            # ... and minimalTrackedFeatures
UNRELATED = 4                                                    # the frame that shows another texture
SEED, HYP = 7, 487
CARRIED = ("angle", "response", "octave", "det_dist")


def params():
    """RANSAC as shipped with errorVersionVO (0) in errorVersion"""
    return default_ransac_params(0)


def offsets():
    """where frame k's content lies against frame 0's: the running sum of SHIFTS"""
    out = [(0.0, 0.0)]
    for sx, sy in SHIFTS:
        out.append((out[-1][0] + sx, out[-1][1] + sy))
    return out


@functools.lru_cache(maxsize=None)
def images(cn):
    """frames 0 .. 3 of the moving texture and frame 4, an unrelated one"""
    out = [T.smooth_texture(ROWS, COLS, cn, seed=21, shift=(-ox, -oy)) for ox, oy in offsets()]
    return out + [T.smooth_texture(ROWS, COLS, cn, seed=99)]


@functools.lru_cache(maxsize=None)
def depths():
    """A depth image per frame: a tilted plane 2 .. 4.7 m with a block of zeros and a block at 6.4 m, moved with the texture; the
    unrelated frame sees frame 0's plane."""
    out = []
    for ox, oy in offsets() + [(0.0, 0.0)]:
        v, u = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
        u, v = u - ox, v - oy
        d = 10000 + 70 * u + 50 * v
        d[(u >= 20) & (u < 40) & (v >= 20) & (v < 40)] = 0
        d[(u >= 80) & (u < 100) & (v >= 50) & (v < 70)] = 32000
        out.append(np.clip(np.rint(d), 0, 65535).astype(np.uint16))
    return out


def first_rows(oracle, n, seed, frame=0):
    """The rows of a sequence's first frame, by hand: n random positions, their undistorted 3-D points in the frame's depth image and
    key point columns that are recognisable by index."""
    xy = T.random_points(ROWS, COLS, n, seed)
    rows = A.assemble(oracle, xy, np.arange(n, dtype=np.int32), depths()[frame], K, DIST5, DEPTH_SCALE)
    rng = np.random.RandomState(seed)
    return dict(xy=rows["xy"], xy_undist=rows["xy_undist"], pts=rows["pts"], det_dist=rows["det_dist"],
                angle=(rng.rand(n) * 360).astype(f32), response=rng.randn(n).astype(f32), octave=rng.randint(0, 8, size=n).astype(np.int32))


def dmatches(m3):
    """(k, 3) int (i, j, 0) -> DMatch(i, j, 0) with distance 0 (MatcherOpenCV::performTracking, matcherOpenCV.cpp:293)"""
    out = np.zeros(len(m3), DMATCH_DTYPE)
    if len(m3):
        out["queryIdx"], out["trainIdx"], out["imgIdx"] = m3[:, 0], m3[:, 1], m3[:, 2]
    return out


def empty_stats():
    s = np.zeros(1, STATS_DTYPE)[0]
    s["bestHypothesis"], s["pointInlierRatio"] = -1, np.nan
    return s


def ransac_list(oracle, prm, cfg, K, prev, cur, matches, valid=True):
    """One pair of ps_ransac_match_lists: dict(mask -- None where no byte is written --, pose (4, 4), stats).  prev / cur: the rows
    of the two sets that ARE points (count rows), or None for a set the pair cannot name.  The rules for what the host form refuses:
    valid = False (numMatches outside 0 .. cap), a set that is None: the empty list, no mask; a match whose index lies outside its
    set: filtered out in front of the oracle, its mask byte 0, numMatchesIn as given."""
    if not valid or prev is None or cur is None:
        r = oracle.ransac_rigid3d(prm, cfg, K, np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, DMATCH_DTYPE))
        return dict(mask=None, pose=r["pose"], stats=r["stats"])
    matches = np.asarray(matches, DMATCH_DTYPE)
    q, t = matches["queryIdx"].astype(np.int64), matches["trainIdx"].astype(np.int64)
    ok = (q >= 0) & (q < len(prev)) & (t >= 0) & (t < len(cur))
    r = oracle.ransac_rigid3d(prm, cfg, K, prev, cur, matches[ok])
    mask = np.zeros(len(matches), np.uint8)
    mask[np.nonzero(ok)[0]] = r["mask"]
    stats = r["stats"].copy()
    stats["numMatchesIn"] = len(matches)
    return dict(mask=mask, pose=r["pose"], stats=stats)


def ransac_lists(oracle, prm, K, prev_sets, cur_sets, pairs, matches, num_matches, cap, estimator=EST_RANSAC, H=HYP, seed=SEED,
                 prev_counts=None, cur_counts=None, prev_cap=None, cur_cap=None):
    """ps_ransac_match_lists: P pairs over lists of point sets; pair p draws from seed + p.  prev_counts / cur_counts override a set's
    count (a count outside 0 .. capacity makes every pair that names the set empty)."""
    out = []
    for p, n in enumerate(num_matches):
        a, b = (p, p) if pairs is None else (int(pairs[p][0]), int(pairs[p][1]))

        def pick(sets, counts, capacity, s):
            if not 0 <= s < len(sets):
                return None
            n_s = len(sets[s]) if counts is None else int(counts[s])
            if not 0 <= n_s <= (capacity if capacity is not None else max(n_s, 0)):
                return None
            return np.asarray(sets[s], f32).reshape(-1, 3)[:n_s]
        cfg, _ = make_config(estimator, H, seed=seed + p)
        valid = 0 <= int(n) <= cap
        out.append(ransac_list(oracle, prm, cfg, K, pick(prev_sets, prev_counts, prev_cap, a), pick(cur_sets, cur_counts, cur_cap, b),
                               matches[p][:max(int(n), 0)] if valid else None, valid))
    return out


def tracked_rows(oracle, next_pts, kept_idx, depth, prev=None):
    """ps_assemble_tracked for one pair: the rows kept_idx names.  depth None: no depth frame (points of depth 0)."""
    kept_idx = np.asarray(kept_idx, np.int32)
    d = depth if depth is not None else np.zeros((ROWS, COLS), np.uint16)
    r = A.assemble(oracle, next_pts, kept_idx, d, K, DIST5, DEPTH_SCALE)
    out = dict(xy=r["xy"], xy_undist=r["xy_undist"], pts=r["pts"])
    if prev is not None:
        for n in CARRIED:
            if n in prev:
                out[n] = np.asarray(prev[n])[kept_idx]
    return out


def step(oracle, cn, pair, rows, p, depth_frame=None, prm=None, estimator=EST_RANSAC, H=HYP, seed=SEED, err_threshold=ERR_THRESHOLD,
         min_dist=MIN_DIST):
    """matcher.cpp:147-211 for pair p = (previous frame, current frame) of the scene starting from `rows`.  Returns everything
    ps_track_vo_pairs writes for the pair: next_pts, status, err, matches, kept_idx, rows (the frame's), mask, pose (4, 4), stats."""
    prm = prm or params()
    imgs, deps = images(cn), depths()
    n = len(rows["xy"])
    nxt, status, err = (T.track(imgs[pair[0]], imgs[pair[1]], rows["xy"], WIN, LEVELS, MAX_COUNT, EPS) if n
                        else (np.zeros((0, 2), f32), np.zeros(0, np.uint8), np.zeros(0, f32)))
    kept, m3 = T.select_pairwise(nxt, status, err, err_threshold, min_dist)
    g = pair[1] if depth_frame is None else depth_frame
    new = tracked_rows(oracle, nxt, kept, deps[g] if 0 <= g < len(deps) else None, rows)
    matches = dmatches(m3)
    cfg, _ = make_config(estimator, H, seed=seed + p)
    r = ransac_list(oracle, prm, cfg, K, rows["pts"], new["pts"], matches)
    return dict(next_pts=nxt, status=status, err=err, matches=matches, kept_idx=kept, rows=new, mask=r["mask"], pose=r["pose"],
                stats=r["stats"])


def refill_step(counts, minimal=MINIMAL_TRACKED):
    """the first step whose rows count fewer than `minimal` points, len(counts) where none does"""
    for k, c in enumerate(counts):
        if c < minimal:
            return k
    return len(counts)


# The batches of the GPU tests, by capacity: (previous frame, current frame, previous points, their seed) -- the accepted pair, the
# next two of the sequence from hand-built rows, the unrelated pair (rejected) and a pair with two previous points (identity).
# The second batch is the same five kinds with at most 64 previous points each: a capacity below one block of 256 rows.
BATCH = [((0, 1), 260, 3), ((1, 2), 64, 4), ((2, 3), 150, 5), ((0, UNRELATED), 200, 6), ((0, 1), 2, 8)]
BATCH64 = [((0, 1), 64, 13), ((1, 2), 48, 14), ((2, 3), 63, 15), ((0, UNRELATED), 64, 16), ((1, 2), 2, 18)]
BATCHES = {300: BATCH, 64: BATCH64}


@functools.lru_cache(maxsize=None)
def batch(cn, capacity=300):
    """[(pair, first rows, the step's results)] of the batch for `capacity`, computed once"""
    from oracle import oracle_py
    oracle_py.build()
    out = []
    for p, (pair, n, seed) in enumerate(BATCHES[capacity]):
        rows = first_rows(oracle_py, n, seed, pair[0])
        out.append((pair, rows, step(oracle_py, cn, pair, rows, p)))
    return out
