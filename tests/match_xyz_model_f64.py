"""Guided map matching restated in plain float64 numpy (no GPU, nothing from oracle/, no restatement of this project), plus the
scenes and the check that tests/test_match_xyz_model_host.py (oracle.match_xyz and map_l2_ref.match_xyz_l2 against this model),
tests/test_gpu_match_xyz_model.py (the kernels against this model) and tests/fuzz_gpu.py::run_map share.

Written from the reference's src/Matcher/matcher.cpp alone (line numbers below), not from oracle/putslam_oracle.c, tests/map_l2_ref.py
or the kernels, and independent of them: it never forms a squared sphere bound, takes every distance and every float value in
float64 by numpy's own reductions, and gets the binary value from unpackbits.

  ladder (:617-622)            try k > 1: radius + 0.02 (k - 1), max(0.1, ratio - 0.05 (k - 1)), in double; try 1 as given
  predicted level (:643-651,   clamp(ceil(log(1.2^octave detDist / curDist) / log 1.2), 0, 7); an input whose quotient lies
                   :683-692)   within 1e-9 of an integer is ambiguous (a libm may put it on either side)
  candidates (:699-711)        d = |map - cur| in float64 from the float32 inputs; norm < radius, and
                               curLevel - 1 <= mapLevel <= curLevel + 1
  value (:719-721)             binary: popcount of the per-byte SATURATING map - cur (cv::Mat subtraction of CV_8U), exact;
                               float: sqrt(sum(((double)map_k - (double)cur_k)^2)), in whatever order numpy sums
  best (:714-726)              the first candidate whatever its value, a later one only if value < bestVal
  emit (:734-746)              every candidate with ratio * (double)value <= (double)bestVal, in ascending i, features in
                               ascending j, imgIdx -1 (a default-constructed cv::DMatch)

A float32 implementation cannot be compared with this decision for decision where a keypoint lies within rounding of the sphere
or a value within rounding of the ratio line.  Such features are marked AMBIGUOUS and held to less (their matches must come from
the outer candidate set); check() caps their share per scene at AMBIGUOUS_CAP, so a scene cannot hide behind them.
  sphere   certainly inside: d < r (1 - W); certainly outside: d >= r (1 + W); W = 1e-6.  A float32 norm (three subtractions,
           three squares, two additions, a root) is within (1 + u)^3.5 - 1 = 2.1e-7 of the real one in any summation order
           (u = 2^-24); the comparison with the double radius is exact.  W leaves a factor of four.
  ratio    float values only (the binary rule is exact: one IEEE product of a double and a small integer on either side): some
           candidate has |ratio v - best| <= 1e-6 best, or two least values lie within 1e-6 of each other and taking the other
           one as bestVal changes what is emitted.  The float32 value of the definition is within 2 u of the model's.
MUTATIONS are other readings of the same lines; the host test shows that each of them fails check() against the unmodified
implementations.

MEASURED (CPU only: python tests/match_xyz_model_f64.py, and tests/test_match_xyz_model_host.py with -s)
  float32 norm   the model's own float32 run of the norm against its float64 run over the five scenes of SCENES (2 279 920
                 (feature, keypoint) pairs): the largest |d32 / d64 - 1| is 1.82e-07, under the 2.2e-7 of the derivation and a
                 fifth of W (test_float32_norm_stays_inside_the_margin asserts both).  Of those pairs, against the ten ladder
                 radii (22.8 M comparisons), 0 lie within W of a radius.
  ambiguous      share of the features with candidates, cap 0.5 %: binary 0 of 4 886 over the five scenes x tries 1, 5, 10
                 (the binary ratio line is exact and never ambiguous); float RATIO LINE: 0 of 4 962 (SURF), 0 of 5 016 (SIFT),
                 0 of 4 973 (width 20); sphere: one feature of the width-20 scene 1000 x 1100 at try 5 (1 of 803, 0.12 %), none
                 elsewhere.  The 40 random configurations of the GPU fuzz slice and every scene of the GPU tests: 0.
  float value    worst |distance / model - 1| of map_l2_ref's restated value: 1.18 u (SURF), 0.98 u (SIFT), 1.35 u (width 20);
                 of the kernels' on the GPU tests' scenes 1.09 u; the check's bound is 4 u.
  mutations      features flipped / distances off on the host test's mutation cases (two random scenes x tries 1, 5, 10 and the
                 directed scenes; binary rows against oracle.match_xyz, no_sqrt on SURF rows against map_l2_ref.match_xyz_l2):
                   cur_minus_map 105 / 846   xor 68 / 967       window0 485 / 0     window2 319 / 0      strict_ratio 1 / 0
                   ratio_on_best 780 / 0     first_best 112 / 0  ladder_k 87 / 0     no_sqrt 70 / 1127    best_only 161 / 0
                 (strict_ratio can only show on an exact tie: the directed scene with 0.5 x 16 == 8 is the one feature.)
"""
import numpy as np

U = 2.0 ** -24
W = 1e-6                  # the sphere's margin: 4 x (1 + u)^3.5 - 1, rounded up (module docstring)
RATIO_BAND = 1e-6         # the ratio line's margin, relative to bestVal
DIST_TOL = 4 * U          # float distance against the model's value
LEVEL_BAND = 1e-9
AMBIGUOUS_CAP = 0.005     # share of a scene's features with candidates that may be ambiguous
NORM32_BOUND = 2.2e-7

MUTATIONS = ("cur_minus_map", "xor", "window0", "window2", "strict_ratio", "ratio_on_best", "first_best", "ladder_k", "no_sqrt",
             "best_only")
BINARY_MUTATIONS = tuple(m for m in MUTATIONS if m != "no_sqrt")

# nmap x ncur of the random scenes (1023 / 1025: either side of a tile of 1024 keypoints)
SCENES = ((65, 1023), (257, 1025), (500, 500), (1000, 1100), (300, 2000))
TRIES = (1, 5, 10)
RADIUS, RATIO = 0.12, 0.55          # matchingXYZSphereRadius / matchingXYZacceptRatioOfBestMatch of the reference's settings


# ------------------------------------------------------------------------------------------------ pieces
def ladder(radius, ratio, k, mutation=None):
    """(radius, ratio) of try k = 1, 2, ... (:617-622)."""
    radius, ratio = float(radius), float(ratio)
    if mutation == "ladder_k":
        return radius + 0.02 * k, (max(0.1, ratio - 0.05 * (k - 1)) if k > 1 else ratio)
    if k > 1:
        return radius + 0.02 * (k - 1), max(0.1, ratio - 0.05 * (k - 1))
    return radius, ratio


def predicted_level(octave, det_dist, cur_dist):
    """(level, ambiguous) of :643-651 / :683-692, elementwise."""
    with np.errstate(all="ignore"):
        x = np.power(1.2, np.asarray(octave, np.float64)) * np.asarray(det_dist, np.float64) / np.asarray(cur_dist, np.float64)
        q = np.log(x) / np.log(1.2)
        level = np.clip(np.ceil(q), 0, 7).astype(np.int64)
        return level, np.abs(q - np.rint(q)) < LEVEL_BAND


def distances(map_pos, cur_pos, dtype=np.float64):
    """(nmap, ncur) |map - cur|, every operation in `dtype` (float32: the naive run the margin W is measured on)."""
    mp = np.asarray(map_pos, np.float32).reshape(-1, 3).astype(dtype)
    cp = np.asarray(cur_pos, np.float32).reshape(-1, 3).astype(dtype)
    d = mp[:, None, :] - cp[None, :, :]
    s = (d * d).sum(axis=2, dtype=dtype)
    assert s.dtype == dtype
    return np.sqrt(s)


def value_binary(a, b, mutation=None):
    """(n,) popcount of the saturating a - b per byte, as float64; a, b (n, 32) uint8."""
    a, b = np.asarray(a, np.uint8).astype(np.int16), np.asarray(b, np.uint8).astype(np.int16)
    if mutation == "xor":
        d = a ^ b
    elif mutation == "cur_minus_map":
        d = np.maximum(b - a, 0)
    else:
        d = np.maximum(a - b, 0)
    return np.unpackbits(d.astype(np.uint8), axis=1).sum(axis=1).astype(np.float64)


def value_float(a, b, mutation=None):
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)
    s = (d * d).sum(axis=1)
    return s if mutation == "no_sqrt" else np.sqrt(s)


def _emit(v, best, ratio, mutation):
    if mutation == "strict_ratio":
        return ratio * v < best
    if mutation == "ratio_on_best":
        return v <= ratio * best
    return ratio * v <= best


def _feature(v, ratio, is_float, mutation):
    """One feature's candidates' values -> (emit mask, ambiguous)."""
    best, best_at = v[0], 0                             # the first candidate whatever its value
    if mutation != "first_best":
        for k in range(1, len(v)):
            if v[k] < best:
                best, best_at = v[k], k
    if mutation == "best_only":
        keep = np.zeros(len(v), bool)
        keep[best_at] = True
    else:
        keep = _emit(v, best, ratio, mutation)
    ambiguous = False
    if is_float and best > 0:
        ambiguous = bool((np.abs(ratio * v - best) <= RATIO_BAND * best).any())
        if not ambiguous and len(v) > 1:
            second = np.partition(v, 1)[1]
            if second - best <= RATIO_BAND * best:
                ambiguous = bool((_emit(v, second, ratio, mutation) != keep).any())
    return keep, ambiguous


class Answer:
    """The model's answer for one (map view, frame, radius, ratio).
    exact      {j: (trainIdx (n,) int64, value (n,) float64)} for every feature that is not ambiguous and emits something
    ambiguous  {j: outer candidate set (int64 array)}
    with_candidates   how many features have a non-empty outer candidate set
    candidates (nmap,) the certain candidates per feature (the directed scenes are built from these counts)"""

    def __init__(self, nmap, is_float):
        self.nmap, self.is_float = nmap, is_float
        self.exact, self.ambiguous = {}, {}
        self.with_candidates = 0
        self.candidates = np.zeros(nmap, np.int64)
        self.sphere_ambiguous = self.ratio_ambiguous = 0

    def pairs(self):
        """[(j, i)] of the exact features, in the order of emission."""
        return [(j, int(i)) for j in sorted(self.exact) for i in self.exact[j][0]]


def match_xyz(map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, radius, ratio, mutation=None):
    """The model.  Descriptors (n, 32) uint8 (binary rule) or (n, D) float32 (float rule)."""
    assert mutation is None or mutation in MUTATIONS
    map_desc, cur_desc = np.asarray(map_desc), np.asarray(cur_desc)
    is_float = map_desc.dtype != np.uint8
    nmap, ncur = len(map_pos), len(cur_pos)
    ans = Answer(nmap, is_float)
    if nmap == 0 or ncur == 0:
        return ans
    radius, ratio = float(radius), float(ratio)
    d = distances(map_pos, cur_pos)
    ml, cl = np.asarray(map_level, np.int64)[:, None], np.asarray(cur_level, np.int64)[None, :]
    win = {"window0": 0, "window2": 2}.get(mutation, 1)
    level_ok = (cl - win <= ml) & (ml <= cl + win)
    inside = (d < radius * (1 - W)) & level_ok
    outer = (d < radius * (1 + W)) & level_ok
    ans.candidates = inside.sum(axis=1)
    unsure = (inside != outer).any(axis=1)
    jj, ii = np.nonzero(outer)
    if len(jj) == 0:
        return ans
    val = (value_float if is_float else value_binary)(map_desc[jj], cur_desc[ii], mutation)
    starts = np.flatnonzero(np.r_[True, jj[1:] != jj[:-1]])
    ends = np.r_[starts[1:], len(jj)]
    ans.with_candidates = len(starts)
    for lo, hi in zip(starts, ends):
        j = int(jj[lo])
        if unsure[j]:
            ans.ambiguous[j] = ii[lo:hi].copy()
            ans.sphere_ambiguous += 1
            continue
        keep, amb = _feature(val[lo:hi], ratio, is_float, mutation)
        if amb:
            ans.ambiguous[j] = ii[lo:hi].copy()
            ans.ratio_ambiguous += 1
        elif keep.any():
            ans.exact[j] = (ii[lo:hi][keep], val[lo:hi][keep])
    return ans


# ------------------------------------------------------------------------------------------------ the shared check
class Report:
    def __init__(self):
        self.flipped = []           # non-ambiguous features whose emitted (trainIdx) list differs from the model's
        self.order_ok = True        # rows come feature by feature in ascending j
        self.img_bad = 0            # rows of non-ambiguous features with imgIdx != -1
        self.dist_bad = 0           # rows of agreeing features whose distance misses the model's value
        self.worst_u = 0.0          # worst |distance / value - 1| / u of the float rows compared
        self.outside = 0            # rows of ambiguous features with a trainIdx outside the outer set
        self.ambiguous = self.with_candidates = 0

    def failures(self):
        f = []
        if self.flipped:
            f.append("%d features differ from the model, first %s" % (len(self.flipped), self.flipped[:5]))
        if not self.order_ok:
            f.append("rows not in ascending queryIdx")
        if self.img_bad:
            f.append("%d rows with imgIdx != -1" % self.img_bad)
        if self.dist_bad:
            f.append("%d distances off (worst %.2f u)" % (self.dist_bad, self.worst_u))
        if self.outside:
            f.append("%d rows of ambiguous features outside their candidate sets" % self.outside)
        if self.ambiguous > AMBIGUOUS_CAP * self.with_candidates:
            f.append("%d of %d features with candidates ambiguous: above the cap" % (self.ambiguous, self.with_candidates))
        return f


def compare(matches, ans):
    """A match list (a structured array with queryIdx, trainIdx, imgIdx, distance) of any implementation against an Answer."""
    r = Report()
    r.ambiguous, r.with_candidates = len(ans.ambiguous), ans.with_candidates
    q = np.asarray(matches["queryIdx"], np.int64)
    t = np.asarray(matches["trainIdx"], np.int64)
    img = np.asarray(matches["imgIdx"], np.int64)
    dist = np.asarray(matches["distance"])
    r.order_ok = bool((np.diff(q) >= 0).all())
    got = {}
    for k in np.argsort(q, kind="stable"):
        got.setdefault(int(q[k]), []).append(int(k))
    for j, rows in got.items():
        rows = np.array(rows)
        if j in ans.ambiguous:
            r.outside += int((~np.isin(t[rows], ans.ambiguous[j])).sum())
            continue
        r.img_bad += int((img[rows] != -1).sum())
        if j not in ans.exact or t[rows].tolist() != ans.exact[j][0].tolist():
            r.flipped.append(j)
            continue
        v = ans.exact[j][1]
        if ans.is_float:
            assert dist.dtype == np.float32
            with np.errstate(all="ignore"):
                rel = np.where(v > 0, np.abs(dist[rows].astype(np.float64) / v - 1), np.abs(dist[rows].astype(np.float64)))
            r.worst_u = max(r.worst_u, float(rel.max()) / U)
            r.dist_bad += int((rel > DIST_TOL).sum())
        else:
            r.dist_bad += int((dist[rows].astype(np.float64) != v).sum())
    r.flipped += [j for j in ans.exact if j not in got]
    r.flipped.sort()
    return r


def check(matches, ans, what=""):
    """Asserts compare()'s report clean, the cap on ambiguous features included; returns the report."""
    r = compare(matches, ans)
    f = r.failures()
    assert not f, (what, f)
    return r


# ------------------------------------------------------------------------------------------------ scenes
def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def noisy_unit_rows(rng, prev, src):
    y = prev[src].astype(np.float64) + 0.5 / np.sqrt(prev.shape[1]) * rng.standard_normal((len(src), prev.shape[1]))
    return (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)


def _makers(kind):
    """(fresh(rng, n), linked(rng, rows, src)) of a descriptor kind: "binary" (a linked row has 5 % of its bits flipped), a width D
    (unit rows; linked: + N(0, 0.25 / D) per element, renormalised), or such a pair of functions for rows made elsewhere."""
    if isinstance(kind, str):
        assert kind == "binary"
        return (lambda g, n: g.integers(0, 256, (n, 32), dtype=np.uint8),
                lambda g, rows, src: rows[src] ^ np.packbits(g.random((len(src), 256)) < 0.05, axis=1))
    if isinstance(kind, (int, np.integer)):
        return (lambda g, n: unit_rows(g, n, int(kind))), noisy_unit_rows
    return kind


def frame(rng, n, kind="binary"):
    """(pos, desc, level) of n keypoints: uniform(-1.5, 1.5) + (0, 0, 2.5), predicted levels of random octaves and detection
    distances."""
    cp = (rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 2.5]).astype(np.float32)
    norm = np.linalg.norm(cp.astype(np.float64), axis=1)
    cl, _ = predicted_level(rng.integers(0, 8, n), norm * rng.uniform(0.8, 1.25, n), norm)
    return cp, _makers(kind)[0](rng, n), cl.astype(np.int32)


def view(rng, fr, n, kind="binary", sigma=0.05):
    """(pos, desc, level) of n map features at sigma around random keypoints of the frame fr, their rows linked to those
    keypoints', their levels off by -2 ... 2; around nothing (an empty frame): like a frame."""
    cp, cd, cl = fr
    if len(cp) == 0 or n == 0:
        mp, md, _ = frame(rng, n, kind)
        return mp, md, rng.integers(0, 8, n).astype(np.int32)
    src = rng.integers(0, len(cp), n)
    mp = (cp[src] + rng.normal(0, sigma, (n, 3))).astype(np.float32)
    ml = np.clip(cl[src] + rng.integers(-2, 3, n), 0, 7).astype(np.int32)
    return mp, _makers(kind)[1](rng, cd, src), ml


def scene(rng, nmap, ncur, kind="binary", sigma=0.05):
    """One frame and one view of it: dict(map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level)."""
    fr = frame(rng, ncur, kind)
    mp, md, ml = view(rng, fr, nmap, kind, sigma)
    return dict(map_pos=mp, map_desc=md, map_level=ml, cur_pos=fr[0], cur_desc=fr[1], cur_level=fr[2])


def _pad(items, cap):
    pos = np.zeros((len(items), cap, 3), np.float32)
    desc = np.zeros((len(items), cap) + items[0][1].shape[1:], items[0][1].dtype)
    level = np.zeros((len(items), cap), np.int32)
    for k, (p, d, l) in enumerate(items):
        pos[k, :len(p)], desc[k, :len(p)], level[k, :len(p)] = p, d, l
    return dict(pos=pos, desc=desc, level=level, nkpts=np.array([len(p) for p, _, _ in items], np.int32), cap=cap)


def sets(rng, view_counts, frame_counts, view_cap, frame_cap, source, kind="binary", sigma=0.05):
    """(views, frames) in the batched layout -- dict(pos (n, cap, 3), desc (n, cap, ...), level (n, cap), nkpts, cap) --: view v
    lies around frame source[v]."""
    frames = [frame(rng, n, kind) for n in frame_counts]
    views = [view(rng, frames[source[v]], n, kind, sigma) for v, n in enumerate(view_counts)]
    return _pad(views, view_cap), _pad(frames, frame_cap)


def side(s, i):
    n = int(s["nkpts"][i])
    return s["pos"][i, :n], s["desc"][i, :n], s["level"][i, :n]


def args(s):
    return s["map_pos"], s["map_desc"], s["map_level"], s["cur_pos"], s["cur_desc"], s["cur_level"]


def _rows_like(rng, kind, n):
    return _makers(kind)[0](rng, n)


def _cluster(rng, centre, n, radius):
    """n points at 0.2 ... 0.8 radius around centre."""
    v = rng.standard_normal((n, 3))
    v *= (rng.uniform(0.2, 0.8, n) * radius / np.linalg.norm(v, axis=1))[:, None]
    return (np.asarray(centre, np.float64) + v).astype(np.float32)


def scene_stash(rng, kind="binary", radius=RADIUS):
    """Three features, 5 m apart, with exactly 15, 16 and 17 candidates (asserted from the model's counts) and twelve keypoints
    each that fail on the level or on the sphere."""
    counts = (15, 16, 17)
    mp = np.array([[-5, 0, 3], [0, 0, 3], [5, 0, 3]], np.float32)
    cp, cl = [], []
    for c, n in zip(mp, counts):
        cp += [_cluster(rng, c, n, radius), _cluster(rng, c, 6, radius), _cluster(rng, c, 6, radius) + np.float32(2 * radius)]
        cl += [rng.integers(2, 5, n), np.r_[[0, 1, 5, 6, 7], [0]], rng.integers(2, 5, 6)]
    cp, cl = np.concatenate(cp), np.concatenate(cl)
    order = rng.permutation(len(cp))
    cp, cl = cp[order], cl[order]
    s = dict(map_pos=mp, map_level=np.full(3, 3, np.int32), cur_pos=cp, cur_level=cl.astype(np.int32),
             map_desc=_rows_like(rng, kind, 3), cur_desc=_rows_like(rng, kind, len(cp)))
    assert match_xyz(*args(s), radius, 0.55).candidates.tolist() == list(counts)
    return s


def scene_tile(rng, kind="binary", radius=RADIUS):
    """1025 keypoints; feature 1's only candidates are keypoints 1023 and 1024 (an LDS tile holds 1024), features 0 and 2 lie in
    the crowd."""
    s = scene(rng, 3, 1025, kind)
    far = np.array([10, 10, 10], np.float32)
    s["map_pos"][1] = far
    s["cur_pos"][1023:] = _cluster(rng, far, 2, radius)
    s["cur_level"][1023:] = s["map_level"][1] = 4
    a = match_xyz(*args(s), radius, 0.55)
    assert a.candidates[1] == 2 and set(a.exact[1][0].tolist()) <= {1023, 1024} and not a.ambiguous
    return s


def scene_ratio_equal(rng):
    """Binary: one feature whose candidates have the values 8, 16 and 17, for ratio 0.5: 0.5 x 16 == 8 exactly (emitted), 0.5 x 17
    is not."""
    md = np.zeros((1, 32), np.uint8)
    md[0, :3] = 0xFF
    cd = np.zeros((3, 32), np.uint8)
    cd[0, :3] = [0xFF, 0x00, 0xFF]        # 8
    cd[1, :3] = [0x00, 0x00, 0xFF]        # 16
    cd[2, :3] = [0x00, 0x00, 0xFE]        # 17
    cd[:, 3:] = rng.integers(0, 256, (3, 29), dtype=np.uint8)        # (bits the saturating difference never sees: map is 0 there)
    pos = np.array([[0.1, 0.2, 2.0]], np.float32)
    s = dict(map_pos=pos, map_desc=md, map_level=np.array([3], np.int32), cur_pos=np.repeat(pos, 3, 0), cur_desc=cd,
             cur_level=np.array([3, 2, 4], np.int32))
    a = match_xyz(*args(s), RADIUS, 0.5)
    assert a.exact[0][0].tolist() == [0, 1] and a.exact[0][1].tolist() == [8.0, 16.0]
    return s


def scene_first_not_least(rng, kind="binary"):
    """One feature, three candidates; the first is not the least: binary values 20, 4, 30 (ratio 0.55 emits the second only; with
    the first taken as best all three), float rows with the feature's row a noisy copy of the second candidate's."""
    pos = np.array([[0.3, -0.2, 1.5]], np.float32)
    if kind == "binary":
        md = np.zeros((1, 32), np.uint8)
        md[0, :4] = 0xFF
        cd = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        cd[0, :4] = [0x00, 0x00, 0x0F, 0xFF]      # 8 + 8 + 4 + 0
        cd[1, :4] = [0xFF, 0xFF, 0xFF, 0x0F]      # 4
        cd[2, :4] = [0x00, 0x00, 0x00, 0x03]      # 8 + 8 + 8 + 6
    else:
        fresh, linked = _makers(kind)
        cd = fresh(rng, 3)
        md = linked(rng, cd, np.array([1]))
    s = dict(map_pos=pos, map_desc=md, map_level=np.array([5], np.int32), cur_pos=_cluster(rng, pos[0], 3, RADIUS), cur_desc=cd,
             cur_level=np.array([5, 4, 6], np.int32))
    a = match_xyz(*args(s), RADIUS, RATIO)
    assert a.exact[0][0].tolist() == [1]
    if kind == "binary":
        assert match_xyz(*args(s), RADIUS, 0.1).exact[0][1].tolist() == [20.0, 4.0, 30.0]
    return s


def directed(rng, kind="binary"):
    """[(name, scene, radius, ratio)]: the directed scenes of one descriptor kind."""
    out = [("stash", scene_stash(rng, kind), RADIUS, RATIO), ("stash, ratio 0.1", scene_stash(rng, kind), RADIUS, 0.1),
           ("tile", scene_tile(rng, kind), RADIUS, RATIO), ("first not least", scene_first_not_least(rng, kind), RADIUS, RATIO)]
    if kind == "binary":
        out.append(("ratio x value == best", scene_ratio_equal(rng), RADIUS, 0.5))
    return out


# ------------------------------------------------------------------------------------------------ measurements
def norm32_margin(scenes):
    """The largest |d32 / d64 - 1| of the model's own float32 norm over (nmap, ncur) scenes, and how many (feature, keypoint)
    pairs lie within W of any of the ten ladder radii."""
    worst, near, pairs = 0.0, 0, 0
    radii = [ladder(RADIUS, RATIO, k)[0] for k in range(1, 11)]
    for n, (nmap, ncur) in enumerate(scenes):
        s = scene(np.random.default_rng(1000 + n), nmap, ncur)
        d64 = distances(s["map_pos"], s["cur_pos"])
        d32 = distances(s["map_pos"], s["cur_pos"], np.float32)
        ok = d64 > 0
        worst = max(worst, float(np.abs(d32[ok].astype(np.float64) / d64[ok] - 1).max()))
        near += sum(int(((d64 >= r * (1 - W)) & (d64 < r * (1 + W))).sum()) for r in radii)
        pairs += d64.size
    return worst, near, pairs


if __name__ == "__main__":
    worst, near, pairs = norm32_margin(SCENES)
    print("largest |d32 / d64 - 1| over %d pairs: %.3e (bound %.1e); within W of a ladder radius: %d" % (pairs, worst, NORM32_BOUND, near))
    for kind in ("binary", 20, 64, 128):
        for n, (nmap, ncur) in enumerate(SCENES):
            s = scene(np.random.default_rng(2000 + n), nmap, ncur, kind)
            for k in TRIES:
                a = match_xyz(*args(s), *ladder(RADIUS, RATIO, k))
                print("%-6s %4d x %4d try %2d: %5d features with candidates, %d sphere-ambiguous, %d ratio-ambiguous"
                      % (kind, nmap, ncur, k, a.with_candidates, a.sphere_ambiguous, a.ratio_ambiguous))
