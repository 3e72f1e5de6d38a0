"""RANSAC scoring, selection and refit restated in plain float64 numpy (no GPU, nothing from oracle/), plus the inputs and
the checks that tests/test_ransac_model_host.py (oracle against this model) and tests/test_gpu_ransac_model.py (kernels
against this model) share.

Written from the reference's src/TransformEst/RANSAC.cpp and RGBD::point3Dto2D (src/RGBD/RGBD.cpp:92-98), not from
oracle/putslam_oracle.c, and independent of it: it calls nothing in oracle/, uses numpy's LAPACK SVD and inverse where the
oracle and the kernels repeat Eigen's Jacobi SVD and cofactor inverse, and works in float64 where they work in float32.
What it shares with them is DESIGN.md section 2's sample rule (an input of the build, not of the reference).

  depth filter (RANSAC.cpp:65-74)   a match goes when either point has a NaN, z < 0.1 or z > 6; 0.1 and 6.0 stay
  sample of hypothesis h            explicit raw draws: index = draw % M, a repeat moves on to the next free index;
                                    seeded stream: draw(seed, h, j) = splitmix64(seed ^ splitmix64(h << 8 | j)) >> 33,
                                    index = draw % M, a repeat is drawn again
  3-point model / refit (:207-244)  Eigen::umeyama(cur, prev, false): SVD of the cross covariance, last column of U flipped
                                    when det(U) det(V) < 0
  errors under (R, t) (:251-436)    old = R cur + t, new = R^-1 (prev - t), e = |old - prev|,
                                    r0 = |proj(new) - proj(cur)|, r1 = |proj(old) - proj(prev)|,
                                    proj: u = x fx / z + cx, v = y fy / z + cy, no test on z
  decision                          0: e < thrE; 4: e < thrE prev.z; 1: r0 < thrR and r1 < thrR; 2: all three;
                                    Mahalanobis (3, dead in the reference: cov is never filled) and unknown modes count 0
  selection (:438-455)              the first hypothesis with the strictly largest count among the iterations run
  refit + re-selection (:152-158)   Umeyama over that hypothesis's loop inliers, then the Euclidean test (adaptive for
                                    mode 4: computeMatchInlierRatioEuclidean reads the error version) over those inliers
  gate (:77-80, :161-164)           M < minimalNumberOfMatches, or float32(count) / float32(M) below the minimal ratio:
                                    identity and no inliers

A float32 implementation cannot be compared with this decision for decision: a match whose error lies within rounding of
its threshold may fall on either side.  count_bracket(w) therefore gives, per hypothesis, the counts with every threshold
scaled by (1 - w) and by (1 + w); an implementation of the same formulas must land inside, one of other formulas does not
(MUTATIONS below are such other formulas, so that the tests can show that they would notice).  A hypothesis whose sample is
nearly collinear (second singular value of its covariance below 1e-3 of the first, or below 1e-4 m^2) has a rotation that
float32 does not determine; it is set aside, and the tests cap how many may be.

MEASURED MARGINS (python tests/ransac_model_f64.py prints both; CPU only)

  w    The model run with dtype=float32 (the same lines of code: a naive float32 implementation that owes nothing to the
       project) against its own float64 brackets, over every run of RUNS (3 classes x 4 modes x 400 hypotheses, the scaled
       camera, the halved thresholds and the small match counts), well-conditioned hypotheses only: the smallest w on a
       1.25-step grid at which every float32 count lies inside is
           4.81e-05
       All runs but one need no margin at all on that grid (1e-8: no float32 decision of theirs differs); the one is the
       halved thresholds in mode 4, hypothesis 100, whose sample has sigma_2 = 1.4e-3 sigma_1 -- just inside the
       conditioning rule -- and moves one error by 1.6e-6 m next to a threshold of 0.0214 m.  W = 4 x that, rounded up to
       a power of ten: 1e-3.  The factor 4 covers the kernels summing and inverting in another order than numpy.
  umeyama   see UMEYAMA_BOUNDS: numpy's float32 SVD fit against the long-double fit, 200 seeds per family and k.
"""
import numpy as np

EUCLIDEAN, REPROJECTION, BOTH, MAHALANOBIS, ADAPTIVE = 0, 1, 2, 3, 4
MODES = (EUCLIDEAN, REPROJECTION, BOTH, ADAPTIVE)
MUTATIONS = ("adaptive_cur_z", "one_direction", "real_new_from_prev", "no_inverse", "fx_for_v", "refit_reprojection",
             "last_max")

W = 1e-3                  # 4 x the measured 4.81e-05, rounded up to a power of ten (module docstring)
SIGMA_REL, SIGMA_ABS = 1e-3, 1e-4      # the conditioning rule
COND_CAP = 0.02           # share of a run's hypotheses that may be set aside
REFIT_TOL = 1e-5          # tests/test_oracle_kat.py::test_umeyama_vs_float64's figure for k >= 8
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ pieces
def depth_filter(prev, cur, q, t):
    """Indices (into the match list) of the matches that survive RANSAC.cpp:65-74, in their order."""
    p, c = np.asarray(prev, np.float64)[q], np.asarray(cur, np.float64)[t]
    bad = np.isnan(p).any(1) | np.isnan(c).any(1) | (p[:, 2] < 0.1) | (p[:, 2] > 6) | (c[:, 2] < 0.1) | (c[:, 2] > 6)
    return np.flatnonzero(~bad)


def sample_explicit(raw, M):
    """(H, 3) match indices from (H, 3) raw draws: draw % M, a repeat moves on to the next free index."""
    raw = np.asarray(raw, np.int64)
    idx = np.zeros(raw.shape, np.int64)
    for j in range(3):
        v = raw[:, j] % M
        for _ in range(j):
            v = np.where((idx[:, :j] == v[:, None]).any(1), (v + 1) % M, v)
        idx[:, j] = v
    return idx


def _splitmix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw31(seed, h, j):
    """The seeded stream's draw j of hypothesis h (arrays allowed)."""
    key = (np.asarray(h, np.uint64) << np.uint64(8)) | np.asarray(j, np.uint64)
    return _splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _splitmix64(key)) >> np.uint64(33)


def sample_seeded(seed, H, M):
    """(H, 3) match indices of the seeded stream: draw % M, a repeat is drawn again (the batched calls' stream)."""
    idx = np.zeros((H, 3), np.int64)
    d = (draw31(seed, np.arange(H)[:, None], np.arange(16)[None, :]) % np.uint64(M)).astype(np.int64)
    for h in range(H):
        got, j = [], 0
        while len(got) < 3:
            v = int(d[h, j]) if j < 16 else int(draw31(seed, h, j) % np.uint64(M))
            if v not in got:
                got.append(v)
            j += 1
        idx[h] = got
    return idx


def umeyama(src, dst, dtype=np.float64):
    """Eigen::umeyama(src, dst, false) over the last two axes (..., k, 3): R (..., 3, 3), t (..., 3) with dst ~ R src + t,
    and the singular values of the cross covariance."""
    src, dst = np.asarray(src, dtype), np.asarray(dst, dtype)
    ms, md = src.mean(-2, keepdims=True), dst.mean(-2, keepdims=True)
    cov = np.swapaxes(dst - md, -1, -2) @ (src - ms) / dtype(src.shape[-2])
    U, s, Vt = np.linalg.svd(cov)
    flip = np.linalg.det(U) * np.linalg.det(Vt) < 0
    S = np.ones(s.shape, dtype)
    S[..., 2] = np.where(flip, -1, 1)
    R = (U * S[..., None, :]) @ Vt
    t = md[..., 0, :] - (R @ ms[..., 0, :, None])[..., 0]
    return R, t, s


def umeyama_long(src, dst):
    """The refit's reference: means and covariance summed in long double, the 3 x 3 SVD in float64 (numpy has no wider
    one; its 1e-16 is five orders below anything asserted).  4 x 4 float64, dst ~ T src."""
    s, d = np.asarray(src, np.longdouble), np.asarray(dst, np.longdouble)
    ms, md = s.mean(0), d.mean(0)
    cov = ((d - md).T @ (s - ms) / np.longdouble(len(s))).astype(np.float64)
    U, sv, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = (md - T[:3, :3].astype(np.longdouble) @ ms).astype(np.float64)
    return T


def project(p, K, mutation=None):
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    if mutation == "fx_for_v":
        fy = fx
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([p[..., 0] * fx / p[..., 2] + cx, p[..., 1] * fy / p[..., 2] + cy], -1)


def errors(R, t, P, C, K, mutation=None):
    """e, r0, r1 of every match (P, C: (M, 3) previous / current points) under every pose (R (H, 3, 3), t (H, 3)): (H, M)."""
    old = np.einsum("hij,mj->hmi", R, C) + t[:, None, :]
    if mutation == "no_inverse":
        new = np.einsum("hij,mj->hmi", R, P) + t[:, None, :]
    else:
        new = np.einsum("hij,hmj->hmi", np.linalg.inv(R), P[None] - t[:, None, :])
    with np.errstate(invalid="ignore"):
        e = np.linalg.norm(old - P[None], axis=-1)
        real_new = project(P if mutation == "real_new_from_prev" else C, K, mutation)
        r0 = np.linalg.norm(project(new, K, mutation) - real_new[None], axis=-1)
        r1 = np.linalg.norm(project(old, K, mutation) - project(P, K, mutation)[None], axis=-1)
    return e, r0, r1


def decide(mode, e, r0, r1, pz, cz, thrE, thrR, mutation=None):
    """Inlier flags (H, M).  NaN errors compare false, as in the reference."""
    dt = e.dtype.type
    thrE, thrR = dt(thrE), dt(thrR)
    with np.errstate(invalid="ignore"):
        if mode == EUCLIDEAN:
            return e < thrE
        if mode == ADAPTIVE:
            return e < thrE * (cz if mutation == "adaptive_cur_z" else pz)[None]
        rep = (r1 < thrR) if mutation == "one_direction" else (r0 < thrR) & (r1 < thrR)
        if mode == REPROJECTION:
            return rep
        if mode == BOTH:
            return (e < thrE) & rep
    return np.zeros(e.shape, bool)


# ------------------------------------------------------------------------------------------------ the model of one call
class Model:
    """One estimateTransformation call.  prev / cur (n, 3), q / t: the match list's queryIdx / trainIdx, K: 9 floats row-major.
    Samples: raw (H, 3) explicit draws, or seed + H for the seeded stream."""

    def __init__(self, prev, cur, q, t, K, mode, thrE=0.04, thrR=2.0, raw=None, seed=None, H=None, min_matches=15,
                 min_ratio=0.2, mutation=None, dtype=np.float64):
        assert mutation is None or mutation in MUTATIONS
        self.mode, self.thrE, self.thrR, self.mutation, self.dtype = mode, thrE, thrR, mutation, dtype
        self.min_matches, self.min_ratio = min_matches, min_ratio
        self.m = len(q)
        self.kept = depth_filter(prev, cur, q, t)
        self.M = len(self.kept)
        self.P = np.asarray(prev, np.float64)[np.asarray(q)[self.kept]].astype(dtype)
        self.C = np.asarray(cur, np.float64)[np.asarray(t)[self.kept]].astype(dtype)
        self.K = np.asarray(K, np.float64).astype(dtype)
        self.H = len(raw) if raw is not None else H
        if self.M >= 3:
            self.idx = sample_explicit(raw, self.M) if raw is not None else sample_seeded(seed, H, self.M)
            self.R, self.t, self.sv = umeyama(self.C[self.idx], self.P[self.idx], dtype)
            self.valid = ~np.isnan(self.R[:, 0, 0])                        # RANSAC.cpp:239
            self.e, self.r0, self.r1 = errors(self.R, self.t, self.P, self.C, self.K, mutation)
        else:
            self.idx = np.zeros((self.H, 3), np.int64)
            self.valid = np.zeros(self.H, bool)
            self.sv = np.zeros((self.H, 3))
            self.e = self.r0 = self.r1 = np.zeros((self.H, 0), dtype)

    def well_conditioned(self):
        s = np.asarray(self.sv, np.float64)
        return ~((s[:, 1] < SIGMA_REL * s[:, 0]) | (s[:, 1] < SIGMA_ABS))

    def flags(self, scale=1.0):
        f = decide(self.mode, self.e, self.r0, self.r1, self.P[:, 2], self.C[:, 2], self.thrE * scale, self.thrR * scale,
                   self.mutation)
        return f & self.valid[:, None]

    def counts(self, scale=1.0):
        return self.flags(scale).sum(1)

    def count_bracket(self, h=None, w=W):
        """(lo, hi): the counts with both thresholds scaled by (1 - w) and by (1 + w); arrays over all hypotheses when h is None."""
        lo, hi = self.counts(1.0 - w), self.counts(1.0 + w)
        return (lo, hi) if h is None else (int(lo[h]), int(hi[h]))

    def select(self, iterations):
        """The first hypothesis with the strictly largest count among the iterations run (-1: none scored above 0)."""
        c = self.counts()[:iterations]
        if len(c) == 0 or c.max() == 0:
            return -1
        return int(len(c) - 1 - np.argmax(c[::-1])) if self.mutation == "last_max" else int(np.argmax(c))

    def final_flags(self, T, members, scale=1.0, slack=0.0):
        """Re-selection (RANSAC.cpp:156) among `members` (flags over the M kept matches) under the 4 x 4 pose T: Euclidean,
        adaptive for mode 4 -- whatever the loop's metric was.  The threshold is scaled by `scale` and moved by `slack` metres."""
        T = np.asarray(T, np.float64)
        P, C = self.P.astype(np.float64), self.C.astype(np.float64)
        if self.mutation == "refit_reprojection":
            e, r0, r1 = errors(T[None, :3, :3], T[None, :3, 3], P, C, self.K.astype(np.float64))
            f = decide(self.mode, e, r0, r1, P[:, 2], C[:, 2], self.thrE * scale + slack, self.thrR * scale, None)[0]
        else:
            e = np.linalg.norm(C @ T[:3, :3].T + T[:3, 3] - P, axis=1)
            thr = self.thrE * scale * (P[:, 2] if self.mode == ADAPTIVE else 1.0) + slack
            f = e < thr
        return f & members

    def ratio(self, count):
        return np.float32(count) / np.float32(self.M)

    def run(self, iterations):
        """The model's own answer for `iterations` trips of the loop: dict(best, count, ratio, accepted, pose, mask (over the
        m matches of the list), numInliers)."""
        out = dict(best=-1, count=0, ratio=np.float32(0), accepted=0, pose=np.eye(4), mask=np.zeros(self.m, bool), numInliers=0)
        if self.M < self.min_matches or self.M < 3:
            return out
        b = self.select(iterations)
        if b < 0:
            return out
        members = self.flags()[b]
        out.update(best=b, count=int(members.sum()), ratio=self.ratio(members.sum()))
        if float(out["ratio"]) < self.min_ratio:
            return out
        T = umeyama_long(self.C[members], self.P[members])
        fin = self.final_flags(T, members)
        out["mask"][self.kept[fin]] = True
        out.update(accepted=1, pose=T, numInliers=int(fin.sum()))
        return out


# ------------------------------------------------------------------------------------------------ the shared checks
def check_counts(model, counts, M, w=W):
    """Violations (strings) of `counts` (every hypothesis scored, 0 for an invalid model) against the model's brackets, and the
    number of hypotheses set aside for their sample's conditioning."""
    bad = []
    if M != model.M:
        return ["M %d, model %d" % (M, model.M)], 0
    if model.M < 3:
        return ["count %d at M < 3" % c for c in counts if c != 0], 0
    lo, hi = model.count_bracket(None, w)
    ok = model.well_conditioned()
    c = np.asarray(counts)
    for h in np.flatnonzero(ok & ((c < lo) | (c > hi))):
        bad.append("hypothesis %d: count %d outside [%d, %d]" % (h, c[h], lo[h], hi[h]))
    return bad, int((~ok).sum())


def check_end_to_end(model, res, fixed, w=W):
    """Violations of one whole call's results against the model.  res: pose (4 x 4, float32), mask (over the m matches),
    stats (numMatchesIn, numMatchesValid, bestHypothesis, bestInlierCount, iterationsRun, numInliers, accepted,
    bestInlierRatio).  fixed: the fixed schedule (every hypothesis is run).  Returns (violations, selection_only):
    selection_only says that the best hypothesis's bracket was not empty, so that its inlier set -- and with it refit, mask
    and numInliers -- is not determined by the model; such a case is checked up to the selection."""
    st, bad = res["stats"], []
    pose, mask = np.asarray(res["pose"], np.float64), np.asarray(res["mask"]).astype(bool)

    def want(name, got, exp):
        if got != exp:
            bad.append("%s %r, model %r" % (name, got, exp))

    def rejected():
        want("accepted", int(st["accepted"]), 0)
        want("numInliers", int(st["numInliers"]), 0)
        want("mask.sum", int(mask.sum()), 0)
        if not np.array_equal(pose, np.eye(4)):
            bad.append("pose of a rejected call is not the identity")

    want("numMatchesIn", int(st["numMatchesIn"]), model.m)
    want("numMatchesValid", int(st["numMatchesValid"]), model.M)
    if model.M < model.min_matches or model.M < 3:                       # RANSAC.cpp:77-80
        want("iterationsRun", int(st["iterationsRun"]), 0)
        want("bestHypothesis", int(st["bestHypothesis"]), -1)
        rejected()
        return bad, False
    its, b, cnt = int(st["iterationsRun"]), int(st["bestHypothesis"]), int(st["bestInlierCount"])
    if not (1 <= its <= model.H) or (fixed and its != model.H):
        return bad + ["iterationsRun %d of %d" % (its, model.H)], False
    if not 0 <= b < its:
        return bad + ["bestHypothesis %d with %d iterations" % (b, its)], False
    lo, hi = model.count_bracket(None, w)
    ok = model.well_conditioned()
    if not ok[b]:
        return bad, True
    if not lo[b] <= cnt <= hi[b]:
        bad.append("best hypothesis %d: count %d outside [%d, %d]" % (b, cnt, lo[b], hi[b]))
    h = np.arange(its)
    first = model.mutation != "last_max"
    beaten = np.where((h < b) == first, lo[:its] >= cnt, lo[:its] > cnt) & ok[:its] & (h != b)
    for k in np.flatnonzero(beaten):
        bad.append("hypothesis %d has at least %d inliers, the reported best %d has %d" % (k, lo[k], b, cnt))
    want("bestInlierRatio", np.float32(st["bestInlierRatio"]), model.ratio(cnt))
    accepted = not float(model.ratio(cnt)) < model.min_ratio              # RANSAC.cpp:161
    if not accepted:
        rejected()
        return bad, False
    want("accepted", int(st["accepted"]), 1)
    want("numInliers", int(st["numInliers"]), int(mask.sum()))
    if lo[b] != hi[b]:
        return bad, True
    members = model.flags()[b]
    T = umeyama_long(model.C[members], model.P[members])
    diff = float(np.abs(pose - T).max())
    if not diff < REFIT_TOL:
        bad.append("refit pose %.3g from the long-double fit over the model's %d inliers" % (diff, members.sum()))
        return bad, False
    got = mask[model.kept]
    if mask.sum() != got.sum():
        bad.append("mask set on a match that the depth filter removed")
    certain, possible = model.final_flags(pose, members, 1.0 - w), model.final_flags(pose, members, 1.0 + w)
    if (certain & ~got).any() or (got & ~possible).any():
        bad.append("final mask: %d certain inliers missing, %d impossible ones set" % ((certain & ~got).sum(), (got & ~possible).sum()))
    # numInliers against the model's own refit pose: a pose difference of `diff` per entry moves an error by
    # diff (|x| + |y| + |z| + 1) at the most
    slack = diff * float((np.abs(model.C).sum(1) + 1.0).max())
    nlo, nhi = model.final_flags(T, members, 1.0 - w, -slack).sum(), model.final_flags(T, members, 1.0 + w, slack).sum()
    if not nlo <= int(st["numInliers"]) <= nhi:
        bad.append("numInliers %d, model [%d, %d]" % (st["numInliers"], nlo, nhi))
    return bad, False


# ------------------------------------------------------------------------------------------------ inputs
K_SKEW = np.array([525.0, 0.0, 331.0, 0.0, 420.0, 247.5, 0.0, 0.0, 1.0], np.float32)      # fy = 0.8 fx, cx != cy
K_SMALL = (K_SKEW * np.float32(0.03)).astype(np.float32)
K_SMALL[8] = 1.0
CLASSES = ((30.0, 0.5, 0.02, 0.6), (5.0, 0.1, 0.004, 0.7), (40.0, 1.0, 0.03, 0.3))    # angle deg, translation m, noise m, true share
N_FULL, H_DRAWS = 257, 400
SMALL_M = (3, 14, 15, 64, 65)


def _points(rng, n):
    z = rng.uniform(0.3, 5.5, n)
    return np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)


def motion(rng, angle_deg, trans):
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    ang = np.deg2rad(angle_deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    d = rng.standard_normal(3)
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx), d / np.linalg.norm(d) * trans


def make_input(cls, n=N_FULL, seed=0):
    """prev, cur (n, 3) float32 and the motion: cur = R^T (prev - t) + noise for a share of the matches, unrelated points for
    the rest; matches are the identity list.  Points whose partner would leave the depth range are drawn again.  n = 257 has
    five previous points moved along their rays to z = 0.05, 6.5, NaN (dropped: M = 254 = three 64-match blocks and a tail of
    62) and 0.1, 6.0 (kept: the filter's edges)."""
    angle, trans, noise, share = cls
    rng = np.random.default_rng([seed, n, int(angle), int(trans * 10)])
    R, t = motion(rng, angle, trans)
    prev = np.zeros((0, 3))
    while len(prev) < n:
        p = _points(rng, 4 * n)
        cz = ((p - t) @ R)[:, 2]
        prev = np.concatenate([prev, p[(cz > 0.3) & (cz < 5.5)]])[:n]
    special = n == N_FULL
    if special:
        for i, z in ((20, 0.05), (70, 6.5), (130, 0.1), (200, 6.0)):
            prev[i] *= z / prev[i, 2]
    cur = (prev - t) @ R + rng.normal(0, noise, (n, 3))
    out = rng.random(n) >= share
    cur[out] = _points(rng, int(out.sum()))
    if special:
        prev[100, 2] = np.nan
        cur[:, 2] = np.clip(cur[:, 2], 0.1, 6.0)      # (the partners of z = 0.1 / 6.0 may leave the range: they meet its edge)
        cur[100] = _points(rng, 1)[0]
    prev, cur = prev.astype(np.float32), cur.astype(np.float32)
    if special:
        prev[130, 2], prev[200, 2] = 0.1, 6.0           # exactly the filter's constants as float32 holds them
    return prev, cur, R, t


def make_draws(seed, H=H_DRAWS):
    raw = np.random.default_rng([77, seed]).integers(0, 2 ** 31, (H, 3)).astype(np.uint32)
    raw[5], raw[11] = (7, 7, 7), (0, 1, 0)          # forced repeats
    return raw


def runs():
    """(name, class index, n, mode, K, thrE, thrR, draw seed) of every committed run."""
    out = []
    for ci in range(len(CLASSES)):
        for mode in MODES:
            out.append(("class%d-mode%d" % (ci, mode), ci, N_FULL, mode, K_SKEW, 0.04, 2.0, ci))
    for mode in (REPROJECTION, BOTH):
        out.append(("smallK-mode%d" % mode, 0, N_FULL, mode, K_SMALL, 0.04, 2.0, 3))
    for mode in MODES:
        out.append(("halved-mode%d" % mode, 1, N_FULL, mode, K_SKEW, 0.02, 1.0, 4))
    for n in SMALL_M:
        for mode in MODES:
            out.append(("M%d-mode%d" % (n, mode), 1, n, mode, K_SKEW, 0.04, 2.0, 10 + n))
    return out


RUNS = runs()
_INPUTS, _MODELS = {}, {}


def run_input(run):
    """prev, cur, q, t (identity match list), raw draws of a run of RUNS (computed once, shared, read-only)."""
    name, ci, n, mode, K, thrE, thrR, ds = run
    key = (ci, n, ds)
    if key not in _INPUTS:
        prev, cur, _, _ = make_input(CLASSES[ci], n)
        raw = make_draws(ds)
        for a in (prev, cur, raw):
            a.setflags(write=False)
        _INPUTS[key] = (prev, cur, np.arange(n), np.arange(n), raw)
    return _INPUTS[key]


def run_model(run, mutation=None, dtype=np.float64, raw=None, min_matches=15, min_ratio=0.2):
    name, ci, n, mode, K, thrE, thrR, ds = run
    prev, cur, q, t, raw0 = run_input(run)
    plain = mutation is None and dtype is np.float64 and raw is None and (min_matches, min_ratio) == (15, 0.2)
    if plain and name in _MODELS:
        return _MODELS[name]
    model = Model(prev, cur, q, t, K, mode, thrE, thrR, raw=raw0 if raw is None else raw, mutation=mutation, dtype=dtype,
                 min_matches=min_matches, min_ratio=min_ratio)
    if plain:
        _MODELS[name] = model         # (a Model is never written to after its construction)
    return model


# ------------------------------------------------------------------------------------------------ the Umeyama refit on its own
FAMILIES = ("good", "far", "planar", "near_planar", "collinear", "thin", "tiny", "huge")
POSE_FAMILIES = ("good", "far", "planar", "near_planar", "tiny", "huge")       # the data determines the rotation
UMEYAMA_K = (3, 4, 64, 65, 1000)


KAPPA_MAX = 20.0      # sets of a POSE_FAMILIES family: sigma_1 <= KAPPA_MAX (sigma_2 + sigma_3) of the cross covariance


def family_points(family, k, rng, sets=1):
    """(sets, k, 3) float32 source and destination sets: dst = R src + t + noise (25 degrees, 0.5 scene units at the most).
    A rotation moves by |E| / (sigma_2 + sigma_3) under a perturbation E of the covariance, so a family whose pose is
    asserted holds no slim set (a random triangle is one now and then, whatever the family): such a set is drawn again."""
    scale = {"tiny": 1e-3, "huge": 1e3}.get(family, 1.0)
    s, d = np.zeros((sets, k, 3)), np.zeros((sets, k, 3))
    for i in range(sets):
        while True:
            p = rng.uniform(-1, 1, (k, 3))
            if family == "planar":
                p[:, 2] = 0
            elif family == "near_planar":
                p[:, 2] *= 1e-3
            elif family == "collinear":
                p[:, 1:] = 0
            elif family == "thin":
                p[:, 1:] *= 1e-4
            p = p * scale + np.array([0, 0, 3 * scale]) + (np.array([40.0, -30.0, 50.0]) if family == "far" else 0)
            R, t = motion(rng, rng.uniform(0, 25), rng.uniform(0, 0.5) * scale)
            s[i], d[i] = p, p @ R.T + t + rng.normal(0, 0.004 * scale, (k, 3))
            sv = umeyama(s[i].astype(np.float32), d[i].astype(np.float32))[2]
            if family not in POSE_FAMILIES or sv[0] <= KAPPA_MAX * (sv[1] + sv[2]):
                break
    return s.astype(np.float32), d.astype(np.float32)


def umeyama_quality(src, dst, T):
    """Of a float32 fit T (4 x 4) of one set against the long-double fit: (|det R - 1|, |R R^T - I| max, excess of the mean
    squared residual over the optimum in units of eps32 sigma_src sigma_dst, pose difference: max entry of the rotation's,
    and of the translation's relative to 1 + the larger centroid norm)."""
    T = np.asarray(T, np.float64)
    s, d = np.asarray(src, np.longdouble), np.asarray(dst, np.longdouble)
    Tl = umeyama_long(src, dst)

    def msr(X):
        return float((((s @ X[:3, :3].astype(np.longdouble).T + X[:3, 3]) - d) ** 2).sum(1).mean())

    ss, sd = float(np.sqrt(((s - s.mean(0)) ** 2).sum(1).mean())), float(np.sqrt(((d - d.mean(0)) ** 2).sum(1).mean()))
    R = T[:3, :3]
    cen = 1.0 + max(float(np.linalg.norm(s.mean(0).astype(np.float64))), float(np.linalg.norm(d.mean(0).astype(np.float64))))
    pose = max(float(np.abs(R - Tl[:3, :3]).max()), float(np.abs(T[:3, 3] - Tl[:3, 3]).max()) / cen)
    return (abs(np.linalg.det(R) - 1.0), float(np.abs(R @ R.T - np.eye(3)).max()),
            (msr(T) - msr(Tl)) / (EPS32 * ss * sd), pose)


def numpy_f32_fit(src, dst):
    R, t, _ = umeyama(src, dst, np.float32)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


# Worst figures of numpy's float32 SVD fit (numpy_f32_fit) over 200 seeds per family and k, measured by measure_umeyama()
# (python tests/ransac_model_f64.py): (family, k) -> (residual excess in eps32 sigma_src sigma_dst, pose difference), each
# floored at 16 eps32 (16 for the excess, whose unit already is eps32).  The tests allow 4 x these.
UMEYAMA_BOUNDS = {
    ("good", 3): (16, 1.91e-06), ("good", 4): (16, 1.91e-06), ("good", 64): (16, 1.91e-06),
    ("good", 65): (16, 1.91e-06), ("good", 1000): (16, 1.91e-06),
    ("far", 3): (16, 1.91e-06), ("far", 4): (16, 1.91e-06), ("far", 64): (16, 1.91e-06),
    ("far", 65): (16, 1.91e-06), ("far", 1000): (16, 1.91e-06),
    ("planar", 3): (16, 1.91e-06), ("planar", 4): (16, 1.91e-06), ("planar", 64): (16, 1.91e-06),
    ("planar", 65): (16, 1.91e-06), ("planar", 1000): (16, 1.91e-06),
    ("near_planar", 3): (16, 1.91e-06), ("near_planar", 4): (16, 1.91e-06), ("near_planar", 64): (16, 1.91e-06),
    ("near_planar", 65): (16, 1.91e-06), ("near_planar", 1000): (16, 1.91e-06),
    ("collinear", 3): (16, 1.91e-06), ("collinear", 4): (16, 1.91e-06), ("collinear", 64): (16, 1.91e-06),
    ("collinear", 65): (16, 1.91e-06), ("collinear", 1000): (16, 1.91e-06),
    ("thin", 3): (16, 0.000336), ("thin", 4): (16, 3.97e-05), ("thin", 64): (16, 5.37e-05),
    ("thin", 65): (16, 8.84e-05), ("thin", 1000): (16, 0.00103),
    ("tiny", 3): (16, 1.91e-06), ("tiny", 4): (16, 1.91e-06), ("tiny", 64): (16, 1.91e-06),
    ("tiny", 65): (16, 1.91e-06), ("tiny", 1000): (16, 1.91e-06),
    ("huge", 3): (16, 1.91e-06), ("huge", 4): (16, 1.91e-06), ("huge", 64): (16, 1.91e-06),
    ("huge", 65): (16, 1.91e-06), ("huge", 1000): (16, 1.91e-06),
}


def check_umeyama(family, k, src, dst, T):
    """Violations of float32 fits T (sets, 4, 4) of the sets src / dst (sets, k, 3) of a family, and the worst figures
    (det, orthogonality, residual excess, pose difference).  Properness and the residual for every family, the pose where
    the data determines it."""
    ex_bound, pose_bound = UMEYAMA_BOUNDS[family, k]
    bad, worst = [], np.zeros(4)
    for i in range(len(src)):
        q = np.array(umeyama_quality(src[i], dst[i], T[i]))
        worst = np.maximum(worst, q)
        if not (q[0] < 1e-5 and q[1] < 1e-5):
            bad.append("set %d: |det R - 1| %.3g, |R R^T - I| %.3g" % (i, q[0], q[1]))
        if not q[2] < 4 * ex_bound:
            bad.append("set %d: residual excess %.3g eps32 sigma sigma, bound %.3g" % (i, q[2], 4 * ex_bound))
        if family in POSE_FAMILIES and not q[3] < 4 * pose_bound:
            bad.append("set %d: pose difference %.3g, bound %.3g" % (i, q[3], 4 * pose_bound))
    return bad, worst


def umeyama_sets(family, k, seeds=200):
    """The (seeds, k, 3) sets of a family that the bounds were measured on and the tests run on."""
    return family_points(family, k, np.random.default_rng([FAMILIES.index(family), k]), seeds)


def measure_umeyama(seeds=200):
    table = {}
    for fam in FAMILIES:
        for k in UMEYAMA_K:
            s, d = umeyama_sets(fam, k, seeds)
            q = np.array([umeyama_quality(s[i], d[i], numpy_f32_fit(s[i], d[i])) for i in range(seeds)])
            table[fam, k] = (max(q[:, 2].max(), 16.0), max(q[:, 3].max(), 16 * EPS32))
    return table


def measure_w():
    """The smallest w (1.25-step grid from 1e-8) at which the float32 run of the model stays inside the float64 brackets on
    every run of RUNS, per run."""
    worst = {}
    for run in RUNS:
        m64, m32 = run_model(run), run_model(run, dtype=np.float32)
        if m64.M < 3:
            continue
        c32, ok = m32.counts(), m64.well_conditioned()
        w = 1e-8
        while True:
            lo, hi = m64.count_bracket(None, w)
            if ((c32 >= lo) & (c32 <= hi))[ok].all():
                break
            w *= 1.25
        worst[run[0]] = (w, int((~ok).sum()))
    return worst


if __name__ == "__main__":
    ws = measure_w()
    for name, (w, ex) in ws.items():
        print("%-16s w %.2e   set aside %d" % (name, w, ex))
    print("measured w: %.2e" % max(w for w, _ in ws.values()))
    for (fam, k), (ex, ps) in measure_umeyama().items():
        print('    ("%s", %d): (%.3g, %.3g),' % (fam, k, ex, ps))
