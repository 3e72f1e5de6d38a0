"""MatcherOpenCV::detectFeatures for detector = "ORB" (reference src/Matcher/matcherOpenCV.cpp:118-180), restated twice in numpy from
the project's reading of OpenCV 3.0 - 3.3's ORB_Impl::detectAndCompute (key points only), computeKeyPoints, HarrisResponses,
ICAngles, KeyPointsFilter and scalar fastAtan2.  No OpenCV was at hand: the reading is UNPINNED.

 (a) literal      per-level loops; retainBest with an explicit sort and a scan over the ties; Harris over the 49 offsets; the umax
                  loops of ICAngles with the paired rows +-v; scalar fastAtan2; the grid loop with stable argsorts;
 (b) closed form  Sobel maps by shifted arrays and the 7 x 7 sums through an integral image; the moments through one disc mask;
                  vectorised fastAtan2; retainBest as a threshold; the final order as ONE lexicographic key (response descending, ROI
                  in loop order, level, raster position) with the per-ROI cut counted by rank.

FAST, its suppression and the grid come from fast_ref.py, the level geometry and the resize from orb_ref.py: neither is copied.
tests/test_orb_detect_ref_host.py holds (a) and (b) to each other; the GPU tests hold the library to them byte for byte.

Integer arithmetic except where stated; float operations are single IEEE binary32 operations; cv_round rounds half to even.
  grey     the WHOLE image with CV_RGB2GRAY (fast_ref.to_gray: channel 0 weighs 4899), one channel as it is; every ROI of the grid
           is an image of its own with its own pyramid (orb_ref.level_geometry / orb_ref.resize), raw levels only.
  quotas   factor = (float)(1.0 / scaleFactor); nd = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
           q_l = cv_round(nd), nd *= factor for l < nlevels - 1; q_last = max(nfeatures - sum, 0).
  level    FAST-9/16 (threshold clamped to 0 .. 255, suppression, response = score) on the level as an image of its own; kept
           31 <= x < cols - 31, 31 <= y < rows - 31; retainBest(2 q_l) by the score, ties at the cut all kept; Harris (block 7,
           k = 0.04f) at the survivors; retainBest(q_l) by Harris, ties kept; the angle of the intensity centroid (half patch 15).
  list     levels ascending, raster order inside a level (THE PROJECT'S DECISION); pt = (x0 * scale_l, y0 * scale_l).
  order    fast_ref's grid loop: stable by response descending, cut to maxInROI, ROI origin added as floats, joined, cut.
"""
import math

import numpy as np

import fast_ref as F
import orb_ref as O

f32 = np.float32
EDGE = 31
HALF_PATCH = 15
HARRIS_K = f32(0.04)
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
DBL_EPSILON_F = f32(2.220446049250313e-16)
RAD2DEG = f32(180.0 / math.pi)
P1, P3, P5, P7 = (f32(f32(c) * RAD2DEG) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))


def params(n_features=500, scale_factor=1.2, n_levels=8, fast_threshold=20, grid_rows=1, grid_cols=1, max_features=500):
    return dict(n_features=int(n_features), scale_factor=float(f32(scale_factor)), n_levels=int(n_levels), fast_threshold=int(fast_threshold),
                grid_rows=int(grid_rows), grid_cols=int(grid_cols), max_features=int(max_features))


def quotas(n_features, scale_factor=1.2, n_levels=8):
    factor = f32(1.0 / float(f32(scale_factor)))
    nd = f32(f32(f32(n_features) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(n_levels)))))
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(O.cv_round(nd))
        total += out[-1]
        nd = f32(nd * factor)
    out.append(max(n_features - total, 0))
    return out


def umax_construction():
    """OpenCV's construction of umax: cv_round(sqrt(hp^2 - v^2)) up to vmax = floor(hp sqrt(2) / 2 + 1), the rest by symmetry."""
    hp = HALF_PATCH
    half = f32(f32(hp) * f32(np.sqrt(f32(2)))) / f32(2)
    vmax, vmin = int(math.floor(f32(half + f32(1)))), int(math.ceil(half))
    umax = [0] * (hp + 2)
    for v in range(vmax + 1):
        umax[v] = O.cv_round(math.sqrt(float(hp * hp - v * v)))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return tuple(umax[:hp + 1])


# ---------------------------------------------------------------------------------------------- pieces
def fast_atan2(y, x):
    """scalar; degrees"""
    y, x = f32(y), f32(x)
    ax, ay = f32(abs(x)), f32(abs(y))
    c = f32(min(ax, ay) / f32(max(ax, ay) + DBL_EPSILON_F))
    c2 = f32(c * c)
    a = f32(f32(P7 * c2) + P5)
    a = f32(f32(a * c2) + P3)
    a = f32(f32(a * c2) + P1)
    a = f32(a * c)
    if ax < ay:
        a = f32(f32(90) - a)
    if x < 0:
        a = f32(f32(180) - a)
    if y < 0:
        a = f32(f32(360) - a)
    return a


def fast_atan2_v(y, x):
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    c = (np.minimum(ax, ay) / (np.maximum(ax, ay) + DBL_EPSILON_F)).astype(f32)
    c2 = (c * c).astype(f32)
    a = ((((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c).astype(f32)
    a = np.where(ax < ay, f32(90) - a, a).astype(f32)
    a = np.where(x < 0, f32(180) - a, a).astype(f32)
    return np.where(y < 0, f32(360) - a, a).astype(f32)


def harris_sums_literal(img, x0, y0):
    """(a, b, c) over the 7 x 7 block around (x0, y0); img a list of lists or an array"""
    a = b = c = 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y, x = y0 + dy, x0 + dx
            p = lambda oy, ox: int(img[y + oy][x + ox])  # noqa: E731
            ix = (p(0, 1) - p(0, -1)) * 2 + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
            iy = (p(1, 0) - p(-1, 0)) * 2 + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
            a += ix * ix
            b += iy * iy
            c += ix * iy
    return a, b, c


def harris_response(a, b, c):
    """scalar or arrays of ints -> float32"""
    scale = f32(f32(1) / f32(4 * 7 * f32(255)))
    s4 = f32(f32(f32(scale * scale) * scale) * scale)
    fa, fb, fc = np.asarray(a).astype(f32), np.asarray(b).astype(f32), np.asarray(c).astype(f32)
    det = (fa * fb).astype(f32) - (fc * fc).astype(f32)
    tr = (fa + fb).astype(f32)
    return ((det.astype(f32) - ((HARRIS_K * tr).astype(f32) * tr).astype(f32)).astype(f32) * s4).astype(f32)


def ic_angle_literal(img, x0, y0, umax=UMAX):
    m01 = m10 = 0
    for u in range(-HALF_PATCH, HALF_PATCH + 1):
        m10 += u * int(img[y0][x0 + u])
    for v in range(1, HALF_PATCH + 1):
        v_sum = 0
        d = umax[v]
        for u in range(-d, d + 1):
            plus, minus = int(img[y0 + v][x0 + u]), int(img[y0 - v][x0 + u])
            v_sum += plus - minus
            m10 += u * (plus + minus)
        m01 += v * v_sum
    return fast_atan2(f32(m01), f32(m10))


def retain_best_literal(kps, n, key):
    """KeyPointsFilter::retainBest as a set: kps in their order, those whose key(kp) is >= the n-th largest"""
    if n >= len(kps):
        return list(kps)
    if n == 0:
        return []
    ranked = sorted((key(k) for k in kps), reverse=True)
    boundary = ranked[n - 1]
    last = n
    while last < len(ranked) and ranked[last] == boundary:   # the scan over the ties
        last += 1
    out = [k for k in kps if key(k) >= boundary]
    assert len(out) == last
    return out


def pyramid_raw(gray, scale_factor, n_levels, loops=False):
    """[(raw, scale)] of one grey image"""
    rs = O.resize_loops if loops else O.resize
    out = []
    for l, (r, c, scale) in enumerate(O.level_geometry(gray.shape[0], gray.shape[1], scale_factor, n_levels)):
        assert r >= 1 and c >= 1
        out.append((gray if l == 0 else rs(out[-1][0], r, c), scale))
    return out


# ---------------------------------------------------------------------------------------------- (a) literal
def detect_roi_literal(gray, p):
    """The detector on one grey image.  Returns [(x0, y0, level, ptx, pty, response, angle)] levels ascending, raster inside."""
    qs = quotas(p["n_features"], p["scale_factor"], p["n_levels"])
    t = F.clamp_threshold(p["fast_threshold"])
    out = []
    for l, (raw, scale) in enumerate(pyramid_raw(gray, p["scale_factor"], p["n_levels"])):
        R, C = raw.shape
        kps = [k for k in F.fast_literal(raw, t, True)[2] if EDGE <= k[0] < C - EDGE and EDGE <= k[1] < R - EDGE]
        kps = retain_best_literal(kps, 2 * qs[l], lambda k: k[2])
        img = raw.tolist()
        scored = [(k[0], k[1], harris_response(*harris_sums_literal(img, k[0], k[1]))) for k in kps]
        scored = retain_best_literal(scored, qs[l], lambda k: k[2])
        for x, y, r in scored:
            ptx = f32(x) if l == 0 else f32(f32(x) * scale)
            pty = f32(y) if l == 0 else f32(f32(y) * scale)
            out.append((x, y, l, ptx, pty, f32(r), ic_angle_literal(img, x, y)))
    return out


def _pack(rows):
    xy = np.array([[r[0], r[1]] for r in rows], f32).reshape(-1, 2)
    return (xy, np.array([r[2] for r in rows], f32), np.array([r[3] for r in rows], f32), np.array([r[4] for r in rows], np.int32))


def detect_literal(img, p):
    """The grid loop around detect_roi_literal.  Returns (xy (n, 2) f32, response (n,) f32, angle (n,) f32, octave (n,) int32)."""
    gray = F.to_gray(img)
    per_roi = F.max_in_roi(p["max_features"], p["grid_rows"], p["grid_cols"])
    joined = []
    for x0, y0, w, h in F.roi_rects(gray.shape[0], gray.shape[1], p["grid_rows"], p["grid_cols"]):
        kps = detect_roi_literal(gray[y0:y0 + h, x0:x0 + w], p)
        order = np.argsort(-np.array([k[5] for k in kps], np.float64), kind="stable")
        for j in order[:per_roi]:
            k = kps[j]
            joined.append((f32(k[3] + f32(x0)), f32(k[4] + f32(y0)), k[5], k[6], k[2]))
    order = np.argsort(-np.array([k[2] for k in joined], np.float64), kind="stable")
    return _pack([joined[j] for j in order[:p["max_features"]]])


# ---------------------------------------------------------------------------------------------- (b) closed form
_DV, _DU = np.mgrid[-HALF_PATCH:HALF_PATCH + 1, -HALF_PATCH:HALF_PATCH + 1]
_DISC = np.abs(_DU) <= np.array(UMAX)[np.abs(_DV)]
DISC_DU, DISC_DV = _DU[_DISC], _DV[_DISC]


def harris_maps(raw):
    """(a, b, c) int64 maps: the 7 x 7 sums of Ix^2, Iy^2, Ix Iy around every pixel at least 4 from the edge, 0 elsewhere"""
    g = raw.astype(np.int64)
    R, C = g.shape
    ix, iy = np.zeros((R, C), np.int64), np.zeros((R, C), np.int64)
    ix[1:-1, 1:-1] = (g[1:-1, 2:] - g[1:-1, :-2]) * 2 + (g[:-2, 2:] - g[:-2, :-2]) + (g[2:, 2:] - g[2:, :-2])
    iy[1:-1, 1:-1] = (g[2:, 1:-1] - g[:-2, 1:-1]) * 2 + (g[2:, :-2] - g[:-2, :-2]) + (g[2:, 2:] - g[:-2, 2:])
    out = []
    for m in (ix * ix, iy * iy, ix * iy):
        ii = np.zeros((R + 1, C + 1), np.int64)
        ii[1:, 1:] = m.cumsum(0).cumsum(1)
        box = np.zeros((R, C), np.int64)
        box[3:R - 3, 3:C - 3] = ii[7:, 7:] - ii[:-7, 7:] - ii[7:, :-7] + ii[:-7, :-7]
        out.append(box)
    return out


def levels_closed(gray, p):
    """Per level of one grey image: dict(raw, score, x, y -- the survivors of the first cut in raster order --, response, angle, kept
    -- the mask of the second cut --, scale, quota, candidates -- the emitted FAST key points inside the border)."""
    qs = quotas(p["n_features"], p["scale_factor"], p["n_levels"])
    t = F.clamp_threshold(p["fast_threshold"])
    out = []
    for l, (raw, scale) in enumerate(pyramid_raw(gray, p["scale_factor"], p["n_levels"])):
        R, C = raw.shape
        corner, score = F.fast_closed(raw, t)
        mask, _ = F.emitted_closed(corner, score, True)
        border = np.zeros((R, C), bool)
        if R > 2 * EDGE and C > 2 * EDGE:
            border[EDGE:R - EDGE, EDGE:C - EDGE] = True
        y, x = np.nonzero(mask & border)
        s = score[y, x].astype(np.int64)
        cand, n = len(s), 2 * qs[l]
        if n == 0:
            keep = np.zeros(cand, bool)
        elif cand > n:
            keep = s >= np.sort(s)[::-1][n - 1]
        else:
            keep = np.ones(cand, bool)
        y, x = y[keep], x[keep]
        if len(x):
            a, b, c = (m[y, x] for m in harris_maps(raw))
            resp = harris_response(a, b, c)
            I = raw.astype(np.int64)[y[:, None] + DISC_DV[None, :], x[:, None] + DISC_DU[None, :]]
            angle = fast_atan2_v((I * DISC_DV[None, :]).sum(1).astype(f32), (I * DISC_DU[None, :]).sum(1).astype(f32))
        else:
            resp, angle = np.zeros(0, f32), np.zeros(0, f32)
        if qs[l] == 0:
            kept = np.zeros(len(x), bool)
        elif len(x) > qs[l]:
            kept = resp >= np.sort(resp)[::-1][qs[l] - 1]
        else:
            kept = np.ones(len(x), bool)
        out.append(dict(raw=raw, score=score, x=x, y=y, response=resp, angle=angle, kept=kept, scale=scale, quota=qs[l], candidates=cand))
    return out


def detect_closed(img, p, want_levels=False):
    """detectFeatures as one ordering.  Returns (xy, response, angle, octave) [, the levels_closed of every ROI in loop order]."""
    gray = F.to_gray(img)
    per_roi = F.max_in_roi(p["max_features"], p["grid_rows"], p["grid_cols"])
    cols = dict(x=[], y=[], r=[], a=[], o=[], q=[], px=[], py=[])
    all_levels = []
    for q, (x0, y0, w, h) in enumerate(F.roi_rects(gray.shape[0], gray.shape[1], p["grid_rows"], p["grid_cols"])):
        levels = levels_closed(gray[y0:y0 + h, x0:x0 + w], p)
        all_levels.append(levels)
        x = np.concatenate([lv["x"][lv["kept"]] for lv in levels])
        y = np.concatenate([lv["y"][lv["kept"]] for lv in levels])
        r = np.concatenate([lv["response"][lv["kept"]] for lv in levels]).astype(f32)
        a = np.concatenate([lv["angle"][lv["kept"]] for lv in levels]).astype(f32)
        o = np.concatenate([np.full(int(lv["kept"].sum()), l, np.int64) for l, lv in enumerate(levels)])
        sc = np.array([lv["scale"] for lv in levels], f32)[o] if len(o) else np.zeros(0, f32)
        rank = np.empty(len(r), np.int64)     # place inside the ROI: response descending, (level, raster) among equals
        rank[np.lexsort((np.arange(len(r)), -r.astype(np.float64)))] = np.arange(len(r))
        keep = rank < per_roi
        cols["px"].append(((x.astype(f32) * sc).astype(f32) + f32(x0)).astype(f32)[keep])
        cols["py"].append(((y.astype(f32) * sc).astype(f32) + f32(y0)).astype(f32)[keep])
        for name, v in (("x", x), ("y", y), ("r", r), ("a", a), ("o", o)):
            cols[name].append(v[keep])
        cols["q"].append(np.full(int(keep.sum()), q, np.int64))
    c = {k: np.concatenate(v) for k, v in cols.items()}
    order = np.lexsort((c["x"], c["y"], c["o"], c["q"], -c["r"].astype(np.float64)))[:p["max_features"]]
    out = (np.stack([c["px"][order], c["py"][order]], axis=1).astype(f32).reshape(-1, 2), c["r"][order].astype(f32), c["a"][order].astype(f32),
           c["o"][order].astype(np.int32))
    return out + (all_levels,) if want_levels else out


# ---------------------------------------------------------------------------------------------- scenes
def tiled(rows, cols, period=40, seed=11):
    """One period x period patch of blocks and noise repeated: every key point of level 0 recurs with the same neighbourhood, so
    Harris responses tie exactly across the copies that lie inside the border."""
    patch = F.blocks(period, period, seed, 10, noise=0)
    patch = np.clip(patch.astype(np.int32) + np.random.RandomState(seed).randint(-20, 21, size=patch.shape), 0, 255).astype(np.uint8)
    reps = ((rows + period - 1) // period, (cols + period - 1) // period)
    return np.tile(patch, reps)[:rows, :cols]


def scene(name, rows, cols):
    if name == "texture":
        return O.texture(rows, cols, 4)
    if name == "noise256":
        return F.noise256(rows, cols, 7)
    if name == "noise4":
        return F.noise4(rows, cols, 5)
    if name == "tiled":
        return tiled(rows, cols)
    raise KeyError(name)


def colour(gray_like, seed):
    """three channels that differ, so that RGB2GRAY and BGR2GRAY differ"""
    return F.colour(gray_like, seed)


def image(name, rows, cols, cn=1):
    g = scene(name, rows, cols)
    return g if cn == 1 else colour(g, 17)


# The runs of the device tests (tests/test_gpu_orb_detect.py); tests/test_orb_detect_ref_host.py holds (a) to (b) on every one
# and asserts the premises of PREMISE_CASES on (b) first.  (scene, rows, cols, channels, params)
PREMISE_CASES = [
    ("texture", 96, 128, 1, params(12, 1.2, 3)),       # three live levels; 56 x 74 would be the fourth
    ("noise256", 96, 128, 3, params(12, 1.2, 3)),
    ("noise4", 150, 200, 1, params(24, 1.2, 8)),       # five live levels
    ("texture", 150, 200, 3, params(24, 1.2, 8)),
]
TILED_CASE = ("tiled", 150, 200, 1, params(12, 1.2, 3))
PARAM_CASES = [("texture", 96, 128, 1, params(nf, sf, nl, t)) for nf, sf, nl, t in [
    (12, 1.5, 3, 20), (12, 1.2, 1, 20), (24, 1.2, 8, 20), (12, 1.2, 3, 0), (12, 1.2, 3, 255), (0, 1.2, 3, 20), (1, 1.2, 3, 20),
    (2, 1.2, 3, 20),        # quotas 1, 1, 0: the last level's quota is 0
    (500, 1.2, 8, 20)]]     # no cut bites
# maximalTrackedFeatures 0: nothing comes out, and the read-back of the levels still holds both cuts (a draw of tests/fuzz_front_end.py
# found the second cut's flags unwritten by such a call)
PARAM_CASES.append(("texture", 96, 128, 1, params(12, 1.2, 3, 20, 1, 1, 0)))
EDGE_CASES = [("noise256", 63, 64, 1, params(20, 1.2, 8)),     # level 0 has a 1 x 2 interior
              ("noise256", 62, 90, 1, params(20, 1.2, 8))]     # nothing
GRID_CASES = [("texture", 192, 256, cn, params(24, 1.2, 3, 20, gr, gc, mx)) for cn, gr, gc, mx in [
    (1, 1, 1, 20), (3, 2, 2, 30), (1, 2, 3, 30), (1, 2, 3, 500)]]   # ROIs of 192 x 256, 96 x 128 and 96 x 85
ALL_CASES = PREMISE_CASES + [TILED_CASE] + PARAM_CASES + EDGE_CASES + GRID_CASES
