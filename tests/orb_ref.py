"""The yardstick of ORB description (putslam_amd/csrc/ps_orb.h): the project's reading of OpenCV 3.0 - 3.3's
ORB_Impl::detectAndCompute with useProvidedKeypoints = true -- orb.cpp, the 8-bit resize(INTER_LINEAR), the 8-bit separable
GaussianBlur and cvtColor -- restated twice: `*_loops` with scalar loops, the plain names vectorised.  No OpenCV was at hand: the
reading is UNPINNED.  The device is held to it byte for byte.

Everything but the rotation is integer arithmetic; cv_round rounds half to even; float operations are single IEEE binary32
operations (numpy's float32 scalars and arrays round every operation on its own).

  grey     1 channel: as it is.  3 channels: COLOR_BGR2GRAY, (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14.
  levels   scale_l = (float)pow((double)scaleFactor, l); rows_l = cv_round((float)rows / scale_l), cols_l alike; level 0 is the grey
           image, level l is resized from level l - 1.
  resize   11-bit coefficients: scale = 1.0 / ((double)dn / sn); f = (float)((dx + 0.5) * scale - 0.5); s = floor(f); f -= s;
           columns: s < 0 -> (0, 0), s >= sn - 1 -> (sn - 1, 0); a0 = cv_round((1.f - f) * 2048.f), a1 = cv_round(f * 2048.f);
           rows: f is kept, the indices s and s + 1 are clamped to 0 .. sn - 1.
           h = S[s] * a0 + S[min(s + 1, sn - 1)] * a1;  out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.
  blur     taps {18, 34, 49, 55, 49, 34, 18} (they sum to 257), rows first then columns, in int, min(255, (v + 32768) >> 16),
           BORDER_REFLECT_101 of the unblurred level in borderInterpolate's form (length 1: index 0; else reflect until inside).
  kept     31 <= x < cols - 31, 31 <= y < rows - 31 (float compares, NaN fails), 0 <= octave < nLevels; grouped by octave
           ascending, input order inside an octave.
  row      s = 1.f / scale_octave; centre (cv_round(x * s), cv_round(y * s)); (a, b) = rotation(angle);
           ix = cv_round(px * a - py * b), iy = cv_round(px * b + py * a); bit p = v(point 0) < v(point 1);
           v = the blurred level inside the level, the raw level at the REFLECT_101 index outside.
  rotation (the project's own fixed sequence, no fused operation anywhere)
           angle not finite or |angle| > 2^20: taken as 0.
           q = rint(angle * (float)(1 / 90.)); r = angle - q * 90.f (exact); k = (int)q & 3; t = r * (float)(pi / 180);
           u = t * t;
           S = ((((S9 * u + S7) * u + S5) * u + S3) * (t * u)) + t,         Sn = (float)(+-1 / n!)
           C = (((((C10 * u + C8) * u + C6) * u + C4) * u + C2) * u) + 1.f,  Cn = (float)(+-1 / n!)
           (a, b) = (C, S), (-S, C), (-C, -S), (S, -C) for k = 0 .. 3.
  pattern  256 x (x0, y0, x1, y1) int8 in -15 .. 15.  Default: SplitMix64 from state 0x5055545F4F5242; per draw u, coordinate i is
           ((u >> 8i) & 15) + ((u >> (8i + 4)) & 15) - 15; a draw whose two points are equal is drawn again.
"""
import math

import numpy as np

f32 = np.float32
TAPS = (18, 34, 49, 55, 49, 34, 18)
EDGE = 31
PATTERN_SEED = 0x5055545F4F5242
M64 = (1 << 64) - 1

S3, S5, S7, S9 = f32(-1.0 / 6), f32(1.0 / 120), f32(-1.0 / 5040), f32(1.0 / 362880)
C2, C4, C6, C8, C10 = f32(-0.5), f32(1.0 / 24), f32(-1.0 / 720), f32(1.0 / 40320), f32(-1.0 / 3628800)
INV90 = f32(1.0 / 90.0)
DEG = f32(math.pi / 180.0)
ANGLE_MAX = f32(1048576.0)


def cv_round(v):
    return int(np.rint(v))


# ---- pattern ----
def default_pattern():
    """(256, 4) int8"""
    state = PATTERN_SEED
    out = np.zeros((256, 4), np.int8)
    n = 0
    while n < 256:
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        c = [((z >> (8 * i)) & 15) + ((z >> (8 * i + 4)) & 15) - 15 for i in range(4)]
        if c[0] == c[2] and c[1] == c[3]:
            continue
        out[n] = c
        n += 1
    return out


# ---- levels ----
def level_geometry(rows, cols, scale_factor=1.2, n_levels=8):
    """[(rows_l, cols_l, scale_l float32)]"""
    out = []
    for l in range(n_levels):
        scale = f32(math.pow(float(f32(scale_factor)), float(l)))
        out.append((cv_round(f32(rows) / scale), cv_round(f32(cols) / scale), scale))
    return out


def gray(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    c = img.astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def resize_coeffs(sn, dn, columns):
    """(s0, s1, a0, a1) int arrays of dn entries: the two source indices and their 11-bit weights"""
    scale = 1.0 / (float(dn) / sn)
    s0, s1, a0, a1 = [], [], [], []
    for d in range(dn):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = f32(f - f32(s))
        if columns:
            if s < 0:
                s, f = 0, f32(0)
            if s >= sn - 1:
                s, f = sn - 1, f32(0)
        s0.append(min(max(s, 0), sn - 1))
        s1.append(min(max(s + 1, 0), sn - 1))
        a0.append(cv_round(f32(f32(1) - f) * f32(2048)))
        a1.append(cv_round(f * f32(2048)))
    return np.array(s0), np.array(s1), np.array(a0), np.array(a1)


def resize_loops(src, dr, dc):
    sr, sc = src.shape
    x0, x1, a0, a1 = resize_coeffs(sc, dc, True)
    y0, y1, b0, b1 = resize_coeffs(sr, dr, False)
    out = np.zeros((dr, dc), np.uint8)
    for y in range(dr):
        for x in range(dc):
            h0 = int(src[y0[y], x0[x]]) * int(a0[x]) + int(src[y0[y], x1[x]]) * int(a1[x])
            h1 = int(src[y1[y], x0[x]]) * int(a0[x]) + int(src[y1[y], x1[x]]) * int(a1[x])
            out[y, x] = (((int(b0[y]) * (h0 >> 4)) >> 16) + ((int(b1[y]) * (h1 >> 4)) >> 16) + 2) >> 2
    return out


def resize(src, dr, dc):
    sr, sc = src.shape
    x0, x1, a0, a1 = resize_coeffs(sc, dc, True)
    y0, y1, b0, b1 = resize_coeffs(sr, dr, False)
    s = src.astype(np.int64)
    h = s[:, x0] * a0[None, :] + s[:, x1] * a1[None, :]
    v = ((b0[:, None] * (h[y0] >> 4)) >> 16) + ((b1[:, None] * (h[y1] >> 4)) >> 16)
    return ((v + 2) >> 2).astype(np.uint8)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def reflect101_v(p, n):
    p = np.array(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p, np.where(hi, 2 * n - 2 - p, p))


def blur_loops(src):
    r, c = src.shape
    h = np.zeros((r, c), np.int64)
    for y in range(r):
        for x in range(c):
            h[y, x] = sum(TAPS[i] * int(src[y, reflect101(x + i - 3, c)]) for i in range(7))
    out = np.zeros((r, c), np.uint8)
    for y in range(r):
        for x in range(c):
            v = sum(TAPS[j] * int(h[reflect101(y + j - 3, r), x]) for j in range(7))
            out[y, x] = min(255, (v + 32768) >> 16)
    return out


def blur(src):
    r, c = src.shape
    s = src.astype(np.int64)
    xs = [reflect101_v(np.arange(c) + i - 3, c) for i in range(7)]
    ys = [reflect101_v(np.arange(r) + j - 3, r) for j in range(7)]
    h = sum(TAPS[i] * s[:, xs[i]] for i in range(7))
    v = sum(TAPS[j] * h[ys[j], :] for j in range(7))
    return np.minimum(255, (v + 32768) >> 16).astype(np.uint8)


def pyramid(img, scale_factor=1.2, n_levels=8, loops=False):
    """[(raw, blurred, scale)] per level"""
    rs, bl = (resize_loops, blur_loops) if loops else (resize, blur)
    g = gray(img)
    out = []
    for l, (r, c, scale) in enumerate(level_geometry(g.shape[0], g.shape[1], scale_factor, n_levels)):
        assert r >= 1 and c >= 1
        raw = g if l == 0 else rs(out[-1][0], r, c)
        out.append((raw, bl(raw), scale))
    return out


# ---- rotation ----
def rotation(angle):
    """(a, b) float32 = (cos, sin) of `angle` degrees, the fixed sequence of the docstring; scalar or array"""
    ang = np.asarray(angle, f32)
    with np.errstate(invalid="ignore"):
        ang = np.where(np.abs(ang) <= ANGLE_MAX, ang, f32(0)).astype(f32)
    q = np.rint(ang * INV90).astype(f32)
    r = (ang - q * f32(90)).astype(f32)
    k = q.astype(np.int64) & 3
    t = (r * DEG).astype(f32)
    u = (t * t).astype(f32)
    s = (((S9 * u + S7) * u + S5) * u + S3).astype(f32)
    s = (s * (t * u) + t).astype(f32)
    c = ((((C10 * u + C8) * u + C6) * u + C4) * u + C2).astype(f32)
    c = (c * u + f32(1)).astype(f32)
    a = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s))).astype(f32)
    b = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c))).astype(f32)
    return a, b


def rotation_loops(angle):
    ang = f32(angle)
    if not (abs(ang) <= ANGLE_MAX):
        ang = f32(0)
    q = f32(np.rint(f32(ang * INV90)))
    r = f32(ang - f32(q * f32(90)))
    k = int(q) & 3
    t = f32(r * DEG)
    u = f32(t * t)
    s = S9
    for co in (S7, S5, S3):
        s = f32(f32(s * u) + co)
    s = f32(f32(s * f32(t * u)) + t)
    c = C10
    for co in (C8, C6, C4, C2):
        c = f32(f32(c * u) + co)
    c = f32(f32(c * u) + f32(1))
    return ((c, s), (f32(-s), c), (f32(-c), f32(-s)), (s, f32(-c)))[k]


# ---- description ----
def keep_order(xy, octave, rows, cols, n_levels):
    """input indices of the described key points in output order"""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    octave = np.asarray(octave, np.int32).reshape(-1)
    out = []
    if rows > 2 * EDGE and cols > 2 * EDGE:
        for l in range(n_levels):
            for i in range(len(octave)):
                x, y = xy[i]
                if octave[i] == l and f32(EDGE) <= x < f32(cols - EDGE) and f32(EDGE) <= y < f32(rows - EDGE):
                    out.append(i)
    return np.array(out, np.int32)


def new_counters():
    return dict(outside=0, reach=0, samples=0, bounced=0)


def describe_loops(pyr, xy, angle, octave, pattern=None, counters=None):
    """(desc (k, 32) uint8, kept_idx (k,) int32) of the key points over pyramid() levels.  counters (new_counters()) gathers how
    many samples fell outside their level, how far at most, and how many reflected more than once."""
    pattern = default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    angle = np.asarray(angle, f32).reshape(-1)
    octave = np.asarray(octave, np.int32).reshape(-1)
    rows, cols = pyr[0][0].shape
    kept = keep_order(xy, octave, rows, cols, len(pyr))
    desc = np.zeros((len(kept), 32), np.uint8)
    for j, i in enumerate(kept):
        raw, blr, scale = pyr[octave[i]]
        r, c = raw.shape
        s = f32(f32(1) / scale)
        cx, cy = cv_round(f32(xy[i, 0] * s)), cv_round(f32(xy[i, 1] * s))
        a, b = rotation_loops(angle[i])

        def v(px, py):
            ix = cv_round(f32(f32(f32(px) * a) - f32(f32(py) * b)))
            iy = cv_round(f32(f32(f32(px) * b) + f32(f32(py) * a)))
            x, y = cx + ix, cy + iy
            if counters is not None:
                counters["samples"] += 1
            if 0 <= x < c and 0 <= y < r:
                return int(blr[y, x])
            if counters is not None:
                counters["outside"] += 1
                d = max(-x, x - (c - 1), -y, y - (r - 1))
                counters["reach"] = max(counters["reach"], d)
                once = lambda p, n: n == 1 or 0 <= (-p if p < 0 else (2 * n - 2 - p if p >= n else p)) < n  # noqa: E731
                if not (once(x, c) and once(y, r)):
                    counters["bounced"] += 1
            return int(raw[reflect101(y, r), reflect101(x, c)])

        for p in range(256):
            x0, y0, x1, y1 = (int(t) for t in pattern[p])
            if v(x0, y0) < v(x1, y1):
                desc[j, p >> 3] |= 1 << (p & 7)
    return desc, kept


def describe(pyr, xy, angle, octave, pattern=None, counters=None):
    """describe_loops as array operations; counters as there (tests/test_orb_ref_host.py holds the two to each other)"""
    pattern = default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    angle = np.asarray(angle, f32).reshape(-1)
    octave = np.asarray(octave, np.int32).reshape(-1)
    rows, cols = pyr[0][0].shape
    with np.errstate(invalid="ignore"):
        ok = (xy[:, 0] >= f32(EDGE)) & (xy[:, 0] < f32(cols - EDGE)) & (xy[:, 1] >= f32(EDGE)) & (xy[:, 1] < f32(rows - EDGE))
    ok &= (octave >= 0) & (octave < len(pyr)) & (rows > 2 * EDGE) & (cols > 2 * EDGE)
    idx = np.nonzero(ok)[0]
    kept = idx[np.argsort(octave[idx], kind="stable")].astype(np.int32)
    desc = np.zeros((len(kept), 32), np.uint8)
    pat = pattern.astype(f32)
    for l, (raw, blr, scale) in enumerate(pyr):
        rows_j = np.nonzero(octave[kept] == l)[0]
        if len(rows_j) == 0:
            continue
        i = kept[rows_j]
        r, c = raw.shape
        s = f32(f32(1) / scale)
        cx = np.rint(xy[i, 0] * s).astype(np.int64)[:, None]
        cy = np.rint(xy[i, 1] * s).astype(np.int64)[:, None]
        a, b = rotation(angle[i])
        a, b = a[:, None], b[:, None]
        vals = []
        for o in (0, 2):
            px, py = pat[None, :, o], pat[None, :, o + 1]
            x = cx + np.rint(px * a - py * b).astype(np.int64)
            y = cy + np.rint(px * b + py * a).astype(np.int64)
            inside = (x >= 0) & (x < c) & (y >= 0) & (y < r)
            xr, yr = reflect101_v(x, c), reflect101_v(y, r)
            if counters is not None:
                counters["samples"] += int(inside.size)
                counters["outside"] += int((~inside).sum())
                if not inside.all():
                    reach = np.maximum(np.maximum(-x, x - (c - 1)), np.maximum(-y, y - (r - 1)))
                    counters["reach"] = max(counters["reach"], int(reach[~inside].max()))
                    once_x = np.where(x < 0, -x, np.where(x >= c, 2 * c - 2 - x, x))
                    once_y = np.where(y < 0, -y, np.where(y >= r, 2 * r - 2 - y, y))
                    ok_x = (once_x >= 0) & (once_x < c) if c > 1 else np.ones_like(inside)
                    ok_y = (once_y >= 0) & (once_y < r) if r > 1 else np.ones_like(inside)
                    counters["bounced"] += int((~inside & ~(ok_x & ok_y)).sum())
            vals.append(np.where(inside, blr[yr, xr], raw[yr, xr]).astype(np.int64))
        desc[rows_j] = np.packbits(vals[0] < vals[1], axis=1, bitorder="little")
    return desc, kept


# ---- inputs shared by the host and the device tests ----
SCENES = ("noise", "c255", "c128", "checker", "ramp")


def scene(name, rows, cols, cn, seed=0):
    """(rows, cols) or (rows, cols, 3) uint8"""
    shape = (rows, cols) if cn == 1 else (rows, cols, cn)
    if name == "noise":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if name == "c255":
        return np.full(shape, 255, np.uint8)
    if name == "c128":
        return np.full(shape, 128, np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols]
    base = ((yy + xx) & 1) * 255 if name == "checker" else (xx * 3 + yy * 5 + seed) & 255
    base = base.astype(np.uint8)
    return base if cn == 1 else np.stack([base, np.roll(base, 1, 1), 255 - base], axis=2)


def texture(rows, cols, seed=0):
    """a grey image with structure at every pyramid level: blocks of noise at three sizes"""
    rng = np.random.default_rng(seed)
    img = np.zeros((rows, cols), np.float64)
    for b, w in ((1, 0.2), (3, 0.3), (8, 0.5)):
        blk = rng.integers(0, 256, ((rows + b - 1) // b, (cols + b - 1) // b)).astype(np.float64)
        img += w * np.kron(blk, np.ones((b, b)))[:rows, :cols]
    return np.clip(img, 0, 255).astype(np.uint8)


def random_keypoints(n, rows, cols, n_levels, seed=0):
    """n key points all of which are kept: (xy (n, 2) float32, angle (n,) float32, octave (n,) int32), octaves unsorted"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(EDGE, cols - EDGE - 0.01, n), rng.uniform(EDGE, rows - EDGE - 0.01, n)], axis=1).astype(f32)
    angle = rng.uniform(0, 360, n).astype(f32)
    octave = rng.integers(0, n_levels, n).astype(np.int32)
    return xy, angle, octave


def edge_keypoints(rows, cols, n_levels):
    """the named cases: the bounds of x and y and the floats just inside / outside, NaN, octaves -1 and n_levels, the rounding
    ties 40.5 / 41.5, the named angles, every octave"""
    lo, hi_x, hi_y = f32(EDGE), f32(cols - EDGE), f32(rows - EDGE)
    below = lambda v: np.nextafter(f32(v), f32(-1e9))  # noqa: E731
    mx, my = f32(cols / 2), f32(rows / 2)
    pts = []
    for x in (lo, below(lo), hi_x, below(hi_x), f32(np.nan)):
        pts.append((x, my, 10.0, 0))
    for y in (lo, below(lo), hi_y, below(hi_y), f32(np.nan)):
        pts.append((mx, y, 20.0, 1))
    pts += [(mx, my, 0.0, -1), (mx, my, 0.0, n_levels), (40.5, 41.5, 0.0, 0), (41.5, 40.5, 33.0, 0)]
    for ang in (-1.0, 0.0, 45.0, 90.0, 359.5):
        for l in range(n_levels):
            pts.append((mx + l, my - l * 0.25, ang, l))
    a = np.array(pts, np.float64)
    return a[:, :2].astype(f32), a[:, 2].astype(f32), a[:, 3].astype(np.int32)


def corner_pattern():
    """the default pattern with a +-15 corner pair first and a pair of equal points (its bit is 0) second"""
    p = default_pattern().copy()
    p[0] = (15, 15, -15, -15)
    p[1] = (3, -4, 3, -4)
    p[2] = (-15, 15, 15, -15)
    return p
