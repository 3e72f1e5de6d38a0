"""The measurement uncertainty of the frame loop, restated sequentially: RGBD::computeNormal and RGBD::computeRGBGradient
(src/RGBD/RGBD.cpp:100-187), DepthSensorModel::computeCov, informationMatrixFromImageCoordinates, uncertinatyFromNormal,
uncertinatyFromRGBGradient and normalizeVector (src/Grabber/depthSensorModel.cpp:27-36,55-101), and the choice FeaturesMap::addFeatures
/ addMeasurements make among them (src/Map/featuresMap.cpp:110-121,261-274).  numpy scalars, every operation rounded separately, in
the order the reference's expressions give; what ps_feature_uncertainty and ps_measurement_edges (putslam_amd/csrc/ps_uncertainty.h)
must equal byte for byte.

The rules the reference leaves open are include/putslam_hip.h's ("Measurement uncertainty"): the pixel is the truncation of the float
coordinate; a NaN coordinate or one of magnitude 2^31 or more gives NaN everywhere; every NaN is the pattern 0x7FF8000000000000; the
direction of the gradient is an integer rule off the diagonals and this host's libm on the five ties; Eigen's 3 x 3 inverse is the
cofactor form stated there (no Eigen was at hand: that reading is unpinned).

SEEN counts what the restatement met -- kept neighbours 0 .. 8, the gradient's branches -- so that a test can assert its inputs
reach every one."""
import collections
import math

import numpy as np

f32, f64 = np.float32, np.float64
NAN_BITS = np.uint64(0x7FF8000000000000)
PIXEL_LIMIT = 2147483520.0          # the largest float below 2^31: the truncation and its two neighbours fit an int
UIDX = (-1, -1, -1, 0, 1, 1, 1, 0)  # RGBD.cpp:105-106
VIDX = (-1, 0, 1, 1, 1, 0, -1, -1)
TIE_CASES = ((0, 0), (1, 1), (-1, 1), (-1, -1), (1, -1))   # (gradx, grady) of the table's rows
SENSOR_FIELDS = ("fu", "fv", "cu", "cv", "varU", "varV", "c3", "c2", "c1", "c0", "scaleUncertaintyNormal", "scaleUncertaintyGradient")
# DepthSensorModel::Config(), depthSensorModel.h:53-58; the two scale factors are not set there
SENSOR_DEFAULT = dict(fu=582.64, fv=586.97, cu=320.17, cv=260.0, varU=1.1046, varV=0.64160, c3=-8.9997e-06, c2=3.069e-003, c1=3.6512e-006,
                      c0=-0.0017512e-3, scaleUncertaintyNormal=0.0, scaleUncertaintyGradient=0.0)

SEEN = collections.Counter()


def canon(a):
    """The array with every NaN replaced by the one pattern"""
    a = np.array(a, f64)
    a.view(np.uint64)[np.isnan(a)] = NAN_BITS
    return a


def nan_rows(shape):
    return np.full(shape, NAN_BITS, np.uint64).view(f64)


# ------------------------------------------------------------------------------------------------------------ point2Dto3D
def round_size(x, size):
    """RGBD::roundSize (RGBD.cpp:10-16) on a double that is not NaN"""
    x = float(x)
    if x < 0:
        x = 0.0
    elif x > size - 1:
        x = float(size)
    return int(math.floor(x + 0.5))


def point2Dto3D(x, y, depth, K, scale):
    """ps_assemble_frames' arithmetic on the frame as the dense image the reference holds: u == cols in a row that is not the last
    reads the next row's first pixel, u == cols in the last row and v == rows read depth 0.  depth: (rows, cols) uint16."""
    x, y = f32(x), f32(y)
    rows, cols = depth.shape
    off = round_size(x, cols) + round_size(y, rows) * cols
    dv = int(depth[off // cols, off % cols]) if off < rows * cols else 0
    Z = f32(f64(dv) / f64(scale))
    u = (x - f32(K[2])) / f32(K[0])
    v = (y - f32(K[5])) / f32(K[4])
    return u * Z, v * Z, Z


def pixel_of(u, v):
    """((int)u, (int)v), or None where the reference's conversion is undefined"""
    u, v = float(u), float(v)
    if not (abs(u) <= PIXEL_LIMIT and abs(v) <= PIXEL_LIMIT):      # (a NaN fails)
        return None
    return int(u), int(v)


def normalize(v):
    """Eigen's norm() of a Vector3d and three divisions (normalizeVector; RGBD.cpp:141-142,184-185)"""
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / n, v[1] / n, v[2] / n]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ------------------------------------------------------------------------------------------------------------- the normal
def compute_normal(depth, u, v, K, scale):
    """RGBD::computeNormal on the pixel (u, v)"""
    c = point2Dto3D(f32(u), f32(v), depth, K, scale)
    vecs = []
    for du, dv in zip(UIDX, VIDX):
        p = point2Dto3D(f32(u + du), f32(v + dv), depth, K, scale)
        if p[2] > 0:
            vecs.append([f64(p[0] - c[0]), f64(p[1] - c[1]), f64(p[2] - c[2])])     # the difference in float, widened
    SEEN["kept", len(vecs)] += 1
    normals = [cross(vecs[i], vecs[(i + 1) % len(vecs)]) for i in range(len(vecs))]
    s = [f64(0.0), f64(0.0), f64(0.0)]
    for n in normals:
        s = [s[0] + n[0], s[1] + n[1], s[2] + n[2]]
    k = f64(len(normals))
    return normalize([s[0] / k, s[1] / k, s[2] / k])


# ----------------------------------------------------------------------------------------------------------- the gradient
def tie_table(k=1):
    """coord1 / coord2 of RGBD.cpp:164-166 on the five ties at magnitude k, by the literal expression with this host's libm:
    rows TIE_CASES, columns coord1[0], coord1[1], coord2[0], coord2[1]"""
    t = []
    for sx, sy in TIE_CASES:
        t.append(direction_libm(float(sx * k), float(sy * k)))
    return t


def direction_libm(gradx, grady):
    angle = math.atan2(grady, gradx) + (math.pi / 2.0)
    return (int(math.sqrt(2) * math.sin(angle)), int(math.sqrt(2) * math.cos(angle)),
            int(math.sqrt(2) * math.sin(angle + math.pi)), int(math.sqrt(2) * math.cos(angle + math.pi)))


def sgn(x):
    return (x > 0) - (x < 0)


def direction(gradx, grady, ties=None):
    """(coord1[0], coord1[1], coord2[0], coord2[1]) of integer gradients: the integer rule, the table on a tie"""
    ax, ay = abs(gradx), abs(grady)
    if ax == ay:
        ties = ties or tie_table()
        return tuple(ties[TIE_CASES.index((sgn(gradx), sgn(grady)))])
    c = (sgn(gradx) if ax > ay else 0, -sgn(grady) if ay > ax else 0)
    return c + (-c[0], -c[1])


def patch_words(image, u, v):
    """The 3 x 3 patch as the reference reads it, at<uint16_t> on the 8-bit 3-channel image: the little-endian 16-bit word at
    byte (v-1+r) x rowStride + (u-1) x 3 + 2 c.  image: (rows, cols, 3) uint8, rows any stride apart."""
    out = [[0] * 3 for _ in range(3)]
    for r in range(3):
        row = image[v - 1 + r].reshape(-1)
        for c in range(3):
            at = (u - 1) * 3 + 2 * c
            out[r][c] = int(row[at]) | int(row[at + 1]) << 8
    return out


def gradients_of(p):
    gradx = -3 * p[0][0] - 10 * p[0][1] - 3 * p[0][2] + 3 * p[2][0] + 10 * p[2][1] + 3 * p[2][2]
    grady = -3 * p[0][0] - 10 * p[1][0] - 3 * p[2][0] + 3 * p[0][2] + 10 * p[1][2] + 3 * p[2][2]
    return gradx, grady


def compute_rgb_gradient(image, depth, u, v, K, scale, ties=None):
    """RGBD::computeRGBGradient on the pixel (u, v)"""
    rows, cols = depth.shape
    if not ((u - 1 > 0) and (v - 1 > 0) and (u + 1 < cols) and (v + 1 < rows)):
        SEEN["branch", "border"] += 1
        return [f64(1), f64(1), f64(1)]
    gradx, grady = gradients_of(patch_words(image, u, v))
    if abs(gradx) == abs(grady):
        SEEN["tie", sgn(gradx), sgn(grady)] += 1
    c1x, c1y, c2x, c2y = direction(gradx, grady, ties)
    cen = point2Dto3D(f32(u), f32(v), depth, K, scale)
    end = point2Dto3D(f32(u + c1x), f32(v + c1y), depth, K, scale)
    beg = point2Dto3D(f32(u + c2x), f32(v + c2y), depth, K, scale)
    diff = lambda a, b: [f64(a[0] - b[0]), f64(a[1] - b[1]), f64(a[2] - b[2])]   # noqa: E731
    if end[2] > 0 and beg[2] != 0:
        g, branch = diff(end, beg), "end-beg"
    elif cen[2] > 0 and beg[2] != 0:
        g, branch = diff(cen, beg), "cen-beg"
    elif cen[2] > 0 and end[2] != 0:
        g, branch = diff(end, cen), "end-cen"
    else:
        g, branch = [f64(c1x), f64(c1y), f64(0)], "fallback"
    SEEN["branch", branch] += 1
    return normalize(g)


# ------------------------------------------------------------------------------------------------------------ the matrices
def mat_mul(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def transpose(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def inverse(m):
    """The project's reading of Eigen 3's fixed-size 3 x 3 inverse"""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]
    det = (cof(0, 0) * m[0][0] + cof(1, 0) * m[1][0]) + cof(2, 0) * m[2][0]
    invdet = f64(1.0) / det
    return [[cof(j, i) * invdet for j in range(3)] for i in range(3)]


def identity():
    return [[f64(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]


def sensor(**fields):
    s = dict(SENSOR_DEFAULT)
    s.update(fields)
    return {k: f64(v) for k, v in s.items()}


def compute_cov(s, u, v, depth):
    """DepthSensorModel::computeCov(u, v, depth) for unsigned u, v: z^2 = z z and z^3 = z z z, the correctly rounded powers of a
    float-valued z"""
    u, v, z = f64(u), f64(v), f64(depth)
    zero, one = f64(0.0), f64(1.0)
    J = [[z / s["fu"], zero, (u / s["fu"]) - (s["cu"] / s["fu"])], [zero, z / s["fv"], (v / s["fv"]) - (s["cv"] / s["fv"])], [zero, zero, one]]
    R = [[s["varU"], zero, zero], [zero, s["varV"], zero], [zero, zero, ((s["c3"] * (z * z * z) + s["c2"] * (z * z)) + s["c1"] * z) + s["c0"]]]
    return mat_mul(mat_mul(J, R), transpose(J))


def info_image_coordinates(s, u, v, z):
    """informationMatrixFromImageCoordinates(u, v, z) on the float coordinates widened: (unsigned long) truncates; a negative,
    NaN or too large value is undefined there and a NaN matrix here"""
    ud, vd = f64(f32(u)), f64(f32(v))
    if not (0.0 <= ud < 2.0 ** 64 and 0.0 <= vd < 2.0 ** 64):
        return [[f64(np.nan)] * 3 for _ in range(3)]
    return inverse(compute_cov(s, f64(int(ud)), f64(int(vd)), f64(f32(z))))


def from_basis(cols3, d, scale):
    """((R S) S) R^-1 for R with the given columns and S = the identity with S(d, d) = scale"""
    R = [[cols3[j][i] for j in range(3)] for i in range(3)]
    S = identity()
    S[d][d] = f64(scale)
    return mat_mul(mat_mul(mat_mul(R, S), S), inverse(R))


def uncertainty_from_normal(s, normal):
    """uncertinatyFromNormal: y = normal x (1, 0, 0) is taken before the normalisation and never normalised itself"""
    n = [f64(c) for c in normal]
    y = cross(n, [f64(1), f64(0), f64(0)])
    n = normalize(n)
    x = normalize(cross(y, n))
    return from_basis([x, y, n], 2, s["scaleUncertaintyNormal"])


def uncertainty_from_rgb_gradient(s, grad):
    """uncertinatyFromRGBGradient: only S(1, 1) is set"""
    g = [f64(c) for c in grad]
    y = normalize(cross([f64(0), f64(0), f64(1)], g))
    z = normalize(cross(y, g))
    return from_basis([g, y, z], 1, s["scaleUncertaintyGradient"])


# ---------------------------------------------------------------------------------------------------------------- the rows
def rows(xy, pts, depth, image, K, scale, s, model, ties=None, want=("normal", "gradient", "info")):
    """One row set in one frame: dict(normal (n, 3), gradient (n, 3), info (n, 9)) of the wanted members, float64 with canonical
    NaNs.  depth None = the frame lies outside the set: every row NaN.  image is needed for the gradient and for model 2 only."""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    n = len(xy)
    out = {k: nan_rows((n, 9 if k == "info" else 3)) for k in want}
    if depth is None:
        return out
    ties = ties or tie_table()
    with np.errstate(all="ignore"):
        for i in range(n):
            px = pixel_of(xy[i, 0], xy[i, 1])
            if px is None:
                SEEN["bad pixel"] += 1
                continue
            normal = grad = None
            if "normal" in want or ("info" in want and model == 1):
                normal = compute_normal(depth, px[0], px[1], K, scale)
            if "gradient" in want or ("info" in want and model == 2):
                grad = compute_rgb_gradient(image, depth, px[0], px[1], K, scale, ties)
            if "normal" in want:
                out["normal"][i] = canon(normal)
            if "gradient" in want:
                out["gradient"][i] = canon(grad)
            if "info" in want:
                if model == 0:
                    m = info_image_coordinates(s, xy[i, 0], xy[i, 1], pts[i][2])
                elif model == 1:
                    m = inverse(uncertainty_from_normal(s, normal))
                elif model == 2:
                    m = inverse(uncertainty_from_rgb_gradient(s, grad))
                else:
                    m = identity()
                out["info"][i] = canon(np.array(m, f64).reshape(9))
    return out


def measurement_edges(matches, num_matches, mask, pairs, num_maps, frame_pts, xy_undist, image_frame, depths, images, K, scale, s, model,
                      max_matches, want=("normal", "gradient", "info")):
    """matcher.cpp:769-794 then featuresMap.cpp:255-282 for P pairs: pair p's final inliers in match-list order.  matches (P,
    max_matches) structured (queryIdx, trainIdx, ...), mask (P, max_matches); frame_pts (F, cap, 3), xy_undist (F, cap, 2); depths /
    images: lists of frames.  Returns a list of dicts per pair: count, mapRow, curRow, uv, position and the wanted members."""
    F, cap = frame_pts.shape[:2]
    out = []
    for p, (view, fr) in enumerate(np.asarray(pairs).tolist()):
        m = int(num_matches[p])
        if m <= 0 or m > max_matches or not 0 <= view < num_maps or not 0 <= fr < F:
            out.append(dict(count=0))
            continue
        idx = np.flatnonzero(mask[p, :m] != 0)
        q, t = matches["queryIdx"][p, idx].astype(np.int32), matches["trainIdx"][p, idx].astype(np.int32)
        # include/putslam_hip.h: a trainIdx outside 0 .. maxKpts - 1 is not followed: that row's uv and position are NaN (the
        # float NaN 0x7FC00000), and so every member; mapRow and curRow still carry the list's values
        follow = (t >= 0) & (t < cap)
        at = np.where(follow, t, 0)
        uv, pt = np.array(xy_undist[fr, at], f32), np.array(frame_pts[fr, at], f32)
        uv[~follow], pt[~follow] = np.nan, np.nan
        g = int(image_frame[fr])
        inside = 0 <= g < len(depths) and (images is None or g < len(images))
        r = rows(uv, pt, depths[g] if inside else None, images[g] if inside and images is not None else None, K, scale, s, model, want=want)
        r.update(count=len(idx), mapRow=q, curRow=t, uv=uv.astype(f32), position=canon(pt.astype(f64)))
        out.append(r)
    return out
