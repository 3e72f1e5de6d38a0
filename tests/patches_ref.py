"""The specification of the sub-pixel matching on patches, restated sequentially: MatchingOnPatches::computePatch,
computeGradient, optimizeLocation and evaluatePatches of the reference's src/Matcher/MatchingOnPatches.cpp:14-246 (DESIGN.md
section 8.17; include/putslam_hip.h states the rules).  The device kernels (putslam_amd/csrc/ps_patches.h) and the C++
restatement (ps_patches_host.h) are held to these bytes.

Every operation is rounded on its own, in the order the reference writes it: doubles are numpy float64, floats numpy float32,
element-wise array operations are one IEEE operation per element (numpy contracts nothing), and the float sums are taken one
element at a time in element order -- `ufunc.accumulate` is r[k] = op(r[k-1], a[k]) by definition; `scalar=True` takes the same
sums in a Python loop over numpy scalars, and a test holds the two to each other.

Eigen's Matrix3f::inverse(), its lazy 3 x 3 outer product and cv::cvtColor(CV_RGB2GRAY) are restated, not run: that reading is
unpinned against a real build.  Two places where the reference reads outside its images are decided here (status 5 and 6)."""
import numpy as np

F32, F64 = np.float32, np.float64
MAX_ITERATIONS, CONVERGED, NAN_HESSIAN, OUT_OF_IMAGE, MOVED_TOO_FAR, OLD_TAPS_OUTSIDE, NEW_TAPS_OUTSIDE = range(7)
NAN32 = np.array([0x7FC00000], np.uint32).view(F32)[0]
NAN64 = np.array([0x7FF8000000000000], np.uint64).view(F64)[0]


def grey(img):
    """rows x cols (as it is) or rows x cols x 3 (CV_RGB2GRAY, ps_fast.h's rule) uint8 -> int32."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img.astype(np.int32)
    c = img.astype(np.int32)
    return (c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14


def half(patch_size):
    return (patch_size - 1) // 2


def old_taps_inside(x, y, h, rows, cols):
    """finite, int(x) - h - 1 >= 0, int(x) + h + 1 <= cols - 1, the same for y"""
    if not (np.isfinite(x) and np.isfinite(y)) or abs(x) >= 2.0 ** 31 or abs(y) >= 2.0 ** 31:
        return False
    ix, iy = int(x), int(y)
    return ix - h - 1 >= 0 and ix + h + 1 <= cols - 1 and iy - h - 1 >= 0 and iy + h + 1 <= rows - 1


def gate_out(x, y, h, rows, cols):
    """the reference's "Out of image" (:139-143)"""
    return bool(np.isnan(x) or np.isnan(y) or x < h or x > cols - h or y < h or y > rows - h)


def new_taps_inside(x, y, h, rows, cols):
    return int(x) + h + 1 <= cols - 1 and int(y) + h + 1 <= rows - 1


def _canon32(a):
    a = np.array(a, F32)
    a[np.isnan(a)] = NAN32
    return a


def _canon64(v):
    return NAN64 if np.isnan(v) else F64(v)


def _walk(op, values, scalar):
    """((0 op v[0]) op v[1]) op ... in float32, one element at a time"""
    values = np.asarray(values, F32)
    if scalar:
        s = F32(0)
        for v in values:
            s = op(s, v)
        return F32(s)
    return op.accumulate(np.concatenate([np.zeros(1, F32), values]), dtype=F32)[-1]


def compute_patch(I, x, y, h):
    """computePatch (:14-51): E float64 in element order (rows i = int(y) - h .. int(y) + h, inside a row j = int(x) - h ..)"""
    x, y = F64(x), F64(y)
    ix, iy = int(x), int(y)
    xs, ys = x - F64(ix), y - F64(iy)
    one = F64(1)
    tl, tr, bl, br = (one - xs) * (one - ys), xs * (one - ys), (one - xs) * ys, xs * ys
    r0, r1, c0, c1 = iy - h, iy + h + 1, ix - h, ix + h + 1
    a = I[r0:r1, c0:c1].astype(F64)
    b = I[r0:r1, c0 + 1:c1 + 1].astype(F64)
    c = I[r0 + 1:r1 + 1, c0:c1].astype(F64)
    d = I[r0 + 1:r1 + 1, c0 + 1:c1 + 1].astype(F64)
    return (((tl * a + tr * b) + bl * c) + br * d).reshape(-1)


def inverse3(m):
    """the float twin of uncertainty_ref's inverse: the project's reading of Eigen 3's fixed 3 x 3 inverse"""
    m = np.asarray(m, F32)

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return F32(F32(m[i1, j1] * m[i2, j2]) - F32(m[i1, j2] * m[i2, j1]))

    with np.errstate(all="ignore"):
        det = F32(F32(F32(cof(0, 0) * m[0, 0]) + F32(cof(1, 0) * m[1, 0])) + F32(cof(2, 0) * m[2, 0]))
        invdet = F32(F32(1) / det)
        r = np.zeros((3, 3), F32)
        for i in range(3):
            for j in range(3):
                r[i, j] = F32(cof(j, i) * invdet)
    return _canon32(r)


def compute_gradient(I, x, y, h, scalar=False):
    """computeGradient (:53-99): gx, gy (E float32) and the inverse Hessian (3 x 3 float32)"""
    ix, iy = int(F64(x)), int(F64(y))
    r0, r1, c0, c1 = iy - h, iy + h + 1, ix - h, ix + h + 1
    gx = (F32(0.5) * (I[r0:r1, c0 + 1:c1 + 1] - I[r0:r1, c0 - 1:c1 - 1]).astype(F32)).reshape(-1)
    gy = (F32(0.5) * (I[r0 + 1:r1 + 1, c0:c1] - I[r0 - 1:r1 - 1, c0:c1]).astype(F32)).reshape(-1)
    J = [gx, gy, np.ones_like(gx)]
    H = np.zeros((3, 3), F32)
    for a in range(3):
        for b in range(3):
            H[a, b] = _walk(np.add, J[a] * J[b], scalar)
    return gx, gy, inverse3(H)


def model(I, x, y, patch_size, scalar=False):
    """(status, patch, gx, gy, inv): status 5 (no model: None arrays), 2 or 1"""
    h = half(patch_size)
    if not old_taps_inside(x, y, h, I.shape[0], I.shape[1]):
        return OLD_TAPS_OUTSIDE, None, None, None, None
    patch = compute_patch(I, x, y, h)
    gx, gy, inv = compute_gradient(I, x, y, h, scalar)
    return (NAN_HESSIAN if np.isnan(inv[0, 0]) else CONVERGED), patch, gx, gy, inv


def optimize(I, patch, gx, gy, inv, x, y, patch_size, max_iter, min_sqrt_increment, scalar=False):
    """optimizeLocation (:101-200) on a given model -> (status, x, y, iterations)"""
    h = half(patch_size)
    rows, cols = I.shape
    x, y = F64(x), F64(y)
    inv = np.asarray(inv, F32).reshape(3, 3)
    if np.isnan(inv[0, 0]):
        return NAN_HESSIAN, x, y, 0
    sx, sy, mean = x, y, F64(0)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            if gate_out(x, y, h, rows, cols):
                return OUT_OF_IMAGE, x, y, it
            if not new_taps_inside(x, y, h, rows, cols):
                return NEW_TAPS_OUTSIDE, x, y, it
            diff = ((compute_patch(I, x, y, h) - patch) + mean).astype(F32)
            t0 = _walk(np.subtract, diff * gx, scalar)
            t1 = _walk(np.subtract, diff * gy, scalar)
            t2 = _walk(np.subtract, diff, scalar)
            inc0 = F32(F32(F32(inv[0, 0] * t0) + F32(inv[0, 1] * t1)) + F32(inv[0, 2] * t2))
            inc1 = F32(F32(F32(inv[1, 0] * t0) + F32(inv[1, 1] * t1)) + F32(inv[1, 2] * t2))
            x = _canon64(x + F64(inc0))
            y = _canon64(y + F64(inc1))
            if F64(F32(F32(inc0 * inc0) + F32(inc1 * inc1))) < F64(min_sqrt_increment):
                if (x - sx) * (x - sx) + (y - sy) * (y - sy) > F64(h * h):
                    return MOVED_TOO_FAR, x, y, it + 1
                return CONVERGED, x, y, it + 1
    return MAX_ITERATIONS, x, y, max_iter


def align(Iold, Inew, ox, oy, nx, ny, patch_size, max_iter, min_sqrt_increment, scalar=False):
    """The fused form -> (status, x, y, iterations, (patch, gx, gy, inv) or None)"""
    st, patch, gx, gy, inv = model(Iold, ox, oy, patch_size, scalar)
    if st == OLD_TAPS_OUTSIDE:
        return st, F64(nx), F64(ny), 0, None
    st, x, y, it = optimize(Inew, patch, gx, gy, inv, nx, ny, patch_size, max_iter, min_sqrt_increment, scalar)
    return st, x, y, it, (patch, gx, gy, inv)


def align_batch(old_img, new_img, old_pts, new_pts, patch_size, max_iter, min_sqrt_increment):
    """n points of one pair of uint8 images -> dict of arrays shaped as the C ABI's (a point without a model has zero rows)"""
    Io, In = grey(old_img), grey(new_img)
    n, E = len(old_pts), patch_size * patch_size
    out = dict(pts=np.array(new_pts, F64).reshape(n, 2).copy(), status=np.zeros(n, np.uint8), iterations=np.zeros(n, np.int32),
               patch=np.zeros((n, E), F64), gx=np.zeros((n, E), F32), gy=np.zeros((n, E), F32), inv=np.zeros((n, 9), F32))
    for k in range(n):
        st, x, y, it, m = align(Io, In, old_pts[k][0], old_pts[k][1], out["pts"][k, 0], out["pts"][k, 1], patch_size, max_iter,
                                min_sqrt_increment)
        out["status"][k], out["iterations"][k] = st, it
        if it > 0:
            out["pts"][k] = (x, y)
        if m is not None:
            out["patch"][k], out["gx"][k], out["gy"][k], out["inv"][k] = m[0], m[1], m[2], m[3].reshape(9)
    return out


def smooth_texture(rows, cols, seed, channels=1, shift=(0, 0), blur=4):
    """A seeded smooth texture as uint8: uniform noise box-blurred `blur` times (3 x 3, wrapping) and stretched to 16 .. 239,
    read at an offset of `shift` = (dy, dx) whole pixels from a larger field: two calls with different shifts give a pair whose
    content moves by exactly that many pixels."""
    rng = np.random.default_rng(seed)
    pad = 16
    out = []
    for _ in range(channels):
        f = rng.random((rows + 2 * pad, cols + 2 * pad))
        for _ in range(blur):
            f = sum(np.roll(np.roll(f, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
        f = (f - f.min()) / (f.max() - f.min())
        g = np.round(16 + 223 * f).astype(np.uint8)
        out.append(g[pad + shift[0]:pad + shift[0] + rows, pad + shift[1]:pad + shift[1] + cols])
    return out[0].copy() if channels == 1 else np.stack(out, -1).copy()


def ulp_up(v):
    return float(np.nextafter(F64(v), np.inf))


def ulp_down(v):
    return float(np.nextafter(F64(v), -np.inf))


def drawn_points(rng, n, rows, cols, h):
    """old positions mostly inside, new ones within two pixels, with the edges and the non-finite values mixed in"""
    old = np.stack([rng.uniform(h + 1, cols - h - 1, n), rng.uniform(h + 1, rows - h - 1, n)], 1)
    new = old + rng.uniform(-2, 2, (n, 2))
    pts = np.concatenate([old, new], 1)
    pts[0] = (h + 1, h + 1, h, h)                                   # the first old position with its taps inside; the gate's corner
    pts[1] = (cols - h - 1, h + 1, h + 1, h + 1)                    # one column too far right: status 5
    pts[2] = (ulp_down(cols - h - 1), ulp_down(rows - h - 1), cols - h, rows - h)   # the last one; a start on the gate, taps outside
    pts[3, 2:] = (ulp_down(h), h + 2)                               # one ulp outside the gate
    pts[4, 2:] = (h + 2, ulp_up(rows - h))
    pts[5, 2:] = (np.nan, h + 2)
    pts[6, 2:] = (h + 2, -np.inf)
    pts[7, :2] = (np.inf, h + 3)
    pts[8, :2] = (h + 3, np.nan)
    pts[9, :2] = (-3e9, 1e300)
    pts[10, 2:] = (cols - h - 0.5, h + 2)                           # inside the gate, taps outside: status 6
    pts[11, 2:] = pts[11, :2]                                        # an exact start
    return pts
