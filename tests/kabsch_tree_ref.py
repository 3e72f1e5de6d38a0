"""The summation tree of ps_kabsch_f64 restated in numpy (no GPU), plus the point-cloud families and the extended-precision
reference that tests/test_kabsch_tree_host.py and tests/test_gpu_standalone_geometry.py share.

kabsch_tree(A, B, ld) performs, operation for operation, what the kernels of putslam_amd/csrc/ps_geometry.h perform:

  n <= 16384 (ps_kabsch_f64_kernel, one wavefront, G = 1) and n > 16384 (ps_kabsch_f64_sums / _cov / _finish, G =
  min(ceil(n / 4096), 1024) wavefronts) share the shape
    - a lane's partial sum runs sequentially from 0.0 over i = g*64 + lane, += G*64;
    - a wavefront's sum is lane 0 of v + shfl_down(v, o) for o = 1, 2, 4, 8, 16, 32;
    - the means are sum / (double)n, the points are centred with those means;
    - the nine products a[r] * b[c] are rounded before they are added (the device code is built with -ffp-contract=off);
  and differ in how the G per-wave results meet: the single wavefront uses its tree's result as it is, the multi-wave form
  adds the per-wave partials in wave order starting from 0.0 (kabsch_means, ps_kabsch_f64_finish).
  Then: the oracle's f64 Jacobi SVD (the device repeats its operation order: oracle/po_svd.inc), the handedness d = -1 iff
  det(V) det(W) < 0 (kabsch_handedness, cofactor determinants), R = (W0 V0 + W1 V1) + (W2 d) V2 and
  t = (R0 (-cA0) + (R1 (-cA1) + R2 (-cA2))) + cB.

Numpy adds, subtracts, multiplies and divides float64 arrays with one IEEE operation per element and never fuses, so the
result is the device's, byte for byte (NaN payloads apart).
"""
import numpy as np

from oracle import oracle_py

SINGLE_WAVE_MAX = 16384      # ps_kabsch_f64: n <= this -> one wavefront
POINTS_PER_WAVE = 4096       # G = ceil(n / this) ...
MAX_WAVES = 1024             # ... capped here


def waves(n):
    """G of a call with n points."""
    return 1 if n <= SINGLE_WAVE_MAX else min((n + POINTS_PER_WAVE - 1) // POINTS_PER_WAVE, MAX_WAVES)


def _lane_sums(n, G, chunk):
    """Per-lane partial sums, (G, 64, C): lane (g, l) adds chunk rows i = g*64 + l, += G*64 sequentially from 0.0.
    chunk(i0, m) -> the (m, C) summands of points i0 .. i0+m."""
    W = G * 64
    s = None
    for i0 in range(0, n, W):                       # one trip of every lane
        m = min(W, n - i0)
        x = chunk(i0, m)
        if s is None:
            s = np.zeros((W, x.shape[1]), np.float64)
        s[:m] = s[:m] + x                           # lanes past the end of the last trip keep their sum
    return s.reshape(G, 64, -1)


def _wave_tree(v):
    """Lane 0 of v = v + shfl_down(v, o), o = 1 .. 32, per wavefront: (G, 64, C) -> (G, C)."""
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _in_wave_order(part):
    """(G, C) -> (C,): s = 0.0; for g: s += part[g]."""
    s = np.zeros(part.shape[1], np.float64)
    for g in range(part.shape[0]):
        s = s + part[g]
    return s


def det3(M):
    """det3 of ps_device_math.h: the cofactor expansion along the first row, every product and difference rounded."""
    return ((M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]))
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def tree_sums(A, B):
    """(cA, cB, H, G): the means and the 3x3 covariance sum the kernels hand to the SVD."""
    n = A.shape[0]
    G = waves(n)
    AB = np.concatenate([A, B], axis=1)                                     # (n, 6): sa[0..2], sb[0..2]
    part = _wave_tree(_lane_sums(n, G, lambda i0, m: AB[i0:i0 + m]))        # (G, 6)
    sums = part[0] if n <= SINGLE_WAVE_MAX else _in_wave_order(part)
    mean = sums / np.float64(n)
    cA, cB = mean[:3], mean[3:]

    def products(i0, m):
        a = A[i0:i0 + m] - cA
        b = B[i0:i0 + m] - cB
        return (a[:, :, None] * b[:, None, :]).reshape(m, 9)
    part2 = _wave_tree(_lane_sums(n, G, products))                          # (G, 9)
    H = (part2[0] if n <= SINGLE_WAVE_MAX else _in_wave_order(part2)).reshape(3, 3)
    return cA, cB, H, G


def kabsch_tree(A, B, ld=None):
    """The 4x4 float64 pose ps_kabsch_f64 returns for the (n,3) clouds A, B.  ld: as oracle_py.kabsch_f64 takes it (views of
    column-major storage with that leading dimension); the elements are read through the view, so no padding row is."""
    A, B, n, ld = oracle_py.column_major_ld(A, B, ld)
    T = np.eye(4)
    if n == 0:
        return T
    with np.errstate(all="ignore"):
        cA, cB, H, _ = tree_sums(A, B)
        V, _, W = oracle_py.jacobi_svd3(H, np.float64)      # V = svd.matrixU(), W = svd.matrixV()
        d = np.float64(-1.0 if det3(V) * det3(W) < 0.0 else 1.0)     # kabsch_handedness
        for i in range(3):
            R = [(W[i, 0] * V[j, 0] + W[i, 1] * V[j, 1]) + (W[i, 2] * d) * V[j, 2] for j in range(3)]
            T[i, :3] = R
            T[i, 3] = (R[0] * (-cA[0]) + (R[1] * (-cA[1]) + R[2] * (-cA[2]))) + cB[i]
    return T


# ----------------------------------------------------------------------------------------------------------------------
# extended-precision reference
def longdouble_ok():
    return np.finfo(np.longdouble).eps < 2e-19


def reference_moments(A, B):
    """(cA, cB, H) with np.longdouble means and covariance (pairwise-summed by numpy, 64-bit mantissa)."""
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    cA, cB = Al.mean(0), Bl.mean(0)
    H = (Al - cA).T @ (Bl - cB)
    return cA, cB, H


def kabsch_reference(A, B):
    """(T, sigma): the Kabsch pose from extended-precision moments, a numpy float64 SVD and the reflection handled by the
    sign of det(H); sigma = the singular values of H, descending."""
    cA, cB, H = reference_moments(A, B)
    H64 = H.astype(np.float64)
    U, S, Vt = np.linalg.svd(H64)
    d = 1.0 if np.linalg.det(H64) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (cB - R.astype(np.longdouble) @ cA).astype(np.float64)
    return T, S


def optimal_residual(A, B):
    """max |R A + t - B| of the reference pose, evaluated in extended precision."""
    T, _ = kabsch_reference(A, B)
    return residual(T, A, B)


def residual(T, A, B):
    Tl = T.astype(np.longdouble)
    return float(np.abs(A.astype(np.longdouble) @ Tl[:3, :3].T + Tl[:3, 3] - B.astype(np.longdouble)).max())


# ----------------------------------------------------------------------------------------------------------------------
# point-cloud families
def rotation(rng, max_deg=40.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-max_deg, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


CONDITIONED = ("centred", "offset1e3", "offset1e6", "scale1e-6", "scale1e6")


def conditioned_cloud(kind, n, seed):
    """A well-spread cloud and its rotated, shifted, lightly perturbed copy: R is determined (sigma3 / sigma1 of the
    covariance is far above 1e-3 for n >= 4)."""
    rng = np.random.default_rng([seed, n, CONDITIONED.index(kind)])
    A = rng.uniform(-1.0, 1.0, (n, 3))
    R = rotation(rng)
    B = A @ R.T + rng.normal(0, 1e-3, (n, 3))
    t = np.array([0.1, 0.2, -0.3])
    if kind == "offset1e3":
        A, B = A + 1e3, B + 1e3 + t
    elif kind == "offset1e6":
        A, B = A + 1e6, B + 1e6 + t
    elif kind == "scale1e-6":
        A, B = A * 1e-6, (B + t) * 1e-6
    elif kind == "scale1e6":
        A, B = A * 1e6, (B + t) * 1e6
    else:
        B = B + t
    return A, B


DEGENERATE = ("planar", "collinear", "coincident", "mirrored", "three_points")


def degenerate_cloud(kind, n, seed):
    """Rank-deficient and improper inputs: the pose is decided by rounding noise, its properties are not."""
    rng = np.random.default_rng([seed, n, 100 + DEGENERATE.index(kind)])
    R = rotation(rng)
    t = np.array([0.1, 0.2, -0.3])
    if kind == "planar":
        A = rng.uniform(-1, 1, (n, 3)) * [1, 1, 0]
        return A, A @ R.T + t
    if kind == "collinear":
        A = np.outer(rng.uniform(-1, 1, n), [1.0, 2.0, -0.5])
        return A, A @ R.T + t
    if kind == "coincident":                # H = 0 exactly: det == 0 and the SVD's scale == 0
        return np.tile([0.25, -0.5, 2.0], (n, 1)), np.tile([1.0, 0.5, 1.5], (n, 1))
    if kind == "mirrored":                  # B = A diag(1, 1, -1): the best proper rotation is not the best orthogonal map
        # (a box of unequal sides: with d = -1 the rotation is as well determined as sigma2 - sigma3 is large, and an
        # isotropic cloud has all three singular values within 1 / sqrt(n) of each other)
        A = rng.uniform(-1, 1, (n, 3)) * [1.0, 0.6, 0.3]
        return A, A * [1, 1, -1]
    A = rng.uniform(-1, 1, (3, 3))          # any 3 points: rank 2 at the most
    return A, A @ R.T + t
