"""Host half of the Kabsch pin (no GPU): the restated summation tree of tests/kabsch_tree_ref.py against the oracle where the
two summation orders coincide, both against an extended-precision reference where the rotation is determined, and the
properties of the pose where it is not.  The GPU half (tests/test_gpu_standalone_geometry.py) holds ps_kabsch_f64 to the
restatement byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kabsch_tree_ref as kt  # noqa: E402

EPS = float(np.finfo(np.float64).eps)

# (b): err_tree <= max(M * err_oracle, 16 eps max(1, max|A|, max|B|)).
M_RATIO = 4.0
SIZES = (4, 64, 65, 500, 16384, 16385, 100003)


def _scale(A, B):
    return max(1.0, float(np.abs(A).max()), float(np.abs(B).max()))


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tree_equals_the_oracle_where_the_orders_coincide(oracle, n):
    """Up to three points the lane-strided partial sums and the shuffle tree add in the oracle's sequential order (every
    further summand is +0.0), so the restatement and po_kabsch_f64 must agree byte for byte -- on every family, the
    degenerate and non-finite ones included."""
    clouds = [kt.conditioned_cloud(k, n, s) for k in kt.CONDITIONED for s in range(8)]
    clouds += [kt.degenerate_cloud(k, n, s) for k in kt.DEGENERATE for s in range(4)]
    A, B = kt.conditioned_cloud("centred", n, 99)
    for bad in (np.nan, np.inf, -np.inf):
        A2 = A.copy()
        A2[n - 1, 1] = bad
        clouds += [(A2, B), (B, A2)]
    clouds.append((A * 1e-310, B * 1e-310))                      # subnormal coordinates
    for A, B in clouds:
        n_ = A.shape[0]         # ("three_points" has three whatever n says)
        if n_ > 3:
            continue
        Tt, To = kt.kabsch_tree(A, B), oracle.kabsch_f64(A, B)
        nan = np.isnan(To)
        assert np.array_equal(np.isnan(Tt), nan) and Tt[~nan].tobytes() == To[~nan].tobytes()


def test_ld_reaches_both_sides_and_padding_is_not_read(oracle):
    n, ld = 65, 72
    A, B = kt.conditioned_cloud("centred", n, 5)
    sa, sb = np.full((3, ld), np.nan), np.full((3, ld), np.nan)     # column-major storage, NaN in the padding rows
    sa[:, :n], sb[:, :n] = A.T, B.T
    Av, Bv = sa[:, :n].T, sb[:, :n].T
    assert Av.strides == (8, 8 * ld)
    assert kt.kabsch_tree(Av, Bv, ld).tobytes() == kt.kabsch_tree(A, B).tobytes()
    assert oracle.kabsch_f64(Av, Bv, ld).tobytes() == oracle.kabsch_f64(A, B).tobytes()
    with pytest.raises(AssertionError):
        oracle.kabsch_f64(A, B, ld)                                 # dense row-major arrays are not such a view


def test_wave_counts():
    assert [kt.waves(n) for n in (1, 16384, 16385, 20480, 20481, 4194304, 4194305, 5000000)] == [1, 1, 5, 5, 6, 1024, 1024, 1024]


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", kt.CONDITIONED)
def test_tree_is_as_close_to_extended_precision_as_the_oracle(oracle, kind, n):
    """Where the covariance has sigma3 / sigma1 >= 1e-3 the rotation is determined, and the restated tree may not be further
    from the extended-precision pose than M times the oracle's sequential sums are (or 16 eps of the data's magnitude).

    M: measured on the CPU over these five families x seven sizes x 200 seeds each.  Where err_tree exceeds the 16-eps floor
    -- the only inputs M decides -- the worst err_tree / err_oracle is 1.384 (offset 1e6, n = 500); twice that, rounded up to
    a power of two: M = 4.  At large n with an offset the tree is the better of the two (ratio <= 0.5 at n = 100003, offset
    1e3).  Taken over ALL inputs the quotient is meaningless: on the scale-1e6 family both errors sit below the floor and
    err_oracle is occasionally a single rounding of a 1e-10 translation (ratios up to 2.2e5 with err_tree = 1.2e-9 against a
    floor of 4.5e-9), which says nothing about either summation order."""
    if not kt.longdouble_ok():
        pytest.skip("np.longdouble has no 64-bit mantissa here (eps >= 2e-19): no extended-precision reference")
    compared = 0
    for seed in range(12):
        A, B = kt.conditioned_cloud(kind, n, seed)
        Tr, S = kt.kabsch_reference(A, B)
        if S[2] / S[0] < 1e-3:          # (n = 4: four points are sometimes nearly planar)
            continue
        err_tree = float(np.abs(kt.kabsch_tree(A, B) - Tr).max())
        err_oracle = float(np.abs(oracle.kabsch_f64(A, B) - Tr).max())
        assert err_tree <= max(M_RATIO * err_oracle, 16 * EPS * _scale(A, B)), (kind, n, seed, err_tree, err_oracle)
        compared += 1
        if compared == 3:
            break
    assert compared == 3


# ---------------------------------------------------------------------------------------------------------------- (c)
DEGENERATE_CASES = [(k, n) for k in kt.DEGENERATE for n in (3, 4, 65, 500, 16385) if k != "three_points" or n == 3]


@pytest.mark.parametrize("kind,n", DEGENERATE_CASES)
def test_degenerate_inputs_give_a_proper_rotation_with_the_optimal_residual(oracle, kind, n):
    """Planar, collinear, coincident (H = 0: the det == 0 branch and scale == 0 in the SVD), mirrored and three-point sets:
    the reference pose itself is decided by rounding noise, so the restatement and the oracle are held to what any correct
    answer has -- R R^T = I to 64 eps, det R = +1, and a residual within 64 eps x scale of the extended-precision optimum."""
    if not kt.longdouble_ok():
        pytest.skip("np.longdouble has no 64-bit mantissa here (eps >= 2e-19): no extended-precision reference")
    for seed in range(3):
        A, B = kt.degenerate_cloud(kind, n, seed)
        best = kt.optimal_residual(A, B)
        for name, T in (("tree", kt.kabsch_tree(A, B)), ("oracle", oracle.kabsch_f64(A, B))):
            R = T[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 64 * EPS, (name, kind, n, seed)
            assert abs(np.linalg.det(R) - 1.0) <= 64 * EPS, (name, kind, n, seed)
            assert kt.residual(T, A, B) <= best + 64 * EPS * _scale(A, B), (name, kind, n, seed, kt.residual(T, A, B), best)
            assert np.array_equal(T[3], [0, 0, 0, 1])
