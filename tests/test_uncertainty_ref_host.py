"""The measurement uncertainty without a GPU: the restatement (tests/uncertainty_ref.py) against what needs no tolerance -- the
integer direction rule against the literal libm expression, the tie table at every magnitude, exact normals, the border guard, the
16-bit patch read, the identity --, the correctly rounded cube against this host's pow, and the new part of the C ABI: names,
struct sizes, defaults, NULL contexts, the header as plain C, and the pure-host rules under the sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import uncertainty_ref as U  # noqa: E402

NEW_NAMES = ["ps_sensor_model_default", "ps_debug_gradient_tie_table", "ps_feature_uncertainty", "ps_measurement_edges", "ps_compute_normals",
             "ps_compute_rgb_gradients", "ps_information_matrices", "ps_abi_sizeof_sensor_model", "ps_abi_sizeof_uncertainty_out",
             "ps_abi_sizeof_measurement_edges_out"]
K = np.array([20.0, 0, 9.5, 0, 19.0, 6.5, 0, 0, 1], np.float32)
SCALE = 5000.0
MAGNITUDES = (1, 2, 3, 7, 1000, 12345, 16 * 65535)
G_MAX = 16 * 65535       # |gradx|, |grady| <= (3 + 10 + 3) x 65535


# ------------------------------------------------------------------------------------------------------------ the direction
def test_integer_direction_rule_equals_the_libm_expression_off_the_ties():
    """Random gradients over the whole range and the neighbours of about 3 200 sampled points of the four diagonals, the smallest and
    the largest among them"""
    rng = np.random.RandomState(1)
    g = rng.randint(-G_MAX, G_MAX + 1, size=(200000, 2))
    small = rng.randint(-40, 41, size=(20000, 2))
    d = np.concatenate([rng.randint(1, G_MAX, size=3000), np.arange(1, 200), [G_MAX - 1, G_MAX]])
    near = [(sx * a, sy * (a + e)) for a in d.tolist() for sx in (1, -1) for sy in (1, -1) for e in (-1, 1)]
    near += [(y, x) for x, y in near]
    checked = 0
    for gx, gy in g.tolist() + small.tolist() + near:
        if abs(gx) == abs(gy) or max(abs(gx), abs(gy)) > G_MAX:
            continue
        assert U.direction(gx, gy) == U.direction_libm(float(gx), float(gy)), (gx, gy)
        checked += 1
    assert checked > 240000


def test_tie_table_does_not_depend_on_the_magnitude():
    from putslam_amd import api
    one = U.tie_table(1)
    for k in MAGNITUDES:
        assert U.tie_table(k) == one, k
        assert api.gradient_tie_table(k).tolist() == [list(r) for r in one], k       # the library's libm is this host's
    assert all(v in (-1, 0, 1) for r in one for v in r)
    # a tie is decided by the table and by nothing else
    for k in MAGNITUDES:
        for (sx, sy), row in zip(U.TIE_CASES, one):
            assert U.direction(sx * k, sy * k) == tuple(row)


# --------------------------------------------------------------------------------------------------------- exact geometry
def test_constant_depth_gives_an_exact_axis_normal_at_every_interior_pixel():
    depth = np.full((14, 20), 7000, np.uint16)
    for v in range(1, 13):
        for u in range(1, 19):
            n = U.compute_normal(depth, u, v, K, SCALE)
            assert n[0] == 0 and n[1] == 0 and abs(n[2]) == 1.0, (u, v, n)


def test_pixel_without_neighbours_gives_the_nan_pattern():
    depth = np.zeros((14, 20), np.uint16)
    depth[5, 7] = 4000                       # the centre alone has depth: it is not tested
    xy = np.float32([[7.0, 5.0], [7.9, 5.2], [3.0, 3.0]])
    got = U.rows(xy, np.zeros((3, 3), np.float32), depth, None, K, SCALE, U.sensor(), -1, want=("normal",))["normal"]
    assert (got.view(np.uint64) == U.NAN_BITS).all()
    one = depth.copy()
    one[5, 8] = 4100                         # one neighbour: its cross product with itself is zero, 0 / 0
    got = U.rows(xy[:1], np.zeros((1, 3), np.float32), one, None, K, SCALE, U.sensor(), -1, want=("normal",))["normal"]
    assert (got.view(np.uint64) == U.NAN_BITS).all()


def test_border_guard_returns_unnormalised_ones():
    rows, cols = 14, 20
    rng = np.random.RandomState(2)
    depth = rng.randint(1000, 9000, size=(rows, cols)).astype(np.uint16)
    image = rng.randint(0, 256, size=(rows, cols, 3)).astype(np.uint8)
    for u in range(cols):
        for v in range(rows):
            g = U.compute_rgb_gradient(image, depth, u, v, K, SCALE)
            border = u in (0, 1, cols - 1) or v in (0, 1, rows - 1)
            assert (g == [1.0, 1.0, 1.0]) == border, (u, v, g)
            if not border:
                assert abs(float((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) - 1.0) < 1e-12 or np.isnan(g[0])


def test_patch_read_is_the_sixteen_bit_read_of_the_colour_image():
    """A hand-computed example in a 6 x 5 image whose rows lie 23 bytes apart: at (u, v) = (3, 2) the patch starts at byte
    1 x 23 + 2 x 3 = 29; words at bytes +0, +2, +4 of three rows"""
    parent = np.arange(6 * 23, dtype=np.uint8).reshape(6, 23) * 3 + 1           # byte b holds (3 b + 1) mod 256
    image = np.lib.stride_tricks.as_strided(parent, (6, 5, 3), (23, 3, 1))
    byte = lambda b: (3 * b + 1) % 256   # noqa: E731
    want = [[byte(r * 23 + 6 + 2 * c) + 256 * byte(r * 23 + 7 + 2 * c) for c in range(3)] for r in (1, 2, 3)]
    assert want[0][0] == byte(29) + 256 * byte(30) == 88 + 256 * 91
    got = U.patch_words(image, 3, 2)
    assert got == want
    gx, gy = U.gradients_of(got)
    assert gx == -3 * want[0][0] - 10 * want[0][1] - 3 * want[0][2] + 3 * want[2][0] + 10 * want[2][1] + 3 * want[2][2]
    assert gy == -3 * want[0][0] - 10 * want[1][0] - 3 * want[2][0] + 3 * want[0][2] + 10 * want[1][2] + 3 * want[2][2]
    # ... and not the grey value, nor one channel: the word spans two channels of one pixel or two pixels
    assert got[0][0] & 0xFF == image[1, 2, 0] and got[0][0] >> 8 == image[1, 2, 1] and got[0][1] & 0xFF == image[1, 2, 2] and got[0][1] >> 8 == image[1, 3, 0]


def test_model_minus_one_is_the_identity_and_bad_pixels_are_nan():
    depth = np.full((14, 20), 7000, np.uint16)
    xy = np.float32([[3.0, 4.0], [np.nan, 4.0], [3.0, 3e9], [-2147483648.0, 1.0], [2147483520.0, 1.0]])
    got = U.rows(xy, np.ones((5, 3), np.float32), depth, None, K, SCALE, U.sensor(), -1, want=("info", "normal"))
    assert got["info"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and got["info"][4].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert (got["info"][1:4].view(np.uint64) == U.NAN_BITS).all() and (got["normal"][1:4].view(np.uint64) == U.NAN_BITS).all()


def test_inverse_and_products_on_exact_cases():
    m = [[np.float64(v) for v in r] for r in ([2, 0, 0], [0, 4, 0], [0, 0, 8])]
    assert np.array(U.inverse(m)).tolist() == [[0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.125]]
    # dense products: a structural zero times a NaN is a NaN
    n = [[np.float64(np.nan), np.float64(0), np.float64(0)], [np.float64(0)] * 3, [np.float64(0)] * 3]
    with np.errstate(all="ignore"):
        assert np.isnan(np.array(U.mat_mul(U.identity(), n))[:, 0]).all()
    # model 0 at the principal point of a unit camera: diag(1 / (z^2 varU), 1 / (z^2 varV), 1 / var(z))
    s = U.sensor(fu=1, fv=1, cu=3, cv=4, varU=0.5, varV=0.25, c3=0, c2=0, c1=0, c0=2)
    info = np.array(U.info_image_coordinates(s, 3.9, 4.2, 2.0))
    assert info.tolist() == [[0.5, 0, 0], [0, 1.0, 0], [0, 0, 0.5]]
    with np.errstate(all="ignore"):
        assert np.isnan(np.array(U.info_image_coordinates(s, -1.0, 4.0, 2.0))).all()
        assert np.isnan(np.array(U.info_image_coordinates(s, np.nan, 4.0, 2.0))).all()


# ----------------------------------------------------------------------------------------------------------------- the cube
def test_cube_is_correctly_rounded_and_pow_is_within_one_ulp():
    """computeCov's pow(depth, 3.0) over every depth a 16-bit image holds at scales 5000 and 1000: z z z in double IS the correctly
    rounded cube of a float-valued z (the definition); this host's pow may differ from it, never by more than one ulp."""
    differ = total = 0
    for scale in (5000.0, 1000.0):
        z = (np.arange(1, 65536, dtype=np.float64) / scale).astype(np.float32).astype(np.float64)
        cube = z * z * z
        for zi, ci in zip(z.tolist(), cube.tolist()):
            f = Fraction(zi)
            exact = float(f * f * f)
            assert ci == exact, zi
            p = math.pow(zi, 3.0)
            if p != exact:
                differ += 1
                assert abs(p - exact) <= math.ulp(exact), zi
            total += 1
    print("pow(z, 3.0) differs from the correctly rounded cube in %d of %d cases" % (differ, total))
    assert total == 131070


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_uncertainty()
    assert sizes == {"sensor_model": 96, "uncertainty_out": 24, "measurement_edges_out": 64}
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size, name


def test_new_names_are_declared_exported_and_bound():
    from putslam_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "putslam_hip.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED, name
        fn = getattr(L, name)
        assert fn.argtypes is not None or name.startswith("ps_abi_sizeof_"), name
    lo = header.index("---- Measurement uncertainty")
    assert sorted(set(re.findall(r"\b(ps_\w+)\(", re.sub(r"/\*.*?\*/", " ", header[lo:], flags=re.S)))) == sorted(NEW_NAMES)


def test_sensor_model_default_is_the_headers():
    from putslam_amd import _lib
    from putslam_amd._abi import PsSensorModel, sensor_model
    L = _lib.load()
    s = PsSensorModel(*([-1.0] * 12))
    assert L.ps_sensor_model_default(C.byref(s)) == 0 and L.ps_sensor_model_default(None) == -1
    want = [582.64, 586.97, 320.17, 260.0, 1.1046, 0.64160, -8.9997e-06, 3.069e-003, 3.6512e-006, -0.0017512e-3, 0.0, 0.0]
    assert [getattr(s, n) for n in U.SENSOR_FIELDS] == want
    assert [getattr(sensor_model(), n) for n in U.SENSOR_FIELDS] == want == [U.SENSOR_DEFAULT[n] for n in U.SENSOR_FIELDS]
    assert [n for n, _ in PsSensorModel._fields_] == list(U.SENSOR_FIELDS)
    assert sensor_model(scaleUncertaintyNormal=3).scaleUncertaintyNormal == 3.0


def test_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsDepthSet, PsMapBatch, PsMeasurementEdgesOut, PsPairResults, PsUncertaintyOut, frame_geometry, sensor_model
    L = _lib.load()
    g, s, ds = frame_geometry(np.eye(3).ravel()), sensor_model(), PsDepthSet()
    out = np.full(9, 7.0)
    pv = out.ctypes.data_as(C.c_void_p)
    assert L.ps_feature_uncertainty(None, C.byref(g), C.byref(s), 0, None, C.byref(ds), None, None, None, None, 1, 8, C.byref(PsUncertaintyOut())) == -1
    assert L.ps_measurement_edges(None, C.byref(g), C.byref(s), 0, None, C.byref(ds), None, C.byref(PsMapBatch()), C.byref(PsPairResults()), None,
                                  C.byref(PsMeasurementEdgesOut())) == -1
    assert L.ps_compute_normals(None, C.byref(g), None, 4, 4, 0, None, 1, pv) == -1
    assert L.ps_compute_rgb_gradients(None, C.byref(g), None, 3, 0, None, 4, 4, 0, None, 1, pv) == -1
    assert L.ps_information_matrices(None, C.byref(g), C.byref(s), 0, None, 3, 0, None, 4, 4, 0, None, None, 1, pv) == -1
    assert (out == 7.0).all()
    assert L.ps_debug_gradient_tie_table(1, None) == -1 and L.ps_debug_gradient_tie_table(0, pv) == -1


def test_header_section_is_plain_c(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "abi_check_uncertainty.c"), "-o", str(tmp_path / "abi_check_uncertainty.o")])


def test_pure_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_uncertainty_rule.cpp: the sensor defaults, the tie table and the argument rule in a stand-alone program built
    with -fsanitize=address,undefined, on the CPU"""
    exe = str(tmp_path / "test_uncertainty_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "putslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_uncertainty_rule.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("uncertainty rule ok"), run.stdout
    ties = [int(x) for x in run.stdout.splitlines()[0].split()[1:]]
    assert ties == [v for r in U.tie_table(1) for v in r]
