"""The matching on patches without a GPU: tests/patches_ref.py (the specification, MatchingOnPatches.cpp:14-246 restated) on known
answers, and putslam_amd/csrc/ps_patches_host.h (the sequential C++ restatement: the timing control) held to it byte for byte
through tests/cpp/test_patches_host.cpp, a plain program that is also built once under the address and undefined-behaviour
sanitizers."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patches_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "putslam_amd", "csrc")]
SRC = os.path.join(ROOT, "tests", "cpp", "test_patches_host.cpp")
ULP_UP, ULP_DOWN = R.ulp_up, R.ulp_down


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("patches") / "test_patches_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + INC + [SRC, "-o", exe])
    return exe


def run_host(exe, tmp, old, new, pts4, ps, max_iter, min_inc, step=None):
    """old / new: rows x cols (x 3) uint8; pts4: n x (oldX, oldY, newX, newY) -> the dict of patches_ref.align_batch"""
    rows, cols = old.shape[:2]
    cn = 1 if old.ndim == 2 else 3
    step = step or cols * cn
    pts4 = np.ascontiguousarray(pts4, np.float64).reshape(-1, 4)
    n, E = len(pts4), ps * ps

    def padded(img):
        buf = np.full((rows, step), 0xA5, np.uint8)
        buf[:, :cols * cn] = img.reshape(rows, cols * cn)
        return buf.tobytes()

    cases, results = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<8id", rows, cols, cn, step, ps, max_iter, n, 0, min_inc))
        f.write(padded(old) + padded(new) + pts4.tobytes())
    run = subprocess.run([exe, cases, results], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "patches host ok" in run.stdout, run.stdout
    rec = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("pts", "<f8", 2), ("patch", "<f8", E), ("gx", "<f4", E), ("gy", "<f4", E),
                    ("inv", "<f4", 9)])
    got = np.fromfile(results, rec)
    assert len(got) == n
    return got


def assert_same_bytes(got, want, what=""):
    assert got["status"].tolist() == want["status"].tolist(), what
    assert got["iterations"].tolist() == want["iterations"].tolist(), what
    assert got["pts"].tobytes() == want["pts"].tobytes(), what
    for k in ("patch", "gx", "gy", "inv"):
        assert np.ascontiguousarray(got[k]).tobytes() == want[k].tobytes(), (what, k)


CASES = [  # rows, cols, channels, row padding, patchSize, maxIter, minSqrtIncrement
    (48, 64, 1, 5, 5, 50, 5e-7),
    (48, 64, 3, 7, 13, 50, 0.04),
    (61, 97, 1, 0, 17, 50, 0.04),
    (61, 97, 3, 3, 31, 20, 1e-3),
    (48, 64, 1, 0, 3, 1, 0.0),
    (48, 64, 1, 0, 15, 0, 0.04),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-p%d-i%d" % (c[1], c[0], c[2], c[4], c[5]))
def test_cpp_restatement_equals_the_specification_byte_for_byte(host_exe, tmp_path, case):
    rows, cols, cn, pad, ps, max_iter, min_inc = case
    rng = np.random.default_rng(100 + ps)
    old = R.smooth_texture(rows, cols, 7 + ps, cn)
    new = R.smooth_texture(rows, cols, 7 + ps, cn, shift=(1, -1))
    old[2:12, 20:34] = 77                                            # a flat region: NaN inverse Hessians for the small patches
    pts = R.drawn_points(rng, 24, rows, cols, R.half(ps))
    pts[12, :2] = (26.5, 6.5) if ps <= 5 else pts[12, :2]
    got = run_host(host_exe, str(tmp_path), old, new, pts, ps, max_iter, min_inc, step=cols * cn + pad)
    want = R.align_batch(old, new, pts[:, :2], pts[:, 2:], ps, max_iter, min_inc)
    assert_same_bytes(got, want)
    if max_iter > 1:
        assert {1, 3, 5, 6} <= set(want["status"].tolist())
    if ps <= 5:
        assert want["status"][12] == R.NAN_HESSIAN and np.isnan(want["inv"][12]).all()
        assert (want["inv"][12].view(np.uint32) == 0x7FC00000).all()


def test_cpp_restatement_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, on the CPU, over the edges and the non-finite positions"""
    exe = str(tmp_path / "test_patches_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + INC + [SRC, "-o", exe])
    for rows, cols, cn, pad, ps, max_iter, min_inc in CASES[:4]:
        old = R.smooth_texture(rows, cols, 3, cn)
        new = R.smooth_texture(rows, cols, 3, cn, shift=(0, 1))
        pts = R.drawn_points(np.random.default_rng(ps), 16, rows, cols, R.half(ps))
        got = run_host(exe, str(tmp_path), old, new, pts, ps, max_iter, min_inc, step=cols * cn + pad)
        assert_same_bytes(got, R.align_batch(old, new, pts[:, :2], pts[:, 2:], ps, max_iter, min_inc))


# ---------------------------------------------------------------------------- known answers, held by the C++ restatement
def test_known_answers_hold_for_the_cpp_restatement(host_exe, tmp_path):
    """The named known answers as literal expectations on ps_patches_host.h (through tests/cpp/test_patches_host.cpp), not only on
    the Python specification: the exact start, a flat patch, maxIter 0, every status value, the gate's edges and one ulp beyond
    each, the two divergence bands, NaN / +-inf starts, and the known shift."""
    tmp = str(tmp_path)
    tex = R.smooth_texture(48, 64, 11)
    rows, cols, ps, h = 48, 64, 13, 6

    def go(old, new, pts4, ps_=ps, max_iter=50, min_inc=0.04):
        got = run_host(host_exe, tmp, old, new, [pts4] if np.ndim(pts4) == 1 else pts4, ps_, max_iter, min_inc, step=old.shape[1] + 3)
        return got["status"].tolist(), got["iterations"].tolist(), got["pts"]

    # the same image from integer starts: one step, the position unchanged -- at every patch size
    for size in (3, 5, 13, 17, 31):
        hh = R.half(size)
        x, y = float(hh + 9), float(hh + 5)
        st, it, xy = go(tex, tex, (x, y, x, y), size)
        assert (st, it, xy.tolist()) == ([1], [1], [[x, y]]), size
    # a flat patch: status 2, the position untouched; maxIter 0: status 0, untouched, whatever the start
    flat = np.full((rows, cols), 90, np.uint8)
    st, it, xy = go(flat, tex, (20.0, 20.0, 21.25, 19.5))
    assert (st, it, xy.tolist()) == ([2], [0], [[21.25, 19.5]])
    st, it, xy = go(tex, tex, [(20.0, 20.0, 21.25, 19.5), (20.0, 20.0, -5.0, 1e9)], max_iter=0)
    assert (st, it, xy.tolist()) == ([0, 0], [0, 0], [[21.25, 19.5], [-5.0, 1e9]])
    # every status value
    new = R.smooth_texture(48, 64, 11, shift=(0, 1))
    assert go(tex, tex, (30.0, 24.0, 30.0, 24.0))[0] == [1]
    assert go(tex, new, (30.0, 24.0, 30.5, 24.0), max_iter=1, min_inc=0.0)[:2] == ([0], [1])
    assert go(np.full_like(tex, 5), tex, (30.0, 24.0, 30.0, 24.0))[0] == [2]
    assert go(tex, tex, (30.0, 24.0, 5.5, 24.0))[:2] == ([3], [0])
    st, it, xy = go(tex, tex, (30.0, 24.0, 33.0, 24.0), 3, 50, 1e9)
    assert (st, it) == ([4], [1]) and (xy[0, 0] - 33.0) ** 2 + (xy[0, 1] - 24.0) ** 2 > 1.0
    assert go(tex, tex, (6.5, 24.0, 30.0, 24.0))[:2] == ([5], [0])
    assert go(tex, tex, (30.0, 24.0, 57.5, 24.0))[:2] == ([6], [0])
    # the gate's edges (one step allowed, no increment below 0: a point that passes ends with status 0 after its step)
    o = (30.0, 24.0)
    starts = [(float(h), 20.0), (ULP_DOWN(h), 20.0), (20.0, float(h)), (20.0, ULP_DOWN(h)), (float(cols - h), 20.0), (ULP_UP(cols - h), 20.0),
              (20.0, float(rows - h)), (20.0, ULP_UP(rows - h)),
              # the new image's band [cols - h - 1, cols - h]: inside the gate, taps outside; one ulp below it: inside
              (cols - h - 1.0, 20.0), (cols - h - 0.5, 20.0), (ULP_DOWN(cols - h - 1.0), 20.0), (20.0, rows - h - 1.0), (20.0, ULP_DOWN(rows - h - 1.0)),
              (np.nan, 20.0), (20.0, np.nan), (np.inf, 20.0), (20.0, -np.inf)]
    st, it, xy = go(tex, tex, [o + s for s in starts], max_iter=1, min_inc=0.0)
    assert st == [0, 3, 0, 3, 6, 3, 6, 3, 6, 6, 0, 6, 0, 3, 3, 3, 3]
    assert it == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0]
    for k, s in enumerate(starts):
        if it[k] == 0:
            assert xy[k].tobytes() == np.float64(s).tobytes(), k           # untouched, bit for bit (the NaNs too)
    # the old image's band: x in [h + 1, cols - h - 1), y in [h + 1, rows - h - 1); non-finite old positions
    olds = [(h + 1.0, 24.0), (ULP_DOWN(h + 1.0), 24.0), (ULP_DOWN(cols - h - 1.0), 24.0), (cols - h - 1.0, 24.0), (30.0, h + 1.0),
            (30.0, ULP_DOWN(h + 1.0)), (30.0, ULP_DOWN(rows - h - 1.0)), (30.0, rows - h - 1.0), (np.nan, 24.0), (30.0, np.inf), (-np.inf, 24.0),
            (3e9, 24.0)]
    st, it, xy = go(tex, tex, [q + (30.25, 24.5) for q in olds], max_iter=0)
    assert st == [0, 5, 0, 5, 0, 5, 0, 5, 5, 5, 5, 5] and not any(it) and (xy == [30.25, 24.5]).all()
    # the known shift (2 right, 1 down): from 0.5 px off the truth every point converges and ends nearer than it started
    dy, dx = 1, 2
    old, new = R.smooth_texture(61, 97, 5), R.smooth_texture(61, 97, 5, shift=(-dy, -dx))
    rng = np.random.default_rng(17)
    for size, min_inc in ((13, 0.04), (5, 5e-7), (17, 0.04)):
        hh = R.half(size)
        pts, off = [], []
        for _ in range(12):
            ox = float(np.round(rng.uniform(hh + 3, 97 - hh - 6) * 4) / 4)
            oy = float(np.round(rng.uniform(hh + 3, 61 - hh - 5) * 4) / 4)
            for sx, sy in ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5), (0.5, -0.5)):
                pts.append((ox, oy, ox + dx + sx, oy + dy + sy))
                off.append((ox + dx, oy + dy, np.hypot(sx, sy)))
        st, it, xy = go(old, new, pts, size, 50, min_inc)
        off = np.array(off)
        assert st == [1] * 60, (size, st)
        assert (np.hypot(xy[:, 0] - off[:, 0], xy[:, 1] - off[:, 1]) < off[:, 2]).all(), size


# ------------------------------------------------------------------------------------------------------------ known answers of the specification itself
TEX = R.smooth_texture(48, 64, 11)
I = R.grey(TEX)


def test_sums_by_accumulate_equal_sums_by_scalar_loop():
    new = R.grey(R.smooth_texture(48, 64, 11, shift=(1, 1)))
    for ps, x, y in ((3, 20.25, 20.5), (13, 30.0, 24.75), (17, 31.5, 24.5), (31, 32.1, 24.9)):
        a = R.align(I, new, x, y, x + 0.5, y - 0.5, ps, 6, 1e-6)
        b = R.align(I, new, x, y, x + 0.5, y - 0.5, ps, 6, 1e-6, scalar=True)
        assert a[0] == b[0] and a[3] == b[3] and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
        assert np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()
        for u, v in zip(a[4], b[4]):
            assert u.tobytes() == v.tobytes()


def test_hessian_order_is_free_up_to_patch_15_only_in_general():
    """gx, gy are multiples of 1/2 below 128: products are multiples of 1/4 below 2^14, and 225 of them stay below 2^24 / 4 --
    every partial sum is exact.  From 17 x 17 on (289 x 2^14 > 2^22) a sum may round, so the order is the reference's."""
    assert 15 * 15 * 127.5 * 127.5 * 4 < 2 ** 24 < 17 * 17 * 127.5 * 127.5 * 4


def test_same_image_from_the_exact_start_converges_in_one_step_unmoved():
    for ps in (3, 5, 13, 17, 31):
        h = R.half(ps)
        x, y = float(h + 9), float(h + 5)
        st, nx, ny, it, m = R.align(I, I, x, y, x, y, ps, 50, 0.04)
        assert (st, nx, ny, it) == (R.CONVERGED, x, y, 1)
        assert m[0].tolist() == I[int(y) - h:int(y) + h + 1, int(x) - h:int(x) + h + 1].astype(np.float64).reshape(-1).tolist()


def test_patch_is_the_bilinear_form_and_gradients_are_halved_differences():
    st, patch, gx, gy, inv = R.model(I, 20.5, 17.25, 3)
    assert st == R.CONVERGED
    k = 4                                                            # the centre: i = 17, j = 20
    want = ((0.5 * 0.75) * I[17, 20] + (0.5 * 0.75) * I[17, 21] + (0.5 * 0.25) * I[18, 20]) + (0.5 * 0.25) * I[18, 21]
    assert patch[k] == want
    assert gx[k] == 0.5 * (I[17, 21] - I[17, 19]) and gy[k] == 0.5 * (I[18, 20] - I[16, 20])
    assert gx.dtype == np.float32 and patch.dtype == np.float64 and inv.dtype == np.float32


def test_colour_uses_the_rgb2gray_weights_with_channel_0_as_red():
    img = np.zeros((2, 3, 3), np.uint8)
    img[0, 0], img[0, 1], img[0, 2], img[1, 0] = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    g = R.grey(img)
    assert g[0].tolist() == [(255 * 4899 + 8192) >> 14, (255 * 9617 + 8192) >> 14, (255 * 1868 + 8192) >> 14] and g[1, 0] == 255


def test_inverse_on_exact_cases():
    assert R.inverse3([[2, 0, 0], [0, 4, 0], [0, 0, 8]]).tolist() == [[0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.125]]
    m = np.float32([[4, 1, 2], [1, 3, 0], [2, 0, 5]])
    assert np.abs(R.inverse3(m).astype(np.float64) @ m - np.eye(3)).max() < 1e-6
    z = R.inverse3(np.zeros((3, 3)))
    assert (z.view(np.uint32) == 0x7FC00000).all()                   # 0 x inf: the one NaN pattern


def test_flat_patch_gives_status_2_and_leaves_the_position():
    flat = np.full((48, 64), 90, np.int32)
    st, x, y, it, m = R.align(flat, I, 20.0, 20.0, 21.25, 19.5, 13, 50, 0.04)
    assert (st, x, y, it) == (R.NAN_HESSIAN, 21.25, 19.5, 0) and np.isnan(m[3]).all()
    assert R.model(flat, 20.0, 20.0, 13)[0] == R.NAN_HESSIAN


def test_max_iter_0_gives_status_0_unmoved():
    assert R.align(I, I, 20.0, 20.0, 21.25, 19.5, 13, 0, 0.04)[:4] == (R.MAX_ITERATIONS, 21.25, 19.5, 0)
    # ... even from a start that no step could have taken
    assert R.align(I, I, 20.0, 20.0, np.nan, -5.0, 13, 0, 0.04)[0] == R.MAX_ITERATIONS


def test_every_status_value_is_reached():
    new = R.grey(R.smooth_texture(48, 64, 11, shift=(0, 1)))
    seen = {
        R.align(I, I, 30.0, 24.0, 30.0, 24.0, 13, 50, 0.04)[0],
        R.align(I, new, 30.0, 24.0, 30.5, 24.0, 13, 1, 0.0)[0],       # no increment is below 0: one step, then the limit
        R.align(np.full_like(I, 5), I, 30.0, 24.0, 30.0, 24.0, 13, 50, 0.04)[0],
        R.align(I, I, 30.0, 24.0, 5.5, 24.0, 13, 50, 0.04)[0],
        R.align(I, I, 30.0, 24.0, 33.0, 24.0, 3, 50, 1e9)[0],         # any first step "converges"; this one is longer than h = 1
        R.align(I, I, 6.5, 24.0, 30.0, 24.0, 13, 50, 0.04)[0],
        R.align(I, I, 30.0, 24.0, 57.5, 24.0, 13, 50, 0.04)[0],
    }
    assert seen == set(range(7)), seen


def test_moved_too_far_is_decided_on_the_squared_distance_from_the_start():
    st, x, y, it, _ = R.align(I, I, 30.0, 24.0, 33.0, 24.0, 3, 50, 1e9)
    assert st == R.MOVED_TOO_FAR and it == 1 and (x - 33.0) ** 2 + (y - 24.0) ** 2 > 1.0


def test_gate_edges():
    """newX == h and == cols - h pass the reference's gate, one ulp beyond either fails it (status 3, no step); the position
    on the right edge passes the gate and fails the tap rule (status 6)"""
    ps, h, rows, cols = 13, 6, 48, 64
    m = R.model(I, 30.0, 24.0, ps)

    def go(x, y):
        return R.optimize(I, m[1], m[2], m[3], m[4], x, y, ps, 1, 0.0)
    assert go(float(h), 20.0)[0] == R.MAX_ITERATIONS and go(float(h), 20.0)[3] == 1        # the step was taken
    assert go(ULP_DOWN(h), 20.0)[::3] == (R.OUT_OF_IMAGE, 0)
    assert go(20.0, float(h))[0] == R.MAX_ITERATIONS and go(20.0, ULP_DOWN(h))[::3] == (R.OUT_OF_IMAGE, 0)
    assert go(float(cols - h), 20.0)[::3] == (R.NEW_TAPS_OUTSIDE, 0) and go(ULP_UP(cols - h), 20.0)[::3] == (R.OUT_OF_IMAGE, 0)
    assert go(20.0, float(rows - h))[::3] == (R.NEW_TAPS_OUTSIDE, 0) and go(20.0, ULP_UP(rows - h))[::3] == (R.OUT_OF_IMAGE, 0)


def test_the_two_divergence_bands():
    ps, h, rows, cols = 13, 6, 48, 64
    m = R.model(I, 30.0, 24.0, ps)
    # new image: the gate admits [cols - h - 1, cols - h]; the taps reach columns cols and cols + 1 there
    for x in (cols - h - 1.0, cols - h - 0.5, float(cols - h)):
        assert R.optimize(I, m[1], m[2], m[3], m[4], x, 20.0, ps, 5, 0.04)[0] == R.NEW_TAPS_OUTSIDE
    assert R.optimize(I, m[1], m[2], m[3], m[4], ULP_DOWN(cols - h - 1.0), 20.0, ps, 1, 0.0)[0] == R.MAX_ITERATIONS
    for y in (rows - h - 1.0, float(rows - h)):
        assert R.optimize(I, m[1], m[2], m[3], m[4], 20.0, y, ps, 5, 0.04)[0] == R.NEW_TAPS_OUTSIDE
    # old image: x in [h + 1, cols - h - 1)
    for x, ok in ((h + 1.0, True), (ULP_DOWN(h + 1.0), False), (ULP_DOWN(cols - h - 1.0), True), (cols - h - 1.0, False), (0.0, False),
                  (-1.0, False)):
        assert (R.model(I, x, 24.0, ps)[0] != R.OLD_TAPS_OUTSIDE) == ok, x
    for y, ok in ((h + 1.0, True), (ULP_DOWN(h + 1.0), False), (ULP_DOWN(rows - h - 1.0), True), (rows - h - 1.0, False)):
        assert (R.model(I, 30.0, y, ps)[0] != R.OLD_TAPS_OUTSIDE) == ok, y
    st, x, y, it, mm = R.align(I, I, 3.0, 24.0, 30.25, 24.5, ps, 50, 0.04)
    assert (st, x, y, it, mm) == (R.OLD_TAPS_OUTSIDE, 30.25, 24.5, 0, None)


def test_non_finite_positions():
    for bad in (np.nan, np.inf, -np.inf):
        assert R.align(I, I, bad, 24.0, 30.0, 24.0, 13, 50, 0.04)[0] == R.OLD_TAPS_OUTSIDE
        assert R.align(I, I, 30.0, bad, 30.0, 24.0, 13, 50, 0.04)[0] == R.OLD_TAPS_OUTSIDE
        for pos in ((bad, 24.0), (30.0, bad)):
            st, x, y, it, _ = R.align(I, I, 30.0, 24.0, pos[0], pos[1], 13, 50, 0.04)
            assert st == R.OUT_OF_IMAGE and it == 0
            assert np.float64(x).tobytes() == np.float64(pos[0]).tobytes() and np.float64(y).tobytes() == np.float64(pos[1]).tobytes()


# -------------------------------------------------------------------------------------------------------------- known shift
def test_known_shift_is_approached_from_half_a_pixel_away():
    """A smooth seeded texture and a copy moved by whole pixels (2 right, 1 down): from starts 0.5 px off the truth on either axis
    every drawn point converges (status 1) and ends nearer the truth than it started.  A condition, not a tolerance."""
    dy, dx = 1, 2
    old = R.grey(R.smooth_texture(61, 97, 5))
    new = R.grey(R.smooth_texture(61, 97, 5, shift=(-dy, -dx)))      # new[y + dy, x + dx] = old[y, x]
    assert (new[10 + dy:50 + dy, 10 + dx:80 + dx] == old[10:50, 10:80]).all()
    rng = np.random.default_rng(17)
    n = 0
    for ps, min_inc in ((13, 0.04), (5, 5e-7), (17, 0.04)):
        h = R.half(ps)
        for _ in range(12):
            ox, oy = rng.uniform(h + 3, 97 - h - 6), rng.uniform(h + 3, 61 - h - 5)
            ox, oy = float(np.round(ox * 4) / 4), float(np.round(oy * 4) / 4)
            tx, ty = ox + dx, oy + dy
            for sx, sy in ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5), (0.5, -0.5)):
                st, x, y, it, _ = R.align(old, new, ox, oy, tx + sx, ty + sy, ps, 50, min_inc)
                assert st == R.CONVERGED, (ps, ox, oy, sx, sy, st, it)
                assert np.hypot(x - tx, y - ty) < np.hypot(sx, sy), (ps, ox, oy, sx, sy, x - tx, y - ty)
                n += 1
    assert n == 180
