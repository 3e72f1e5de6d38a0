"""The float-descriptor map matching's definition (tests/map_l2_ref.py) checked on the host: the order of its double sum on a
directed row, how often that order matters on random rows, the whole rule against a float64 brute force; and the library's new
symbols and struct size, which need no device."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_l2_ref as ref  # noqa: E402

from putslam_amd import synth  # noqa: E402

f32 = np.float32


def directed_row():
    """[1, 2^-12, 2^-12, 2^-24, 2^-27 x 16], D = 20; the squares are 1, 2^-24, 2^-24, 2^-48 and sixteen times 2^-54.
    Blocks of four: the first block is 1 + 2^-23 + 2^-48, every addition exact in double; each later block is 4 x 2^-54 = 2^-52,
    one ulp of a double near 1, and is kept: s = 1 + 2^-23 + 2^-48 + 2^-50.  Its root lies above 1 + 2^-24, the middle between the
    floats 1 and 1 + 2^-23, and narrows to 1 + 2^-23.
    One element at a time: each 2^-54 is a quarter ulp and is lost, s = 1 + 2^-23 + 2^-48, whose root is 1 + 2^-24 to the last
    place of a double: the tie narrows to the even float, 1.  A float sum loses 2^-24 at once: 1."""
    return np.array([1.0, 2.0 ** -12, 2.0 ** -12, 2.0 ** -24] + [2.0 ** -27] * 16, f32)


def test_the_block_order_on_a_directed_row():
    a, z = directed_row(), np.zeros(20, f32)
    assert a.dtype == f32 and float(a[3]) == 2.0 ** -24 and float(a[4]) == 2.0 ** -27    # (all entries are float32 values)
    restated = ref.l2_value(a[None, :], z[None, :])[0]
    assert restated.dtype == f32
    assert float(restated).hex() == "0x1.0000020000000p+0", float(restated).hex()
    assert restated.view(np.uint32) == 0x3F800001
    assert float(ref.value_sequential_f64(a, z)).hex() == "0x1.0000000000000p+0"
    assert float(ref.value_f32(a, z)).hex() == "0x1.0000000000000p+0"
    # the same row as map and as frame side, and negated: the value is that of the difference
    assert ref.l2_value(z[None, :], a[None, :])[0].view(np.uint32) == 0x3F800001
    assert ref.l2_value((-a)[None, :], z[None, :])[0].view(np.uint32) == 0x3F800001


def test_accumulation_order_matters_on_random_surf_rows():
    """On random SURF rows the restated value (double accumulation) differs from a float accumulation on
    about half of the pairs (100 554 of 200 000 measured).  The SIFT rows of synth are small integers: every sum of squares
    is an integer below 2^24, every order agrees on them -- so SIFT scenes catch no accumulation error, SURF scenes do."""
    rng = np.random.default_rng(20261019)
    n = 200000
    a, b = synth.float_rows(rng, n, "surf"), synth.float_rows(rng, n, "surf")
    restated = ref.l2_value(a, b)
    in_float = ref.values_f32(a, b)
    differ = int((restated.view(np.uint32) != in_float.view(np.uint32)).sum())
    print("restated != float accumulation on %d of %d SURF pairs" % (differ, n))
    assert differ >= n // 4
    m = 20000
    a, b = synth.float_rows(rng, m, "sift"), synth.float_rows(rng, m, "sift")
    assert ref.l2_value(a, b).tobytes() == ref.values_f32(a, b).tobytes()
    assert float(ref.l2_sumsq(a, b).max()) < 2.0 ** 24


def _scene(kind, n=200, seed=5):
    rng = np.random.default_rng(seed)

    class Levels:                     # (make_frames asks its oracle for predicted levels only)
        @staticmethod
        def predicted_level(octave, det, cur):
            return int(np.clip(np.ceil(np.log(1.2 ** octave * det / cur) / np.log(1.2)), 0, 7))

    frames = ref.make_frames(rng, Levels, [n], n, kind)
    views = ref.make_views(rng, frames, [n], n, [0], kind, sigma=0.05)
    return views, frames


def test_the_rule_against_a_float64_brute_force():
    """Well separated: no candidate lies within 1e-6 of the sphere, no value within 1e-6 (relative) of the ratio line."""
    for kind, radius, ratio in (("surf", 0.12, 0.55), ("sift", 0.30, 0.10), ("surf", 0.30, 0.10)):
        views, frames = _scene(kind)
        args = (views["pos"][0], views["desc"][0], views["level"][0], frames["pos"][0], frames["desc"][0], frames["level"][0])
        got, counts = ref.match_xyz_l2(*args, radius, ratio, return_counts=True)
        want = ref.match_xyz_l2_f64(*args, radius, ratio)
        assert len(got) == len(want) and len(got) > 50, (kind, len(got), len(want))
        assert [(int(m["queryIdx"]), int(m["trainIdx"])) for m in got] == [(j, i) for j, i, _ in want]
        assert np.allclose(got["distance"], [v for _, _, v in want], rtol=1e-6, atol=0)
        assert (got["imgIdx"] == -1).all()
        assert counts.sum() >= len(got) and counts.max() >= 2


def test_best_value_rule_with_nan_and_inf():
    """:714-727 on hand-made candidate lists: a NaN first value emits nothing, a later NaN is ignored, +inf is ordinary,
    ratio 0 drops +inf candidates and keeps finite ones."""
    nan, inf = f32(np.nan), f32(np.inf)
    jj = np.zeros(3, np.int64)
    ii = np.arange(3)
    keep = lambda v, r: ref.select(jj[:len(v)], ii[:len(v)], np.array(v, f32), r).tolist()   # noqa: E731
    assert keep([nan, 1.0, 2.0], 0.55) == [False, False, False]
    assert keep([1.0, nan, 1.5], 0.55) == [True, False, True]
    assert keep([inf], 0.55) == [True]
    assert keep([inf, 3.0, inf], 0.55) == [False, True, False]
    assert keep([inf, 3.0, 0.0], 0.0) == [False, True, True]
    assert keep([0.0, 0.0], 0.55) == [True, True]
    assert keep([4.0, 2.0, 8.0], 0.5) == [True, True, False]          # ratio x value == best exactly
    # a float difference that overflows becomes +inf
    big = np.full((1, 4), 3e38, f32)
    assert ref.l2_value(big, -big)[0] == inf


def test_the_library_exports_the_float_map_calls():
    from putslam_amd import _abi, _lib
    L = _lib.load()
    for name in ("ps_match_xyz_l2_f32", "ps_match_xyz_l2_device", "ps_map_pairs_l2_device", "ps_abi_sizeof_map_batch_f32"):
        assert hasattr(L, name), name
    assert L.ps_abi_sizeof_map_batch_f32() == C.sizeof(_abi.PsMapBatchF32)
    assert C.sizeof(_abi.PsMapBatchF32) == 2 * C.sizeof(_abi.PsFrameSetF32) + 64
    assert L.ps_abi_version() == 2
    b = _abi.PsMapBatchF32()
    b.maps.dim, b.frames.dim, b.maxMatches, b.acceptRatio = 64, 64, 7, 0.55
    assert (b.maps.dim, b.frames.dim, b.maxMatches, b.acceptRatio) == (64, 64, 7, 0.55)
