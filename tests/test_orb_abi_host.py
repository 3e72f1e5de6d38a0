"""The descriptor extractor's part of the C ABI without a GPU: the ctypes mirror of PsOrbParams has the library's size, the
parameter helper carries the shipped values, every entry point rejects a NULL context and leaves its outputs alone, and the
library's default pattern is the restatement's."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_ref as R  # noqa: E402


def test_orb_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_orb()
    assert set(sizes) == {"orb_params"}
    assert L.ps_abi_sizeof_orb_params() == sizes["orb_params"] == 16
    assert L.ps_abi_version() == 2


def test_orb_params_carry_the_shipped_values():
    from putslam_amd._abi import orb_params
    p = orb_params()
    assert (p.scaleFactor, p.nLevels, list(p.reserved)) == (float(np.float32(1.2)), 8, [0, 0])
    q = orb_params(1.5, 6)
    assert (q.scaleFactor, q.nLevels, list(q.reserved)) == (1.5, 6, [0, 0])


def test_orb_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsImageSet, orb_params
    L = _lib.load()
    p, h, n = orb_params(), C.c_void_p(0x1234), C.c_int(7)
    assert L.ps_orb_pyramids_create(None, 80, 96, 1, C.byref(p), None, 2, C.byref(h)) == -1 and h.value == 0x1234
    assert L.ps_orb_pyramids_build_device(None, None, C.byref(PsImageSet()), 0) == -1
    assert L.ps_describe_features_device(None, None, None, None, None, None, None, 1, 4, None, None, None) == -1
    assert L.ps_debug_orb_passes(None, None, C.byref(PsImageSet()), 0, None, None, None, None, None, 1, 4, None, None, None, 31) == -1
    img = np.zeros((80, 96), np.uint8)
    xy, ang, octv = np.full((1, 2), 40, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    desc, kept = np.full((1, 32), 0xA5, np.uint8), np.full(1, 77, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.ps_describe_features(None, vp(img), 80, 96, 1, 0, C.byref(p), None, vp(xy), vp(ang), vp(octv), 1, vp(desc), vp(kept),
                                  C.byref(n)) == -1
    assert n.value == 7 and (desc == 0xA5).all() and kept[0] == 77
    g = (C.c_uint8 * 4)(1, 2, 3, 4)
    assert L.ps_debug_orb_level(None, None, 0, 0, g, g) == -1 and list(g) == [1, 2, 3, 4]
    dims, scale = (C.c_int32 * 2)(5, 6), C.c_float(9.0)
    assert L.ps_orb_pyramids_level(None, 0, dims, C.byref(scale)) == -1 and list(dims) == [5, 6] and scale.value == 9.0
    L.ps_orb_pyramids_destroy(None)   # (harmless)


def test_default_pattern_is_the_restatements():
    from putslam_amd import _lib
    L = _lib.load()
    out = np.zeros(1024, np.int8)
    assert L.ps_orb_pattern_default(out.ctypes.data_as(C.c_void_p)) == 0
    assert out.tobytes() == R.default_pattern().tobytes()
    assert L.ps_orb_pattern_default(None) == -1
