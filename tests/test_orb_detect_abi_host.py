"""The ORB detector's part of the C ABI without a GPU: the ctypes mirror of PsOrbDetectParams has the library's size, every entry
point rejects a NULL context and leaves its outputs alone, the parameter helper carries the shipped values, and the library's own
quotas (pure host arithmetic) are the restatement's."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_orb_detect_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_orb_detect()
    assert set(sizes) == {"orb_detect_params"}
    assert L.ps_abi_sizeof_orb_detect_params() == sizes["orb_detect_params"] == 32
    assert L.ps_abi_version() == 2


def test_orb_detect_params_carry_the_shipped_values():
    from putslam_amd._abi import orb_detect_params
    p = orb_detect_params()
    assert (p.nFeatures, p.nLevels, p.fastThreshold, p.gridRows, p.gridCols, p.maximalTrackedFeatures, p.reserved) == (500, 8, 20, 1, 1, 500, 0)
    assert np.float32(p.scaleFactor) == np.float32(1.2)
    q = orb_detect_params(40, 1.5, 3, 7, 2, 3, 77)
    assert (q.nFeatures, q.nLevels, q.fastThreshold, q.gridRows, q.gridCols, q.maximalTrackedFeatures, q.reserved) == (40, 3, 7, 2, 3, 77, 0)
    assert np.float32(q.scaleFactor) == np.float32(1.5)


def test_orb_detect_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsImageSet, orb_detect_params
    L = _lib.load()
    p, h, n = orb_detect_params(), C.c_void_p(0x1234), C.c_int(7)
    assert L.ps_orb_detector_create(None, 96, 128, 1, C.byref(p), 2, C.byref(h)) == -1 and h.value == 0x1234
    assert L.ps_orb_detect_frames(None, None, C.byref(PsImageSet()), C.byref(p), 500, None, None, None, None, None) == -1
    assert L.ps_debug_orb_detect_passes(None, None, C.byref(PsImageSet()), C.byref(p), 500, None, None, None, None, None, 63) == -1
    xy, resp, ang, octv = (C.c_float * 2)(5.0, 6.0), (C.c_float * 1)(7.0), (C.c_float * 1)(8.0), (C.c_int32 * 1)(9)
    assert L.ps_detect_features_orb(None, None, 96, 128, 1, 0, C.byref(p), xy, resp, ang, octv, 1, C.byref(n)) == -1
    assert n.value == 7 and list(xy) == [5.0, 6.0] and list(resp) == [7.0] and list(ang) == [8.0] and list(octv) == [9]
    g, m = (C.c_uint8 * 4)(1, 2, 3, 4), C.c_int32(-3)
    assert L.ps_debug_orb_detect_level(None, None, 0, 0, g, None, C.byref(m), None, None, None, None, 0) == -1
    assert list(g) == [1, 2, 3, 4] and m.value == -3
    d = (C.c_int32 * 2)(11, 12)
    assert L.ps_orb_detector_level(None, 0, d, None) == -1 and list(d) == [11, 12]
    L.ps_orb_detector_destroy(None)   # (harmless)


def test_library_quotas_are_the_restatements():
    import orb_detect_ref as D
    from putslam_amd import _lib
    from putslam_amd._abi import orb_detect_params
    L = _lib.load()
    for nf, sf, nl in [(500, 1.2, 8), (500, 1.2, 3), (40, 1.2, 4), (0, 1.2, 8), (1, 1.2, 8), (12, 1.2, 3), (24, 1.5, 3), (7, 2.0, 8), (16384, 1.01, 8),
                       (33, 1.2, 1)]:
        q = (C.c_int32 * 8)(*([-1] * 8))
        assert L.ps_orb_detect_quotas(C.byref(orb_detect_params(nf, sf, nl)), q) == 0
        assert list(q) == D.quotas(nf, sf, nl) + [0] * (8 - nl), (nf, sf, nl)
    q = (C.c_int32 * 8)(*([-1] * 8))
    assert L.ps_orb_detect_quotas(None, q) == -1 and L.ps_orb_detect_quotas(C.byref(orb_detect_params(n_levels=9)), q) == -1
    assert L.ps_orb_detect_quotas(C.byref(orb_detect_params()), None) == -1 and list(q) == [-1] * 8
