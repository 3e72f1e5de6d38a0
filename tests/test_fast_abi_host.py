"""The detector's part of the C ABI without a GPU: the ctypes mirror of PsDetectParams has the library's size, every entry point
rejects a NULL context and leaves its outputs alone, and the parameter helper carries the shipped values."""
import ctypes as C


def test_detect_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_detect()
    assert set(sizes) == {"detect_params"}
    assert L.ps_abi_sizeof_detect_params() == sizes["detect_params"] == 24
    assert L.ps_abi_version() == 2


def test_detect_params_carry_the_shipped_values():
    from putslam_amd._abi import detect_params
    p = detect_params()
    assert (p.threshold, p.nonmaxSuppression, p.gridRows, p.gridCols, p.maximalTrackedFeatures, p.reserved) == (10, 1, 1, 1, 500, 0)
    q = detect_params(40, False, 2, 3, 77)
    assert (q.threshold, q.nonmaxSuppression, q.gridRows, q.gridCols, q.maximalTrackedFeatures, q.reserved) == (40, 0, 2, 3, 77, 0)


def test_detect_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsImageSet, detect_params
    L = _lib.load()
    p, h, n = detect_params(), C.c_void_p(0x1234), C.c_int(7)
    assert L.ps_fast_detector_create(None, 48, 64, 1, 2, C.byref(h)) == -1 and h.value == 0x1234
    assert L.ps_detect_features_device(None, None, C.byref(PsImageSet()), C.byref(p), 500, None, None, None) == -1
    assert L.ps_debug_fast_passes(None, None, C.byref(PsImageSet()), C.byref(p), 500, None, None, None, 7) == -1
    xy, resp = (C.c_float * 2)(5.0, 6.0), (C.c_float * 1)(7.0)
    assert L.ps_detect_features(None, None, 48, 64, 1, 0, C.byref(p), xy, resp, 1, C.byref(n)) == -1
    assert n.value == 7 and list(xy) == [5.0, 6.0] and list(resp) == [7.0]
    g = (C.c_uint8 * 4)(1, 2, 3, 4)
    assert L.ps_debug_fast_maps(None, None, 0, g, None, None) == -1 and list(g) == [1, 2, 3, 4]
    L.ps_fast_detector_destroy(None)   # (harmless)
