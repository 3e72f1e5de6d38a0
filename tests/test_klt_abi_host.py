"""The tracker's part of the C ABI without a GPU: the ctypes mirrors of PsKltParams / PsImageSet have the library's sizes, every
entry point rejects a NULL context, and the parameter helper carries the shipped OpenCVParams."""
import ctypes as C


def test_klt_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_klt()
    assert set(sizes) == {"klt_params", "image_set"}
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size, name
    assert sizes["klt_params"] == 32 and sizes["image_set"] == 40
    assert L.ps_abi_version() == 2


def test_klt_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsImageSet, klt_params
    L = _lib.load()
    p, h, k = klt_params(), C.c_void_p(), C.c_int(7)
    assert (p.winSize, p.maxLevels, p.maxCount, p.eps, p.flags, p.minEigThreshold) == (7, 3, 30, 0.01, 0, 1e-4)
    assert L.ps_klt_pyramids_create(None, 48, 64, 1, 7, 3, 2, C.byref(h)) == -1 and not h.value
    assert L.ps_klt_pyramids_build_device(None, None, C.byref(PsImageSet()), 0) == -1
    assert L.ps_klt_track_device(None, None, C.byref(p), None, None, None, 1, 1, None, None, None) == -1
    assert L.ps_klt_select_device(None, None, None, None, None, 1, 1, 1.0, 1.0, None, None, None, None) == -1
    assert L.ps_calc_optical_flow_pyr_lk(None, None, None, 48, 64, 1, 0, None, None, 0, None, None, C.byref(p)) == -1
    assert L.ps_perform_tracking(None, None, None, 48, 64, 1, 0, None, None, 0, C.byref(p), 1.0, 1.0, None, None, None, C.byref(k), None,
                                 None) == -1 and k.value == 7
    assert L.ps_debug_klt_level(None, None, 0, 0, None, None, None) == -1
    assert L.ps_klt_pyramids_num_levels(None) == -1
    L.ps_klt_pyramids_destroy(None)   # (harmless)
