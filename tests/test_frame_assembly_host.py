"""Frame assembly's part of the C ABI and its reference chain without a GPU: the ctypes mirrors have the library's sizes, the new
names are declared, exported and bound and none of them ends in _device (the stream-order table of tests/stream_order_cases.py stays
the set of ps_*_device names), every entry point rejects a NULL context and leaves its outputs alone, the depth set's stride rule
(tests/cpp/test_depth_rule.cpp) holds, and the scene of tests/frame_assembly_ref.py is one in which every step has work to do."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

NEW_NAMES = ["ps_gather_keypoints", "ps_assemble_frames", "ps_front_end_create", "ps_front_end_destroy", "ps_front_end_frames",
             "ps_front_end_frame", "ps_abi_sizeof_depth_set", "ps_abi_sizeof_frame_geometry", "ps_abi_sizeof_frame_rows_out",
             "ps_abi_sizeof_front_end_params"]


def test_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_frame_assembly()
    assert sizes == {"depth_set": 40, "frame_geometry": 88, "frame_rows_out": 96, "front_end_params": 56}
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size, name
    assert L.ps_abi_version() == 2


def test_new_names_are_declared_exported_and_bound_and_none_is_a_device_name():
    from putslam_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "putslam_hip.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED, name
        fn = getattr(L, name)
        assert fn.argtypes is not None or name.startswith("ps_abi_sizeof_"), name
        assert not re.fullmatch(r"ps_\w+_device", name), name
    # what the header declares between the ORB detector's section and the loop-closure section is this list and no other name
    lo, hi = header.index("---- Frame assembly"), header.index("---- Loop-closure candidates")
    assert sorted(set(re.findall(r"\b(ps_\w+)\(", header[lo:hi])) - {"ps_depth_view_bytes"}) == sorted(NEW_NAMES)


def test_parameter_helpers():
    from putslam_amd._abi import frame_geometry, front_end_params, orb_detect_params, orb_params
    p = front_end_params()
    assert (p.detect.nFeatures, p.detect.nLevels, p.detect.maximalTrackedFeatures, p.describe.nLevels) == (500, 8, 500, 8)
    assert np.float32(p.detect.scaleFactor) == np.float32(p.describe.scaleFactor) == np.float32(1.2) and p.DBScanEps == 10.0
    q = front_end_params(orb_detect_params(80, 1.5, 4, 7, 1, 2, 64), orb_params(1.5, 2), 3.0)
    assert (q.detect.gridCols, q.detect.maximalTrackedFeatures, q.describe.nLevels, q.DBScanEps) == (2, 64, 2, 3.0)
    g = frame_geometry(np.arange(9), (1, 2, 3, 4, 5), 1000.0)
    assert list(g.K) == list(range(9)) and list(g.dist5) == [1, 2, 3, 4, 5] and g.depthImageScale == 1000.0


def test_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsDepthSet, PsFrameRowsOut, PsImageSet, frame_geometry, front_end_params
    L = _lib.load()
    g, p, ds, out = frame_geometry(np.eye(3).ravel()), front_end_params(), PsDepthSet(), PsFrameRowsOut()
    h, n = C.c_void_p(0x1234), C.c_int(7)
    assert L.ps_front_end_create(None, 150, 200, 1, C.byref(p), None, 1, C.byref(h)) == -1 and h.value == 0x1234
    assert L.ps_gather_keypoints(None, None, None, 1, 8, None, None, None, None, None, None, None, None, None) == -1
    assert L.ps_assemble_frames(None, C.byref(g), C.byref(ds), 0, None, None, None, 1, 8, C.byref(out)) == -1
    assert L.ps_front_end_frames(None, None, C.byref(PsImageSet()), C.byref(ds), C.byref(g), 8, None, C.byref(out)) == -1
    desc = (C.c_uint8 * 32)(*([9] * 32))
    assert L.ps_front_end_frame(None, None, None, 150, 200, 1, 0, 0, C.byref(p), None, C.byref(g), desc, C.byref(out), 1, C.byref(n)) == -1
    assert n.value == 7 and list(desc) == [9] * 32
    L.ps_front_end_destroy(None)   # (harmless)


def test_depth_rule_program(tmp_path):
    exe = str(tmp_path / "test_depth_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_depth_rule.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "depth rule ok", run.stdout


def test_depth_view_bytes_is_the_librarys():
    from putslam_amd import _lib
    f = _lib.load().ps_depth_view_bytes
    assert f(150, 200, 410) == 149 * 410 + 400 and f(150, 200, 398) == 0


# (detected, thinned, described) per frame: grey and colour, each case of the reference chain
SCENE_COUNTS = {
    (1, "grid1x1"): [(94, 46, 34), (94, 49, 33), (94, 69, 51), (0, 0, 0)],
    (1, "grid1x2"): [(86, 45, 35), (86, 48, 33), (86, 63, 54), (0, 0, 0)],
    (3, "grid1x1"): [(94, 51, 36), (94, 46, 34), (94, 67, 51), (0, 0, 0)],
    (3, "grid1x2"): [(86, 49, 37), (86, 50, 37), (86, 62, 50), (0, 0, 0)],
}


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


@pytest.mark.parametrize("cn", [1, 3])
def test_every_step_of_the_scene_has_work_to_do(oracle, cn):
    """In three frames DBScan removes some key points and not all, describe drops some of the rest and not all and returns them in
    another order than it took them, and some described key points have no depth; the fourth frame yields nothing.  The oracle's
    match and RANSAC accept the pair (0, 1) and no other."""
    import frame_assembly_ref as A
    from putslam_amd._abi import EST_RANSAC, default_ransac_params, make_config
    for name, p, levels in A.CASES:
        frames, counts = A.chain(oracle, A.images(cn), A.depths(), p, levels)
        assert counts == SCENE_COUNTS[cn, name], (cn, name, counts)
        for f, (det, thin, desc) in enumerate(counts[:3]):
            assert A.CAPACITY >= det > thin > desc > 0, (name, f)
        reordered = [bool((np.diff(fr["src_idx"]) < 0).any()) for fr in frames]
        assert sum(reordered) >= 2, (name, reordered)
        missing = [int((fr["pts"][:, 2] == 0).sum()) for fr in frames[:3]]
        assert all(0 < m < len(fr["pts"]) for m, fr in zip(missing, frames)), (name, missing)
        assert all((fr["det_dist"][fr["pts"][:, 2] == 0] == 0).all() and (fr["det_dist"][fr["pts"][:, 2] > 0] > 0).all() for fr in frames)
        moved = [np.abs(fr["xy"] - fr["xy_undist"]).max() for fr in frames[:3]]
        assert min(moved) > 0.01, (name, moved)     # the distortion coefficients move the points
        desc, pts, n = A.frame_set(frames, A.CAPACITY)
        cfg, _ = make_config(EST_RANSAC, 487, 1)
        res = oracle.vo_pairs(default_ransac_params(0), cfg, A.K, desc, pts, n, np.array([[0, 1], [1, 2], [2, 3]], np.int32))
        assert res["stats"]["accepted"].tolist() == [1, 0, 0] and res["numMatches"][0] >= 15 and res["numMatches"][2] == 0, (name, res["stats"])


def test_det_dist_is_the_float_statement():
    """Float products and sums left to right, the float root: not the double root of the double sum, rounded."""
    import frame_assembly_ref as A
    rng = np.random.RandomState(3)
    pts = (rng.rand(4000, 3) * 4).astype(np.float32)
    got = A.det_dist(pts)
    assert got.dtype == np.float64 and (got == got.astype(np.float32)).all()
    other = np.sqrt((pts.astype(np.float64) ** 2).sum(axis=1))
    assert (got != other.astype(np.float32)).any() and np.abs(got - other).max() < 1e-6
