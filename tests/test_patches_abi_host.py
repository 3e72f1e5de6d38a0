"""The matching on patches' part of the C ABI without a GPU: the ctypes mirrors of PsPatchParams / PsPatchModel have the library's
sizes, the new names are declared, exported and bound, every entry point rejects a NULL context, the parameter helper carries the
shipped PatchesParams, and the pure rules (ps_patches_rule.h) pass their stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["ps_patch_models", "ps_patch_align", "ps_compute_patch", "ps_compute_patch_gradient", "ps_optimize_location",
             "ps_optimize_locations", "ps_abi_sizeof_patch_params", "ps_abi_sizeof_patch_model"]


def test_patch_struct_layout_matches_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_patches()
    assert set(sizes) == {"patch_params", "patch_model"}
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size, name
    assert sizes["patch_params"] == 24 and sizes["patch_model"] == 32


def test_new_names_are_declared_exported_and_bound_and_none_is_a_device_suffix_name():
    from putslam_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "putslam_hip.h")).read()
    lo, hi = header.index("/* ---- Sub-pixel matching on patches"), header.index("/* ---- Measurement uncertainty")
    declared = sorted(set(re.findall(r"\b(ps_\w+)\(", re.sub(r"/\*.*?\*/", " ", header[lo:hi], flags=re.S))))
    assert declared == sorted(NEW_NAMES)
    for n in NEW_NAMES:
        assert hasattr(L, n) and n in _lib.EXPORTED and not n.endswith("_device"), n


def test_status_values_and_defaults():
    from putslam_amd import _abi
    p = _abi.patch_params()
    assert (p.patchSize, p.maxIter, p.minSqrtIncrement, p.flags, p.reserved) == (13, 50, 0.04, 0, 0)   # the shipped matcher XMLs
    assert [_abi.PATCH_MAX_ITERATIONS, _abi.PATCH_CONVERGED, _abi.PATCH_NAN_HESSIAN, _abi.PATCH_OUT_OF_IMAGE, _abi.PATCH_MOVED_TOO_FAR,
            _abi.PATCH_OLD_TAPS_OUTSIDE, _abi.PATCH_NEW_TAPS_OUTSIDE] == list(range(7)) and _abi.PATCH_GIVEN_MODEL == 1
    header = open(os.path.join(ROOT, "include", "putslam_hip.h")).read()
    for name, value in (("MAX_ITERATIONS", 0), ("CONVERGED", 1), ("NAN_HESSIAN", 2), ("OUT_OF_IMAGE", 3), ("MOVED_TOO_FAR", 4),
                        ("OLD_TAPS_OUTSIDE", 5), ("NEW_TAPS_OUTSIDE", 6), ("GIVEN_MODEL", 1)):
        assert re.search(r"PS_PATCH_%s = %d\b" % (name, value), header), name


def test_patch_entry_points_reject_a_null_context():
    from putslam_amd import _lib
    from putslam_amd._abi import PsImageSet, PsPatchModel, patch_params
    L = _lib.load()
    p, s, m = patch_params(), PsImageSet(), PsPatchModel()
    st = (C.c_uint8 * 4)(7, 7, 7, 7)
    assert L.ps_patch_models(None, C.byref(s), None, None, None, 1, 1, C.byref(p), C.byref(m), st) == -1
    assert L.ps_patch_align(None, C.byref(s), None, None, None, None, 1, 1, C.byref(p), C.byref(m), st, None) == -1
    assert L.ps_patch_models(None, None, None, None, None, 0, 0, None, None, None) == -1
    assert L.ps_patch_align(None, None, None, None, None, None, 0, 0, None, None, None, None) == -1
    assert L.ps_compute_patch(None, None, 48, 64, 1, 0, None, 0, C.byref(p), None, st) == -1
    assert L.ps_compute_patch_gradient(None, None, 48, 64, 1, 0, None, 0, C.byref(p), None, None, None, st) == -1
    assert L.ps_optimize_location(None, None, None, None, 48, 64, 1, 0, None, 0, None, None, None, C.byref(p), st, None) == -1
    assert L.ps_optimize_locations(None, None, None, 48, 64, 1, 0, None, None, 0, C.byref(p), st, None) == -1
    assert list(st) == [7, 7, 7, 7]


def test_pure_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_patches_rule.cpp: the parameter rule, the sizes, the tap rules and the gate at their edges and the
    image-set rule in a stand-alone program built with -fsanitize=address,undefined, on the CPU"""
    exe = str(tmp_path / "test_patches_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "putslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_patches_rule.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("patches rule ok"), run.stdout


def test_rule_header_agrees_with_the_specification_on_drawn_positions(tmp_path):
    """ps_patches_rule.h decides the old image's tap rule on the doubles, patches_ref.py on the truncated integers: drawn
    positions, the edges, one ulp either side of them and the non-finite values go through tests/cpp/test_patches_rule.cpp
    (`test_patches_rule <file>` prints the header's three decisions per position) and must agree with patches_ref's."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import patches_ref as R
    exe = str(tmp_path / "test_patches_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_patches_rule.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    rows_, cols_ = 61, 64
    recs = []
    for ps in (3, 13, 31):
        h = R.half(ps)
        edges = [h, h + 1, cols_ - h - 1, cols_ - h, rows_ - h - 1, rows_ - h, 0]
        xs = list(rng.uniform(-3, 70, 150)) + [float(e) for e in edges] + [R.ulp_up(e) for e in edges] + [R.ulp_down(e) for e in edges]
        xs += [np.nan, np.inf, -np.inf, 3e9, -3e9, 1e300]
        for x in xs:
            recs.append((x, 30.0, h, rows_, cols_))
            recs.append((30.0 if 30.0 < cols_ - h - 1 else h + 1.0, x, h, rows_, cols_))
    path = str(tmp_path / "positions.bin")
    np.array(recs, np.float64).tofile(path)
    out = subprocess.check_output([exe, path], text=True).split()
    assert len(out) == len(recs)
    for (x, y, h, r, c), got in zip(recs, out):
        h, r, c = int(h), int(r), int(c)
        gate = R.gate_out(x, y, h, r, c)
        want = "%d%d%d" % (R.old_taps_inside(x, y, h, r, c), gate, (not gate) and R.new_taps_inside(x, y, h, r, c))
        assert got == want, (x, y, h, got, want)


def test_dropin_patches_params_are_the_shipped_ones():
    """FrameMatcherHIP's MatcherParameters::PatchesParams and the class's getters, without a GPU"""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_hip()
    g.build_dropin()
    got = json.loads(subprocess.check_output([os.path.join(ROOT, "tests", "cpp", "test_dropin_patches"), "--defaults"], text=True))
    assert got == dict(verbose=0, warping=0, patchSize=13, halfPatchSize=6, maxIter=50, minSqrtIncrement=0.04, getPatchSize=13,
                       getHalfPatchSize=6, ctorPatchSize=9, ctorHalfPatchSize=4)
