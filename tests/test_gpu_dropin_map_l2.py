"""FrameMatcher::matchXYZ / matchXYZLadder route CV_32F descriptor Mats to the float map calls (ps_match_xyz_l2_f32 /
ps_map_pairs_l2_device) and CV_8U Mats to the Hamming path as before: tests/cpp/test_dropin_map_l2 compares the former with the
loop through the C ABI, checks a CV_8U call before and after and the mixed-type refusals, and writes its scenes and inliers to a
file; every inlier it reports must be a record of the Python restatement's match list (tests/map_l2_ref.py) for that try."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_l2_ref as lref  # noqa: E402

from putslam_amd._abi import DMATCH_DTYPE  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_map_l2")


def _take(buf, off, dtype, n):
    a = np.frombuffer(buf, dtype, n, off)
    return a, off + a.nbytes


def test_cpp_dropin_float_map_matching(tmp_path):
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    path = str(tmp_path / "scenes.bin")
    r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 3
    assert r.stderr.count("differ in type or width") == 18          # one line per refused call
    buf, off = open(path, "rb").read(), 0
    for want_d in (64, 128, 20):
        (D, nmap, ncur, used), off = _take(buf, off, np.int32, 4)
        assert D == want_d and 1 <= used <= 10
        mp, off = _take(buf, off, np.float32, nmap * 3)
        md, off = _take(buf, off, np.float32, nmap * D)
        ml, off = _take(buf, off, np.int32, nmap)
        cp, off = _take(buf, off, np.float32, ncur * 3)
        cd, off = _take(buf, off, np.float32, ncur * D)
        cl, off = _take(buf, off, np.int32, ncur)
        for _ in range(2):                 # matchXYZ at try 1, matchXYZLadder at the try it took
            (radius, ratio), off = _take(buf, off, np.float64, 2)
            (n,), off = _take(buf, off, np.int32, 1)
            inl, off = _take(buf, off, DMATCH_DTYPE, int(n))
            full = lref.match_xyz_l2(mp.reshape(-1, 3), md.reshape(-1, D), ml, cp.reshape(-1, 3), cd.reshape(-1, D), cl, float(radius),
                                     float(ratio))
            records = {m.tobytes() for m in full}
            assert len(inl) <= len(full) and all(m.tobytes() in records for m in inl), (D, radius, ratio)
            order = [(int(m["queryIdx"]), int(m["trainIdx"])) for m in inl]
            assert order == sorted(order)
        assert n > 0             # (the try the ladder took has inliers)
    assert off == len(buf)
