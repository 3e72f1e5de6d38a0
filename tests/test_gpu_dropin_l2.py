"""FrameMatcherHIP::performMatching routes CV_32F descriptor Mats to the float matcher (putslam_hip::l2CrossCheckMatch) and CV_8U
Mats to the Hamming matcher as before: tests/cpp/test_dropin_l2 compares the former with a sequential C++ restatement of the
semantics and the latter with ps_match_hamming256, as bytes."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_l2")


def test_cpp_dropin_float_and_binary_mats():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 4
