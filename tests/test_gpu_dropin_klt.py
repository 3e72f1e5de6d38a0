"""FrameMatcherHIP::performTracking (MatcherOpenCV::performTracking, matcherOpenCV.cpp:209-300) on cv::Mat-shaped inputs:
tests/cpp/test_dropin_klt compares its matches and the erased features / keyPoints / detDists with the C ABI's results and with
the reference's selection loop restated in C++, as bytes."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_klt")


def test_cpp_dropin_perform_tracking():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 5
