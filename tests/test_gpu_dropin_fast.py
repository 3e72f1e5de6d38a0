"""FrameMatcherHIP::detectFeatures (MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180, detector "FAST") on cv::Mat-shaped
images: tests/cpp/test_dropin_fast compares its key points -- all six fields -- with the C ABI's results on the same bytes and with
the reference's grid loop restated in C++ with std::stable_sort; another detector is refused, not run on the CPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_fast")


def test_cpp_dropin_detect_features():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 6
    assert 'detector "FAST" only' in r.stderr        # the refusal is loud
