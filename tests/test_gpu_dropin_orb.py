"""FrameMatcherHIP::describeFeatures (MatcherOpenCV::describeFeatures, matcherOpenCV.cpp:183-195, descriptor "ORB") on cv::Mat-shaped
images: tests/cpp/test_dropin_orb compares its rows and the key points it leaves in the caller's list -- all six fields -- with the C
ABI's results on the same bytes and with the specification restated in C++; another descriptor is refused, not run on the CPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_orb")


def test_cpp_dropin_describe_features():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 5
    assert 'descriptor "ORB" only' in r.stderr        # the refusal is loud
