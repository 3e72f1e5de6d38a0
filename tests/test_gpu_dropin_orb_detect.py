"""FrameMatcherHIP::detectFeatures (MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180) with the shipped detector "ORB" on
cv::Mat-shaped images: tests/cpp/test_dropin_orb_detect compares its key points -- all six fields -- with the C ABI's results on the
same bytes and with the specification restated in C++ (tests/cpp/orb_detect_restated.h); a detector other than "ORB" and "FAST" is
refused, not run on the CPU, and the shipped detector on an image too small for its border returns nothing without a word."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_orb_detect")


def test_cpp_dropin_detect_features_orb():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 6
    assert 'detector "ORB" and detector "FAST" only (asked for "SURF")' in r.stderr        # the refusal is loud
    assert r.stderr.count("putslam_hip:") == 2      # ... and the wrong Mat type; the shipped detector on 40 x 40 said nothing
