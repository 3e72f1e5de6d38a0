"""FrameMatcherHIP::trackStep (the first half of Matcher::trackKLT, matcher.cpp:147-211, as one call) on cv::Mat-shaped inputs:
tests/cpp/test_dropin_track_vo compares every output with ps_track_vo_pair's on the same pair and with the reference's loop
:151-211 restated in C++ over the drop-in's performTracking, RGBD::removeImageDistortion, RGBD::keypoints2Dto3D and RANSAC classes,
as bytes; removeTooCloseFeatures > 0 is refused on std::cerr with the identity."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_track_vo")


def test_cpp_dropin_track_step():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 6
