"""FrameMatcherHIP::frontEnd (Matcher::detectInitFeatures, matcher.cpp:19-49, as one call) on cv::Mat-shaped images:
tests/cpp/test_dropin_front_end compares its descriptors, 3-D points, key points -- all six fields -- and undistorted positions with
the C ABI's ps_front_end_frame on the same bytes, runs it as the frontEnd callable of putslam_matcher_glue.h against the matcher's
own detectInitFeatures / match on the rows it made, and has every other detector, descriptor and depth type refused."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_front_end")


def test_cpp_dropin_front_end():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 5
    assert 'detector "ORB" with descriptor "ORB" only (asked for "SURF" and "ORB")' in r.stderr        # the refusals are loud
    assert 'asked for "ORB" and "SIFT"' in r.stderr
    assert r.stderr.count("putslam_hip:") == 4      # ... and the two depth images; maximalTrackedFeatures 0 said nothing
