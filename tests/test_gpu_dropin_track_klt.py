"""FrameMatcherHIP::trackKLT (Matcher::trackKLT, matcher.cpp:133-449) on cv::Mat-shaped frames: tests/cpp/test_dropin_track_klt runs
four frames, grey and colour -- a first call with no features at all (the identity, then the refill from nothing), a frame that is
not due, a due frame whose sandbox is merged into tracked rows, another that is not due -- and compares, after every call, the pose,
the inlier matches, the returned ratio and the whole prev* state with the reference's loop restated in C++ over the drop-in's
performTracking, RGBD, RANSAC, detectFeatures, DBScan and describeFeatures classes (the walk of :359-375 literal), as bytes;
removeTooCloseFeatures > 0 is refused on std::cerr with the identity."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_track_klt")


def test_cpp_dropin_track_klt():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all ok" in r.stdout and r.stdout.count(": ok") == 9
