"""The drop-in's measurement uncertainty -- RGBD::computeNormal / computeRGBGradient and their templates, DepthSensorModel's
computeCov, informationMatrixFromImageCoordinates, uncertinatyFromNormal and uncertinatyFromRGBGradient, and
FrameMatcherHIP::measurementEdges -- on cv::Mat-shaped images that are regions of larger ones: tests/cpp/test_dropin_uncertainty
compares every byte with the C ABI's ps_compute_normals, ps_compute_rgb_gradients and ps_information_matrices on the same arrays."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_uncertainty")


def test_cpp_dropin_uncertainty():
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "dropin uncertainty ok" in r.stdout and "FAILED" not in r.stdout
    assert r.stderr.count("putslam_hip:") == 1 and "trainIdx outside" in r.stderr        # the one refusal is loud
