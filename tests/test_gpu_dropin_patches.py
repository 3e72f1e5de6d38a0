"""The drop-in's MatchingOnPatches -- the reference's constructors, computePatch, computeGradient, optimizeLocation, the getters
and the batch form optimizeLocations -- on cv::Mat-shaped images that are regions of larger ones: tests/cpp/test_dropin_patches
runs the three-call protocol point by point and the batch form against vectors tests/patches_ref.py wrote, byte for byte."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import patches_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tests", "cpp", "test_dropin_patches")

CASES = [  # rows, cols, channels, row padding, patchSize, maxIter, minSqrtIncrement
    (48, 64, 1, 5, 5, 50, 5e-7),        # the demo's parameters
    (61, 97, 3, 7, 13, 50, 0.04),       # the shipped ones, colour
    (61, 97, 1, 0, 17, 50, 0.04),
    (48, 64, 3, 3, 31, 20, 1e-3),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-p%d" % (c[1], c[0], c[2], c[4]))
def test_cpp_dropin_patches(tmp_path, case):
    if not os.path.exists(EXE):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    rows, cols, cn, pad, ps, max_iter, min_inc = case
    step = cols * cn + pad
    old = R.smooth_texture(rows, cols, 60 + ps, cn)
    new = R.smooth_texture(rows, cols, 60 + ps, cn, shift=(1, -1))
    old[2:12, 20:34] = 77                                            # a flat region: NaN inverse Hessians for the small patch
    pts = R.drawn_points(np.random.default_rng(200 + ps), 24, rows, cols, R.half(ps))
    if ps <= 5:
        pts[12, :2] = (26.5, 6.5)
    want = R.align_batch(old, new, pts[:, :2], pts[:, 2:], ps, max_iter, min_inc)
    assert {1, 3, 5, 6} <= set(want["status"].tolist()) and (ps > 5 or want["status"][12] == 2)

    def padded(img):
        buf = np.full((rows, step), 0xA5, np.uint8)
        buf[:, :cols * cn] = img.reshape(rows, cols * cn)
        return buf.tobytes()
    cases, expected = str(tmp_path / "cases.bin"), str(tmp_path / "expected.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<8id", rows, cols, cn, step, ps, max_iter, len(pts), 0, min_inc))
        f.write(padded(old) + padded(new) + np.ascontiguousarray(pts, np.float64).tobytes())
    with open(expected, "wb") as f:
        for k in range(len(pts)):
            f.write(struct.pack("<ii", int(want["status"][k]), int(want["iterations"][k])) + want["pts"][k].tobytes() + want["patch"][k].tobytes()
                    + want["gx"][k].tobytes() + want["gy"][k].tobytes() + want["inv"][k].tobytes())
    r = subprocess.run([EXE, cases, expected], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "dropin patches ok: 24 points" in r.stdout and "FAILED" not in r.stdout
    assert "taps leave the image" in r.stderr and "putslam_hip:" in r.stderr        # the refusals are loud
