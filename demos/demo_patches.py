"""The reference's demos/demoPatches.cpp on the device: a 5 x 5 patch around the feature at (64, 312) of an old image is aligned
in a new image from the start (66, 314) -- 50 iterations at most, minSqrtIncrement 5e-7 -- through the reference's three calls:
computePatch, computeGradient, optimizeLocation (api.Context.compute_patch / compute_patch_gradient / optimize_location).

The reference reads 0.png and 1.png, which are not shipped: the pair here is synthetic, a seeded smooth colour texture and the same
texture moved by one pixel right and one down, so the feature's true new position is (65, 313).

    python -m demos.demo_patches        ->  x, y = 64 312 / newX, newY = 66 314 / ... / FINAL: <x> <y>
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS = 480, 640
X, Y, NEW_X, NEW_Y = 64.0, 312.0, 66.0, 314.0
PATCH_SIZE, MAX_ITER, MIN_SQRT_INCREMENT = 5, 50, 0.0000005


def make_pair(seed=2015):
    """(old, new): rows x cols x 3 uint8; new[y + 1, x + 1] = old[y, x]"""
    rng = np.random.default_rng(seed)
    field = rng.random((ROWS + 1, COLS + 1, 3))
    for _ in range(6):   # a 3 x 3 box blur, six times: smooth over a few pixels
        field = sum(np.roll(np.roll(field, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
    field = (field - field.min()) / (field.max() - field.min())
    img = np.round(16 + 223 * field).astype(np.uint8)
    return np.ascontiguousarray(img[1:, 1:]), np.ascontiguousarray(img[:-1, :-1])


def main():
    from putslam_amd import api
    from putslam_amd._abi import patch_params
    old, new = make_pair()
    ctx = api.Context(0)
    prm = patch_params(PATCH_SIZE, MAX_ITER, MIN_SQRT_INCREMENT)
    print("x, y = %g %g" % (X, Y))
    print("newX, newY = %g %g" % (NEW_X, NEW_Y))
    patch, _ = ctx.compute_patch(old, [[X, Y]], prm)
    gx, gy, inv, _ = ctx.compute_patch_gradient(old, [[X, Y]], prm)
    pts, status, iterations = ctx.optimize_location(patch, new, [[NEW_X, NEW_Y]], gx, gy, inv, prm, old_img=old)
    print("status %d after %d iterations" % (status[0], iterations[0]))
    print("\nFINAL: %r %r" % (float(pts[0, 0]), float(pts[0, 1])))


if __name__ == "__main__":
    main()
