"""The per-frame front end of Matcher::detectInitFeatures (matcher.cpp:17-64) / Matcher::match (:452-516) on the CPU, from pieces
the project already has: orb_detect_ref (detect), dbscan_ref_py.dbscan_keep (thin), an index gather, orb_ref (describe), the
oracle's remove_image_distortion and keypoints2Dto3D applied to the DESCRIBED key points in the described order, and the detection
distance in numpy float32.  What ps_front_end_frames (putslam_amd/csrc/ps_frame_assembly.h) must equal byte for byte.

The scene: four 150 x 200 frames with a depth image each -- a texture, the same texture moved by (3, 2) pixels with its depth (a pair
RANSAC accepts), a noise image and a constant image without a key point.  The detector runs eight levels, the descriptor fewer:
describe drops the key points of the octaves it lacks and groups the rest by octave, so its keptIdx is neither complete nor
ascending.  (With equal level counts describe could drop nothing: the detector's own border of 31 pixels per level is the
descriptor's.)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dbscan_ref_py as R  # noqa: E402
import orb_detect_ref as D  # noqa: E402
import orb_ref as O  # noqa: E402

f32 = np.float32
ROWS, COLS = 150, 200
CAPACITY = 100
DBSCAN_EPS = 3.0
K = np.array([210.0, 0, 99.5, 0, 208.0, 74.5, 0, 0, 1], f32)     # a camera whose image is 200 x 150
DIST5 = (-0.0410, 0.3286, 0.0087, 0.0051, -0.5643)               # TUM fr1 (resources/datasetConfig/freiburg1_desk.xml:7)
DEPTH_SCALE = 5000.0
SHIFT = (2, 3)                                                   # rows, cols frame 1 is moved by

# (name, detector parameters, the descriptor's level count): grid 1 x 1 -- five live levels, three described -- and grid 1 x 2 --
# ROIs of 150 x 100 with three live levels, two described
CASES = [("grid1x1", D.params(120, 1.2, 8, 20, 1, 1, CAPACITY), 3), ("grid1x2", D.params(80, 1.2, 8, 20, 1, 2, CAPACITY), 2)]


def images(cn):
    """[texture, the texture moved by SHIFT, noise, constant], grey or with three channels that differ"""
    g = O.texture(ROWS, COLS, 4)
    out = [g, np.roll(g, SHIFT, axis=(0, 1)), D.scene("noise256", ROWS, COLS)]
    if cn == 3:
        out = [D.colour(x, 17 + i) for i, x in enumerate(out)]
    return out + [np.full((ROWS, COLS) if cn == 1 else (ROWS, COLS, 3), 50, np.uint8)]


def depths():
    """A depth image per frame: a tilted plane 0.8 .. 3 m with holes (0 = missing) and noise, so that neighbouring pixels differ;
    frame 1's is frame 0's moved with the image."""
    out = []
    for f in range(4):
        rng = np.random.RandomState(100 + f)
        v, u = np.mgrid[0:ROWS, 0:COLS]
        d = 4000 + 40 * u + 15 * v * (f + 1) + rng.randint(0, 50, size=(ROWS, COLS))
        d[rng.rand(ROWS, COLS) < 0.1] = 0
        out.append(d.astype(np.uint16))
    out[1] = np.roll(out[0], SHIFT, axis=(0, 1))
    return out


def det_dist(pts):
    """matcher.cpp:52-57: float products, float sums left to right, the float square root, widened to double"""
    p = np.asarray(pts, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (p[:, 0] * p[:, 0]).astype(f32)
        s = (s + (p[:, 1] * p[:, 1]).astype(f32)).astype(f32)
        s = (s + (p[:, 2] * p[:, 2]).astype(f32)).astype(f32)
        return np.sqrt(s).astype(f32).astype(np.float64)


def assemble(oracle, xy, kept_idx, depth, K=K, dist5=DIST5, scale=DEPTH_SCALE, angle=None, response=None, octave=None):
    """ps_assemble_frames for one frame: dict(xy, xy_undist, pts, det_dist, src_idx[, angle, response, octave]) of the rows kept_idx
    names, in that order.  depth: a (rows, cols) uint16 view (any row stride); the oracle's rule is applied to it as the dense image
    the reference holds, so what lies between the rows of a padded view is never read."""
    kept_idx = np.asarray(kept_idx, np.int32)
    depth = np.ascontiguousarray(depth)
    p = np.ascontiguousarray(np.asarray(xy, f32).reshape(-1, 2)[kept_idx])
    und = oracle.remove_image_distortion(p, K, dist5) if len(p) else p.copy()
    pts = oracle.keypoints2Dto3D(und, depth, K, scale) if len(p) else np.zeros((0, 3), f32)
    out = dict(xy=p, xy_undist=und, pts=pts, det_dist=det_dist(pts), src_idx=kept_idx)
    for name, a in (("angle", angle), ("response", response), ("octave", octave)):
        if a is not None:
            out[name] = np.asarray(a)[kept_idx]
    return out


def chain(oracle, imgs, deps, p, describe_levels, eps=DBSCAN_EPS):
    """The chain, frame by frame.  Returns ([dict(desc (k, 32), pts (k, 3), xy, xy_undist, angle, response, octave, src_idx,
    det_dist)], [(detected, thinned, described)])."""
    frames, counts = [], []
    for img, dep in zip(imgs, deps):
        xy, resp, ang, octv = D.detect_closed(img, p)
        keep = R.dbscan_keep(xy, octv, eps, 2, 1)
        txy, tresp, tang, toct = xy[keep], resp[keep], ang[keep], octv[keep]      # the gather
        desc, kept = O.describe(O.pyramid(img, p["scale_factor"], describe_levels), txy, tang, toct)
        out = assemble(oracle, txy, kept, dep, angle=tang, response=tresp, octave=toct)
        out["desc"] = desc
        frames.append(out)
        counts.append((len(xy), len(keep), len(kept)))
    return frames, counts


def frame_set(frames, cap):
    """desc (F, cap, 32) u8, pts (F, cap, 3) f32, nkpts (F,) i32: the dense set the oracle's vo_pairs takes"""
    F = len(frames)
    desc, pts, n = np.zeros((F, cap, 32), np.uint8), np.zeros((F, cap, 3), f32), np.zeros(F, np.int32)
    for f, fr in enumerate(frames):
        k = len(fr["pts"])
        desc[f, :k], pts[f, :k], n[f] = fr["desc"], fr["pts"], k
    return desc, pts, n
