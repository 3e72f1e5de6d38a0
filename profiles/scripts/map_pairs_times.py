"""Batched map matching (ps_map_pairs_device, ps_map_match.h) against the path it replaces, in one process, alternating
regions, medians of at least five each, E0 / RANSAC 487, at 500 x 500 (the shipped keypoint budget) and 2000 x 2000:
 (a) a host loop of ps_match_xyz + ps_ransac_rigid3d per pair (host pointers, preallocated buffers, straight through ctypes),
 (b) ONE ps_map_pairs_device call, call -> synchronised, on resident views / frames,
at 10, 64 and 499 pairs; (c) the retry ladder of ten (one call of ten pairs) against one, three and ten sequential tries.
The bar: at 64 and at 499 pairs (b) takes at most a tenth of (a) per pair -- the script exits with status 1 if it does not.
`--kernels P N` only runs (b) a few times: the program of a `rocprofv3 --kernel-trace --stats --output-format csv -- python ... --kernels 499 2000` run."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import map_pairs_ref as mref  # noqa: E402  (the scenes of the tests)
from putslam_amd import api  # noqa: E402
from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402
from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice  # noqa: E402

V = mref.TIMING_VIEWS
scene, HostLoop, batch_time = mref.timing_scene, mref.HostLoop, mref.batch_time


def main():
    ctx = api.Context(0)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        P, n = int(sys.argv[2]), int(sys.argv[3])
        views, frames = scene(ctx, n, n)
        vs, fs = FrameSetDevice(views["desc"], views["pos"], views["nkpts"]), FrameSetDevice(frames["desc"], frames["pos"], frames["nkpts"])
        pairs = np.array([(p % V, p % V) for p in range(P)], np.int32)
        b = MapBatchDevice(vs, views["level"], fs, frames["level"], pairs, 4 * n)
        for _ in range(6):
            batch_time(ctx, prm, cfg, b)
        return 0
    out, ok = [], True
    for n in (500, 2000):
        views, frames = scene(ctx, n, n)
        vs, fs = FrameSetDevice(views["desc"], views["pos"], views["nkpts"]), FrameSetDevice(frames["desc"], frames["pos"], frames["nkpts"])
        for P in (10, 64, 499):
            a, bb, b = mref.host_against_batch(ctx, prm, cfg, views, frames, vs, fs, P, 4 * n)
            got = b.download()
            line = ("%4d x %4d, %3d pairs: (a) host loop %.1f us/pair, (b) one device call %.2f us/pair (%.3f ms per batch), "
                    "(a)/(b) = %.1f; %d matches per pair on average" % (n, n, P, a / P * 1e6, bb / P * 1e6, bb * 1e3, a / bb,
                                                                          int(np.mean(np.maximum(got["numMatches"], 0)))))
            if P >= 64:
                good = bb * 10 <= a
                ok = ok and good
                line += "   bar (b) <= (a) / 10: %s" % ("met" if good else "MISSED")
            out.append(line)
        # (c) the ladder of ten against sequential tries
        rng = np.random.default_rng(5)
        fr1 = mref.make_frames(rng, ctx, [n], n)
        vw1 = mref.make_views(rng, fr1, [n], n, source=[0], sigma=0.01, shift=0.15)
        host1 = HostLoop(ctx, vw1, fr1, prm)
        args = (vw1["pos"][0], vw1["desc"][0], vw1["level"][0], fr1["pos"][0], fr1["desc"][0], fr1["level"][0], prm, cfg, TUM_FR1_K)
        ctx.match_xyz_ladder(*args)
        tl, ts = [], {1: [], 3: [], 10: []}
        for _ in range(5):
            t = time.perf_counter()
            r = ctx.match_xyz_ladder(*args)
            tl.append(time.perf_counter() - t)
            for k in ts:
                t = time.perf_counter()
                for j in range(1, k + 1):
                    rad, rat = mref.ladder_try(0.12, 0.55, j)
                    host1.pair(0, 0, rad, rat, 1 + j - 1)
                ts[k].append(time.perf_counter() - t)
        out.append("%4d x %4d ladder of ten (uploads, one call, one download; took try %d): %.3f ms; sequential tries: one %.3f ms, "
                   "three %.3f ms, ten %.3f ms" % (n, n, r["try_used"], np.median(tl) * 1e3, np.median(ts[1]) * 1e3,
                                                   np.median(ts[3]) * 1e3, np.median(ts[10]) * 1e3))
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
