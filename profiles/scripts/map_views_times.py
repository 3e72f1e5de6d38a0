"""Map views built on the device (ps_map_views_device, ps_map_view.h) against the host path they replace, in one process,
alternating regions, medians of five, at 2000 and 5000 candidates with ten observations each:
 (a) a single-threaded C++ host loop over the same store layout (map_views_host_loop.cpp beside this file, g++ -O2) + the upload
     of the views it built (desc, pts, nkpts, level: pageable buffers into preallocated device tensors, synchronised),
 (b) ONE ps_map_views_device call, call -> synchronised, store and request resident,
at 1, 64 and 499 views.  The bar: at 64 and at 499 views (b) takes at most a tenth of (a) per view -- the script exits with
status 1 if it does not.  (c) one frame's retry ladder end to end, pose in -> matchXYZ results out: the view built by (a') the
host loop for one view, then Context.match_xyz_ladder (uploads, one call of ten pairs, one download) against (b') the request
uploaded, ps_map_views_device, ps_frame_levels_device and ps_map_pairs_device on resident data, the ten stats downloaded.
`--kernels V N` only runs (b) a few times: the program of a `rocprofv3 --kernel-trace --stats -- python ... --kernels 499 2000` run."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import map_pairs_ref as mref  # noqa: E402
import map_view_ref as vref  # noqa: E402  (the scenes and helpers of the tests)
from putslam_amd import api  # noqa: E402
from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402


def ladder(ctx, lib, n, out):
    """(c): one frame, one view of n candidates, the ladder of ten."""
    import torch
    from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice, build_map_views, frame_levels_device, run_map_pairs
    rng = np.random.default_rng(77)
    scene = vref.timing_scene(n, 1, seed=n + 1)
    tm = vref.ViewTiming(ctx, lib, scene, require_visible=True)
    tm.host()
    tm.device()
    kept = tm.check()
    store, cam_inv, ang, cand, cc = scene
    views = vref.build_views(store, cam_inv, ang, 0.5, vref.K_TUM, vref.IMAGE, n, cand, cc, True, fast=True)
    fr = vref.frames_from_views(rng, views, [0], [n], n)
    lvl = vref.frame_levels(fr["pos"], fr["nkpts"], fr["octave"], fr["det"])
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    lad = [mref.ladder_try(0.12, 0.55, k) for k in range(1, 11)]
    fs = FrameSetDevice(fr["desc"], fr["pos"], fr["nkpts"])
    oct_d, det_d = torch.from_numpy(fr["octave"]).to(fs.device), torch.from_numpy(fr["det"]).to(fs.device)
    pairs = np.zeros((10, 2), np.int32)
    ta, tb = [], []
    for rep in range(6):
        t = time.perf_counter()
        tm.host()                                                   # the view on the host (and its upload, which the ladder repeats)
        k = int(tm.hb["nkpts"][0])
        ctx.match_xyz_ladder(tm.hb["pts"][0, :k], tm.hb["desc"][0, :k], tm.hb["level"][0, :k], fr["pos"][0], fr["desc"][0], lvl[0],
                             prm, cfg, TUM_FR1_K)
        ta.append(time.perf_counter() - t)
        t = time.perf_counter()
        built = build_map_views(ctx, tm.sd, cam_inv, ang, 0.5, vref.K_TUM, vref.IMAGE, n, cand=tm.d["cand"], cand_counts=tm.d["cc"],
                                require_visible=True, out=tm.out, use_torch_stream=False)
        cur = frame_levels_device(ctx, fs, oct_d, det_d, use_torch_stream=False)
        b = MapBatchDevice(built, built.map_level, fs, cur, pairs, 8 * n, radius=[x[0] for x in lad], ratio=[x[1] for x in lad])
        run_map_pairs(ctx, prm, cfg, TUM_FR1_K, b, use_torch_stream=False)
        ctx.synchronize()
        b.stats.cpu()
        tb.append(time.perf_counter() - t)
    out.append("%4d candidates, one frame's ladder of ten, pose in -> results out (%d features in view): host-built view + "
               "match_xyz_ladder %.3f ms; request upload + views + levels + map batch on the device %.3f ms (the second includes "
               "allocating the batch's output block)" % (n, kept, np.median(ta[1:]) * 1e3, np.median(tb[1:]) * 1e3))


def main():
    ctx = api.Context(0)
    lib = vref.build_host_loop(tempfile.mkdtemp())
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        V, n = int(sys.argv[2]), int(sys.argv[3])
        tm = vref.ViewTiming(ctx, lib, vref.timing_scene(n, V, seed=V))
        for _ in range(8):
            tm.device()
        return 0
    out, ok = [], True
    for n in (2000, 5000):
        for V in (1, 64, 499):
            tm = vref.ViewTiming(ctx, lib, vref.timing_scene(n, V, seed=V))
            a, a0, b = tm.medians()
            kept = tm.check()
            line = ("%4d candidates x 10 observations, %3d views (%d kept on average): (a) host loop + upload %.1f us/view (loop alone "
                    "%.1f), (b) one device call %.2f us/view (%.3f ms per call), (a)/(b) = %.1f" % (n, V, kept, a / V * 1e6, a0 / V * 1e6,
                                                                                                   b / V * 1e6, b * 1e3, a / b))
            if V >= 64:
                good = b * 10 <= a
                ok = ok and good
                line += "   bar (b) <= (a) / 10: %s" % ("met" if good else "MISSED")
            out.append(line)
            del tm
        ladder(ctx, lib, n, out)
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        open(sys.argv[1], "w").write(txt + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
