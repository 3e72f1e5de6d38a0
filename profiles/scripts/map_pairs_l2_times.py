"""ps_map_pairs_l2_device (float descriptors, D = 64 and 128) against ps_map_pairs_device (binary descriptors) on the same
positions and levels, and the ladder of ten tries in either form.

In one process, alternating regions, medians of five, call -> synchronised:
  * 10 / 64 / 499 pairs x 500 and 2000 keypoints, first-try parameters (radius 0.12, ratio 0.55), RANSAC 487, Euclidean error;
    eight distinct views on eight frames, pair p = (p % 8, p % 8); row capacity = keypoints;
  * Context.match_xyz_ladder / match_xyz_ladder_l2 on one 500 x 500 and one 2000 x 2000 scene, call -> returned (uploads included).
Scenes: tests/map_pairs_ref.py's frames; a view's features sit near keypoints of its frame and carry noisy copies of their
descriptors -- 5 % of the bits flipped (binary), putslam_amd.synth's linked SURF / SIFT rows (float).
argv[1]: output file.  `--kernels`: only a few 499 x 2000 calls of each form, for a kernel trace taken in a run of its own."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import map_pairs_ref as mref  # noqa: E402

from putslam_amd import api, synth  # noqa: E402
from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402
from putslam_amd.device_batch import (FrameSetDevice, FrameSetF32Device, MapBatchDevice, MapBatchF32Device, run_map_pairs,  # noqa: E402
                                      run_map_pairs_l2)

V = 8


def scene(ctx, n, seed):
    """Frames and views with binary, SURF and SIFT descriptors on one set of positions and levels."""
    rng = np.random.default_rng(seed)
    frames = mref.make_frames(rng, ctx, [n] * V, n)
    pos, level = np.zeros((V, n, 3), np.float32), np.zeros((V, n), np.int32)
    desc = {"bin": np.zeros((V, n, 32), np.uint8), "surf": np.zeros((V, n, 64), np.float32), "sift": np.zeros((V, n, 128), np.float32)}
    fdesc = {"bin": frames["desc"], "surf": np.stack([synth.float_rows(rng, n, "surf") for _ in range(V)]),
             "sift": np.stack([synth.float_rows(rng, n, "sift") for _ in range(V)])}
    for v in range(V):
        src = rng.integers(0, n, n)
        pos[v] = (frames["pos"][v, src] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
        level[v] = np.clip(frames["level"][v, src] + rng.integers(-2, 3, n), 0, 7)
        desc["bin"][v] = frames["desc"][v, src] ^ np.packbits(rng.random((n, 256)) < 0.05, axis=1)
        for kind in ("surf", "sift"):
            desc[kind][v] = synth.float_rows_linked(rng, fdesc[kind][v], src, kind)
    nk = np.full(V, n, np.int32)
    return dict(pos=pos, level=level, desc=desc, nkpts=nk), dict(pos=frames["pos"], level=frames["level"], desc=fdesc, nkpts=nk)


def batch(views, frames, kind, P, cap):
    pairs = np.array([(p % V, p % V) for p in range(P)], np.int32)
    if kind == "bin":
        vs = FrameSetDevice(views["desc"][kind], views["pos"], views["nkpts"])
        fs = FrameSetDevice(frames["desc"][kind], frames["pos"], frames["nkpts"])
        return MapBatchDevice(vs, views["level"], fs, frames["level"], pairs, cap), run_map_pairs
    vs = FrameSetF32Device(views["desc"][kind], views["pos"], views["nkpts"])
    fs = FrameSetF32Device(frames["desc"][kind], frames["pos"], frames["nkpts"])
    return MapBatchF32Device(vs, views["level"], fs, frames["level"], pairs, cap), run_map_pairs_l2


def call_s(ctx, prm, cfg, b, run):
    t = time.perf_counter()
    run(ctx, prm, cfg, TUM_FR1_K, b, use_torch_stream=False)
    ctx.synchronize()
    return time.perf_counter() - t


def main():
    kernels_only = "--kernels" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ctx = api.Context(0)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    kinds = ("bin", "surf", "sift")
    out = ["device %s; medians of five, alternating regions, call -> synchronised" % ctx.arch, "",
           "ps_map_pairs_device (binary) / ps_map_pairs_l2_device (SURF D = 64, SIFT D = 128), ms per call",
           "%-6s %-6s %10s %10s %10s   %-13s %-13s %s" % ("kpts", "pairs", "binary", "SURF", "SIFT", "SURF / binary", "SIFT / binary",
                                                            "matches a pair (binary, SURF, SIFT)")]
    for n in ((2000,) if kernels_only else (500, 2000)):
        views, frames = scene(ctx, n, 40 + n)
        for P in ((499,) if kernels_only else (10, 64, 499)):
            bs = {k: batch(views, frames, k, P, n) for k in kinds}
            for k in kinds:
                call_s(ctx, prm, cfg, *bs[k])      # warm-up: the arena grows here
            t = {k: [] for k in kinds}
            for _ in range(5):
                for k in kinds:
                    t[k].append(call_s(ctx, prm, cfg, *bs[k]))
            m = {k: 1e3 * float(np.median(t[k])) for k in kinds}
            got = {k: bs[k][0].download()["numMatches"] for k in kinds}
            assert all((got[k] >= 0).all() for k in kinds)
            out.append("%-6d %-6d %10.3f %10.3f %10.3f   %-13s %-13s %d, %d, %d" %
                       (n, P, m["bin"], m["surf"], m["sift"], "%.2f x" % (m["surf"] / m["bin"]), "%.2f x" % (m["sift"] / m["bin"]),
                        int(got["bin"].mean()), int(got["surf"].mean()), int(got["sift"].mean())))
            del bs
    if not kernels_only:
        out += ["", "the ladder of ten tries as one call (Context.match_xyz_ladder / match_xyz_ladder_l2), call -> returned, ms",
                "%-6s %10s %10s %10s   %s" % ("kpts", "binary", "SURF", "SIFT", "try taken (binary, SURF, SIFT)")]
        for n in (500, 2000):
            views, frames = scene(ctx, n, 90 + n)

            def ladder(k):
                f = ctx.match_xyz_ladder if k == "bin" else ctx.match_xyz_ladder_l2
                s = time.perf_counter()
                r = f(views["pos"][0], views["desc"][k][0], views["level"][0], frames["pos"][0], frames["desc"][k][0], frames["level"][0],
                      prm, cfg, TUM_FR1_K, max_matches=16 * n)
                return time.perf_counter() - s, r["try_used"]

            for k in kinds:
                ladder(k)
            t, used = {k: [] for k in kinds}, {}
            for _ in range(5):
                for k in kinds:
                    s, used[k] = ladder(k)
                    t[k].append(s)
            out.append("%-6d %10.3f %10.3f %10.3f   %d, %d, %d" % (n, *(1e3 * float(np.median(t[k])) for k in kinds), *(used[k] for k in kinds)))
    text = "\n".join(out) + "\n"
    print(text)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
