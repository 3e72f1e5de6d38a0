"""Pyramidal Lucas-Kanade tracking on the GPU (ps_klt.h) against the host loop it replaces.

In one process, medians of five, ms per call, call -> synchronised:
  * pyramids + track + select (ps_klt_pyramids_build_device, ps_klt_track_device, ps_klt_select_device) for 1 / 64 / 499 pairs of
    consecutive 640 x 480 frames at 150 / 500 / 2000 points a pair, grey and colour, with the shipped winSize 7, maxLevels 3,
    maxIter 30, eps 0.01, trackingErrorThreshold 25 and minimalReprojDistanceNewTrackingFeatures 3 -- and the split over the
    three stages, each timed on its own with device events (the pyramid stage is seven launches, the other two one each);
  * one pair through ps_perform_tracking (host pointers, uploads and the allocation of the pyramid set included) against a
    single-thread C++ restatement of the same specification (klt_host_loop.cpp, g++ -O2 -ffp-contract=off, compiled into a
    temporary directory), alternating regions; the two must return the same bytes.
Scene: a sum of 24 cosines, every frame 1.3 px right and 0.7 px up of the one before; points uniform over the image.
argv[1]: output file."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import api, device_batch  # noqa: E402
from putslam_amd._abi import klt_params  # noqa: E402

ROWS, COLS = 480, 640
ERR_THR, MIN_DIST = 25.0, 3.0


def frames(F, cn, dev):
    """(F, ROWS, COLS[, 3]) uint8 on the device: frame f is the texture sampled at (x - 1.3 f, y + 0.7 f)."""
    g = torch.Generator(device="cpu").manual_seed(7)
    y, x = torch.meshgrid(torch.arange(ROWS, device=dev, dtype=torch.float32), torch.arange(COLS, device=dev, dtype=torch.float32), indexing="ij")
    out = torch.empty((F, ROWS, COLS, cn), dtype=torch.uint8, device=dev)
    coef = torch.rand((cn, 24, 4), generator=g)
    for f in range(F):
        xs, ys = x - 1.3 * f, y + 0.7 * f
        for c in range(cn):
            acc = torch.zeros_like(x)
            for k in range(24):
                fx, fy, a, ph = coef[c, k].tolist()
                acc += (0.3 + 0.7 * a) * torch.cos((fx - 0.5) * 0.9 * xs + (fy - 0.5) * 0.9 * ys + 6.2832 * ph)
            out[f, :, :, c] = torch.clamp(torch.round(127.5 + acc * (110.0 / 24 ** 0.5)), 0, 255).to(torch.uint8)
    return out[..., 0] if cn == 1 else out


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def med(fn, timer, reps=5):
    timer(fn)
    ts = []
    for _ in range(reps):
        ms, r = timer(fn)
        ts.append(ms)
    return float(np.median(ts)), r


def main():
    args = sys.argv[1:]
    dev = torch.device("cuda:0")
    ctx = api.Context(0)
    prm = klt_params()
    rng = np.random.default_rng(2026)
    out = ["640 x 480, winSize 7, maxLevels 3, maxIter 30, eps 0.01; ms per call, call -> synchronised, medians of 5",
           "cn  pairs  points | total    | pyramids  track    select  (device events, each stage alone) | tracked  kept (per pair)"]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for cn in (1, 3):
            for P in (1, 64, 499):
                imgs = frames(P + 1, cn, dev)
                pyr = device_batch.KltPyramids(ctx, ROWS, COLS, cn, P + 1)
                pairs = torch.stack([torch.arange(P, dtype=torch.int32), torch.arange(1, P + 1, dtype=torch.int32)], 1).contiguous().to(dev)
                build = lambda: pyr.build(imgs)   # noqa: E731
                t_build, _ = med(build, ev_ms)
                for n in (150, 500, 2000):
                    pts = torch.from_numpy(np.stack([rng.uniform(0, COLS - 1, (P, n)), rng.uniform(0, ROWS - 1, (P, n))], 2).astype(np.float32)).to(dev)
                    cnt = torch.full((P,), n, dtype=torch.int32, device=dev)
                    nxt, st, er = device_batch.track_klt_pairs(ctx, pyr, pairs, pts, cnt, prm)
                    track = lambda: device_batch.track_klt_pairs(ctx, pyr, pairs, pts, cnt, prm, nxt, st, er)   # noqa: E731
                    select = lambda: device_batch.select_tracked(ctx, nxt, st, er, cnt, ERR_THR, MIN_DIST)      # noqa: E731

                    def whole():
                        build()
                        track()
                        return select()
                    t_track, _ = med(track, ev_ms)
                    t_sel, sel = med(select, ev_ms)
                    t_all, _ = med(whole, wall_ms)
                    out.append("%-3d %-6d %-6d | %8.3f | %8.3f %8.3f %8.3f | %.0f  %.0f" % (
                        cn, P, n, t_all, t_build, t_track, t_sel, float(st.float().sum(1).mean()), float(sel[1].float().mean())))
                    print(out[-1], flush=True)
                pyr.close()
                del imgs
    out.append("")
    out.append("one pair, host pointers: single-thread C++ restatement (g++ -O2) against ps_perform_tracking, alternating, same bytes")
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "klt_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "klt_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.klt_track_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double]
        H.klt_select_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
        for cn in (1, 3):
            pair = frames(2, cn, dev).cpu().numpy()
            a, b = np.ascontiguousarray(pair[0]), np.ascontiguousarray(pair[1])
            for n in (150, 500, 2000):
                pts = np.stack([rng.uniform(0, COLS - 1, n), rng.uniform(0, ROWS - 1, n)], 1).astype(np.float32)
                hn, hs, he, hk = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.int32)

                def host():
                    t = time.perf_counter()
                    H.klt_track_host(a.ctypes.data, b.ctypes.data, ROWS, COLS, cn, COLS * cn, pts.ctypes.data, hn.ctypes.data, n,
                                     hs.ctypes.data, he.ctypes.data, prm.winSize, prm.maxLevels, prm.maxCount, prm.eps, prm.flags,
                                     prm.minEigThreshold)
                    k = H.klt_select_host(hn.ctypes.data, hs.ctypes.data, he.ctypes.data, n, ERR_THR, MIN_DIST, hk.ctypes.data)
                    return (time.perf_counter() - t) * 1e3, k

                def gpu():
                    t = time.perf_counter()
                    r = ctx.perform_tracking(a, b, pts, ERR_THR, MIN_DIST, prm)   # synchronous
                    return (time.perf_counter() - t) * 1e3, r
                host(), gpu()
                th, tg = [], []
                for _ in range(5):
                    x, k = host()
                    y, r = gpu()
                    th.append(x)
                    tg.append(y)
                    assert r["next_pts"].tobytes() == hn.tobytes() and r["status"].tobytes() == hs.tobytes() and \
                        r["err"].tobytes() == he.tobytes() and r["kept_idx"].tobytes() == hk[:k].tobytes(), (cn, n)
                out.append("cn %d, %4d points: host loop %8.3f ms, ps_perform_tracking %7.3f ms (%d tracked, %d kept, same bytes)" % (
                    cn, n, np.median(th), np.median(tg), int(hs.sum()), k))
                print(out[-1], flush=True)
    txt = "\n".join(out)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
