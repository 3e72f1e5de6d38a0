"""FAST-9/16 key point detection on the GPU (ps_fast.h) against the host loop it replaces.

In one process, medians of five, ms per call, call -> synchronised:
  * ps_detect_features_device for 1 / 64 / 499 frames of 640 x 480, grey and colour, with the shipped parameters (threshold 10,
    suppression on, grid 1 x 1, maximalTrackedFeatures 500) and with grid 4 x 4 -- and the three passes (score, select, join) each
    queued alone through ps_debug_fast_passes and timed with device events;
  * the score pass as a share of the HBM rate for the bytes it moves: rows x cols x cn read, three bytes a pixel written (grey,
    score, corner -- two if the grey plane, kept for ps_debug_fast_maps, is not counted);
  * one frame through ps_detect_features (host pointers, the upload and the detector's allocation included) against a
    single-thread C++ restatement of the same specification (fast_host_loop.cpp, g++ -O2, compiled into a temporary directory),
    alternating; the two must return the same bytes.
Scene: 1500 random rectangles on grey 100 with +-6 noise, every frame the one before rolled by (3, 5) pixels; colour: three such
scenes as channels.  argv[1]: output file."""
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
from putslam_amd._abi import detect_params  # noqa: E402

ROWS, COLS = 480, 640
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12     # bytes / s: the data sheet's rate and a float4 copy's, measured


def scene(seed):
    rng = np.random.RandomState(seed)
    img = np.full((ROWS, COLS), 100, np.int32)
    for _ in range(1500):
        x0, y0, w, h = rng.randint(0, COLS), rng.randint(0, ROWS), rng.randint(2, 80), rng.randint(2, 60)
        img[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256)
    return np.clip(img + rng.randint(-6, 7, size=img.shape), 0, 255).astype(np.uint8)


def frames(F, cn):
    base = scene(1) if cn == 1 else np.stack([scene(1), scene(2), scene(3)], axis=2)
    return np.stack([np.roll(base, (3 * f, 5 * f), axis=(0, 1)) for f in range(F)])


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
    out = ["640 x 480, threshold 10, suppression on, maximalTrackedFeatures 500; ms per call, call -> synchronised, medians of 5",
           "cn  grid  frames | total    | score    select   join   (device events, each pass alone) | score pass: GB/s moved, share of 8.0 TB/s "
           "(of the 6.29 TB/s a copy reaches) | key points a frame"]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for cn in (1, 3):
            host = frames(499, cn)
            for F in (1, 64, 499):
                imgs = torch.from_numpy(host[:F]).to(dev)
                det = device_batch.FastDetector(ctx, ROWS, COLS, cn, F)
                for g in (1, 4):
                    p = detect_params(grid_rows=g, grid_cols=g)
                    xy, resp, cnt = device_batch.detect_features_batch(ctx, det, imgs, p)
                    run = lambda m: device_batch.detect_features_batch(ctx, det, imgs, p, None, xy, resp, cnt, True, m)   # noqa: E731
                    t_all, _ = med(lambda: run(7), wall_ms)
                    t_score, _ = med(lambda: run(1), ev_ms)
                    t_sel, _ = med(lambda: run(2), ev_ms)
                    t_join, _ = med(lambda: run(4), ev_ms)
                    moved = F * ROWS * COLS * (cn + 3)
                    rate = moved / (t_score * 1e-3)
                    out.append("%-3d %dx%d   %-6d | %8.3f | %8.3f %8.3f %8.3f | %8.1f GB/s  %5.1f %%  (%5.1f %%) | %.1f" % (
                        cn, g, g, F, t_all, t_score, t_sel, t_join, rate / 1e9, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY,
                        float(cnt.float().mean())))
                    print(out[-1], flush=True)
                det.close()
                del imgs
    out.append("")
    out.append("one frame, host pointers: single-thread C++ restatement (g++ -O2) against ps_detect_features, alternating, same bytes")
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "fast_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "fast_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.fast_detect_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]
        for cn in (1, 3):
            img = np.ascontiguousarray(frames(1, cn)[0])
            for g in (1, 4):
                p = detect_params(grid_rows=g, grid_cols=g)
                hx, hr = np.zeros((500, 2), np.float32), np.zeros(500, np.float32)

                def host():
                    t = time.perf_counter()
                    n = H.fast_detect_host(img.ctypes.data, ROWS, COLS, cn, COLS * cn, p.threshold, p.nonmaxSuppression, p.gridRows,
                                           p.gridCols, p.maximalTrackedFeatures, hx.ctypes.data, hr.ctypes.data)
                    return (time.perf_counter() - t) * 1e3, n

                def gpu():
                    t = time.perf_counter()
                    r = ctx.detect_features(img, p)   # synchronous
                    return (time.perf_counter() - t) * 1e3, r
                host(), gpu()
                th, tg = [], []
                for _ in range(5):
                    x, n = host()
                    y, r = gpu()
                    th.append(x)
                    tg.append(y)
                    assert r[0].tobytes() == hx[:n].tobytes() and r[1].tobytes() == hr[:n].tobytes(), (cn, g)
                out.append("cn %d, grid %dx%d: host loop %8.3f ms, ps_detect_features %7.3f ms (%d key points, same bytes)" % (
                    cn, g, g, np.median(th), np.median(tg), n))
                print(out[-1], flush=True)
    txt = "\n".join(out)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
