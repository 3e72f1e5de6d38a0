"""ORB detection on the GPU (ps_orb_detect.h) against the host loop it replaces.

In one process, 640 x 480, the shipped parameters (500 features, scaleFactor 1.2, 8 levels, fastThreshold 20, grid 1 x 1,
maximalTrackedFeatures 500), grey and colour; ms per call, warmed, median [least .. greatest] of five:
  * device-resident batches of 1, 64 and 499 frames: ps_orb_detect_frames, call -> synchronised, and each pass (the pyramids, the
    FAST scores, the first cut, Harris and angle, the second cut with the ROI ordering, the join) queued alone through
    ps_debug_orb_detect_passes and timed with device events;
  * one frame through ps_detect_features_orb (host pointers; the detector's allocation, the upload and the download included)
    against a single-thread C++ restatement of the same specification (orb_detect_host_loop.cpp, g++ -O2, compiled into a temporary
    directory), alternating; the two must return the same bytes.
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
from putslam_amd._abi import orb_detect_params  # noqa: E402

ROWS, COLS = 480, 640
REPS = 5
PASSES = ((1, "pyramids, 8 launches"), (2, "FAST scores, 8 launches"), (4, "first cut"), (8, "Harris + angle"), (16, "second cut + ROI order"),
          (32, "join"))


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
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def spread(fn, timer):
    timer(fn)
    ts = sorted(timer(fn) for _ in range(REPS))
    return ts[REPS // 2], ts[0], ts[-1]


def fmt(t):
    return "%8.3f [%7.3f .. %7.3f]" % t


def main():
    args = sys.argv[1:]
    dev = torch.device("cuda:0")
    ctx = api.Context(0)
    p = orb_detect_params()
    cap = 500
    out = ["640 x 480, the shipped parameters; ms per call, warmed, median [least .. greatest] of %d" % REPS, ""]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for cn in (1, 3):
            all_frames = frames(499, cn)
            for F in (1, 64, 499):
                imgs = torch.from_numpy(all_frames[:F]).to(dev)
                det = device_batch.OrbDetector(ctx, ROWS, COLS, cn, F, p)
                blocks = device_batch.detect_features_orb_batch(ctx, det, imgs, p, cap)
                run = lambda m: device_batch.detect_features_orb_batch(ctx, det, imgs, p, cap, *blocks, True, m)  # noqa: E731
                first = len(out)
                t = spread(lambda: run(63), wall_ms)
                out.append("cn %d, %3d frames resident: call -> synchronised  %s   %8.2f us a frame" % (cn, F, fmt(t), t[0] * 1e3 / F))
                for mask, name in PASSES:
                    t = spread(lambda: run(mask), ev_ms)
                    out.append("    %-28s  %s   %8.2f us a frame" % (name, fmt(t), t[0] * 1e3 / F))
                counts = blocks[4].cpu().numpy()
                out.append("    key points a frame: %d .. %d" % (counts.min(), counts.max()))
                for line in out[first:]:
                    print(line, flush=True)
                det.close()
                del imgs
    out.append("")
    out.append("one frame, host pointers: single-thread C++ restatement (g++ -O2) against ps_detect_features_orb, alternating, same bytes")
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "orb_detect_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "orb_detect_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.orb_detect_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for cn in (1, 3):
            img = np.ascontiguousarray(frames(1, cn)[0])
            hx, hr, ha, ho = np.zeros((cap, 2), np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.int32)
            last = {}

            def host():
                last["n"] = H.orb_detect_host(img.ctypes.data, ROWS, COLS, cn, COLS * cn, p.nFeatures, p.scaleFactor, p.nLevels, p.fastThreshold,
                                              p.gridRows, p.gridCols, p.maximalTrackedFeatures, hx.ctypes.data, hr.ctypes.data, ha.ctypes.data,
                                              ho.ctypes.data)

            def gpu():
                last["r"] = ctx.detect_features_orb(img, p)   # synchronous

            def clock(fn):
                t = time.perf_counter()
                fn()
                return (time.perf_counter() - t) * 1e3
            host(), gpu()
            th, tg = [], []
            for _ in range(REPS):
                th.append(clock(host))
                tg.append(clock(gpu))
                k, r = last["n"], last["r"]
                assert (r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), r[3].tobytes()) == (hx[:k].tobytes(), hr[:k].tobytes(), ha[:k].tobytes(),
                                                                                           ho[:k].tobytes()), cn
            th.sort(), tg.sort()
            out.append("cn %d: host loop %s ms, ps_detect_features_orb %s ms (%d key points, same bytes)" % (
                cn, fmt((th[REPS // 2], th[0], th[-1])), fmt((tg[REPS // 2], tg[0], tg[-1])), last["n"]))
            print(out[-1], flush=True)
    txt = "\n".join(out)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
