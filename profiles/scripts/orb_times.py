"""ORB description on the GPU (ps_orb.h) against the host loop it replaces.

In one process, 640 x 480, scaleFactor 1.2, 8 levels, grey and colour, 500 and 2000 key points a frame (uniform over the part of the
image that is described, random angles, random octaves 0 .. 7); ms per call, warmed, median [least .. greatest] of seven:
  * a resident batch of 499 frames: ps_orb_pyramids_build_device + ps_describe_features_device, call -> synchronised, and each pass
    (level 0, the resizes, the blurs, the placement, the rows) queued alone through ps_debug_orb_passes and timed with device
    events; the bytes a pass moves -- planes read and written once, 512 sample bytes + 48 a row -- as a rate and as a share of the
    6.29 TB/s a float4 copy reaches on this device;
  * one frame through ps_describe_features (host pointers; the set's allocation, the uploads and the download included) against a
    single-thread C++ restatement of the same specification (orb_host_loop.cpp, g++ -O2, compiled into a temporary directory),
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

ROWS, COLS, NL, SF = 480, 640, 8, 1.2
HBM_COPY = 6.29e12     # bytes / s a float4 copy reaches, measured (profiles/r16a)
REPS = 7


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


def keypoints(F, n, seed):
    rng = np.random.RandomState(seed)
    xy = np.stack([rng.uniform(31, COLS - 31.01, (F, n)), rng.uniform(31, ROWS - 31.01, (F, n))], axis=2).astype(np.float32)
    return xy, rng.uniform(0, 360, (F, n)).astype(np.float32), rng.randint(0, NL, (F, n)).astype(np.int32)


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
    F = 499
    out = ["640 x 480, scaleFactor 1.2, 8 levels; ms per call, warmed, median [least .. greatest] of %d" % REPS, ""]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for cn in (1, 3):
            imgs = torch.from_numpy(frames(F, cn)).to(dev)
            pyr = device_batch.OrbPyramids(ctx, ROWS, COLS, cn, F)
            planes = [pyr.level(l)[0][0] * pyr.level(l)[0][1] for l in range(NL)]
            moved = {1: F * ROWS * COLS * (cn + 1), 2: F * sum(planes[l - 1] + planes[l] for l in range(1, NL)), 4: F * 2 * sum(planes)}
            out.append("cn %d, %d frames resident -- the pyramids (bytes moved: planes read and written once)" % (cn, F))
            out.append("  build, call -> synchronised     %s" % fmt(spread(lambda: pyr.build(imgs), wall_ms)))
            for mask, name in ((1, "level 0 (grey)"), (2, "resizes, 7 launches"), (4, "blurs, 8 launches")):
                t = spread(lambda: pyr.build(imgs, passes=mask), ev_ms)
                rate = moved[mask] / (t[0] * 1e-3)
                out.append("  %-30s  %s   %7.1f MB  %7.1f GB/s  %5.1f %% of the copy rate" % (name, fmt(t), moved[mask] / 1e6, rate / 1e9,
                                                                                         100 * rate / HBM_COPY))
            for n in (500, 2000):
                xy, ang, octv = (torch.from_numpy(a).to(dev) for a in keypoints(F, n, 7 + n))
                slots = torch.arange(F, dtype=torch.int32, device=dev)
                counts = torch.full((F,), n, dtype=torch.int32, device=dev)
                desc, kept, num = device_batch.describe_features_batch(ctx, pyr, slots, xy, ang, octv, counts)
                run = lambda m: device_batch.describe_features_batch(ctx, pyr, slots, xy, ang, octv, counts, desc, kept, num, True, m)  # noqa: E731
                out.append("  %d key points a frame" % n)
                out.append("    describe, call -> synchronised  %s" % fmt(spread(lambda: run(31), wall_ms)))
                both = lambda: (pyr.build(imgs), run(31))  # noqa: E731
                out.append("    build + describe                %s" % fmt(spread(both, wall_ms)))
                for mask, name, nbytes in ((8, "placement", F * n * 16), (16, "rows", F * n * (512 + 48))):
                    t = spread(lambda: run(mask), ev_ms)
                    rate = nbytes / (t[0] * 1e-3)
                    out.append("    %-30s  %s   %7.1f MB  %7.1f GB/s  %5.1f %% of the copy rate" % (name, fmt(t), nbytes / 1e6, rate / 1e9,
                                                                                             100 * rate / HBM_COPY))
                assert int(num.min()) == n
            for line in out[-14:]:
                print(line, flush=True)
            pyr.close()
            del imgs
    out.append("")
    out.append("one frame, host pointers: single-thread C++ restatement (g++ -O2) against ps_describe_features, alternating, same bytes")
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "orb_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "orb_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.orb_describe_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for cn in (1, 3):
            img = np.ascontiguousarray(frames(1, cn)[0])
            for n in (500, 2000):
                xy, ang, octv = (a[0].copy() for a in keypoints(1, n, 7 + n))
                hd, hk = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32)
                last = {}

                def host():
                    last["n"] = H.orb_describe_host(img.ctypes.data, ROWS, COLS, cn, COLS * cn, SF, NL, xy.ctypes.data, ang.ctypes.data,
                                                    octv.ctypes.data, n, hd.ctypes.data, hk.ctypes.data)

                def gpu():
                    last["r"] = ctx.describe_features(img, xy, ang, octv)   # synchronous

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
                    assert r[0].tobytes() == hd[:k].tobytes() and r[1].tobytes() == hk[:k].tobytes(), (cn, n)
                th.sort(), tg.sort()
                out.append("cn %d, %4d key points: host loop %s ms, ps_describe_features %s ms (%d rows, same bytes)" % (
                    cn, n, fmt((th[REPS // 2], th[0], th[-1])), fmt((tg[REPS // 2], tg[0], tg[-1])), last["n"]))
                print(out[-1], flush=True)
    txt = "\n".join(out)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
