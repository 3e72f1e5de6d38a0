"""Spatial-exclusion filters on the GPU (ps_exclusion.h) against the host loop they replace.

In one process, alternating regions, medians of five:
  * a single-thread C++ restatement of PUTSLAM::chooseFeaturesToAddToMap (exclusion_host_loop.cpp, g++ -O2, compiled into a
    temporary directory) against ps_exclude, call -> synchronised, at 500 x 1000, 2000 x 2000 and 5000 x 5000 candidates x map
    features, with the shipped cap of 200 and uncapped; the two must return the same indices;
  * a 500-frame x 2000 x 2000 batch through ps_exclude_device (device events).
Scene: half of the candidates sit on a map feature, thresholds 0.03 m and 2 px (putslammapConfig.xml:34-36).
`--batch-only N`: only N batch calls (for a rocprofv3 --kernel-trace --stats run of its own).  argv[1]: output file."""
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

F32 = np.float32
DE, DI = 0.03, 2.0


def scene(rng, n, m):
    m3 = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(0.9, 5.9, m)], 1).astype(F32)
    m2 = np.stack([rng.uniform(0, 640, m), rng.uniform(0, 480, m)], 1).astype(F32)
    f3 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.9, 5.9, n)], 1).astype(F32)
    f2 = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(F32)
    on = np.flatnonzero(rng.random(n) < 0.5)
    k = rng.integers(0, m, len(on))
    f3[on] = m3[k] + rng.normal(0, 0.005, (len(on), 3)).astype(F32)
    f2[on] = m2[k] + rng.normal(0, 0.5, (len(on), 2)).astype(F32)
    return f3, f2, m3, m2


def batch_tensors(rng, F, n, m):
    dev = torch.device("cuda:0")
    fr = [scene(rng, n, m) for _ in range(F)]
    t = lambda i: torch.from_numpy(np.stack([f[i] for f in fr])).to(dev)   # noqa: E731
    return (t(0), t(1), torch.full((F,), n, dtype=torch.int32, device=dev), t(2), t(3),
            torch.full((F,), m, dtype=torch.int32, device=dev))


def batch_ms(ctx, rule, tens):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    kept, nk = device_batch.exclude_device(ctx, rule, *tens)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), nk


def main():
    args = sys.argv[1:]
    rng = np.random.default_rng(2026)
    ctx = api.Context(0)
    if args and args[0] == "--batch-only":
        tens = batch_tensors(rng, 500, 2000, 2000)
        for cap in (200, 10 ** 6):
            for _ in range(int(args[1])):
                batch_ms(ctx, api.rule_new_map_features(DE, DI, cap), tens)
        return
    out = []
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "exclusion_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "exclusion_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.excl_c1_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int,
                                   C.c_void_p]
        for n, m in ((500, 1000), (2000, 2000), (5000, 5000)):
            f3, f2, m3, m2 = scene(rng, n, m)
            buf = np.zeros(n, np.int32)
            for cap, label in ((200, "cap 200"), (10 ** 6, "uncapped")):
                def host():
                    t = time.perf_counter()
                    k = H.excl_c1_host(f3.ctypes.data, f2.ctypes.data, n, m3.ctypes.data, m2.ctypes.data, m, DE, DI, cap, buf.ctypes.data)
                    return time.perf_counter() - t, buf[:k].copy()

                def gpu():
                    t = time.perf_counter()
                    kept = ctx.choose_new_features(f3, f2, m3, m2, DE, DI, cap)      # ps_exclude: synchronous
                    return time.perf_counter() - t, kept
                host(), gpu()                                                            # warm-up of both
                th, tg = [], []
                for _ in range(5):                                                       # alternating regions
                    a, kh = host()
                    b, kg = gpu()
                    th.append(a)
                    tg.append(b)
                    assert kh.tobytes() == kg.tobytes(), (n, m, cap)
                out.append("%d x %d, %s: host loop %.3f ms, ps_exclude %.3f ms call->synchronised (medians of 5, alternating), "
                           "%d accepted, same indices" % (n, m, label, np.median(th) * 1e3, np.median(tg) * 1e3, len(kg)))
    F = 500
    tens = batch_tensors(rng, F, 2000, 2000)
    for cap, label in ((200, "cap 200"), (10 ** 6, "uncapped")):
        rule = api.rule_new_map_features(DE, DI, cap)
        batch_ms(ctx, rule, tens)
        ts = []
        for _ in range(5):
            ms, nk = batch_ms(ctx, rule, tens)
            ts.append(ms)
        out.append("ps_exclude_device %d frames x 2000 x 2000, %s: %.3f ms per batch (median of 5, events) = %.2f us per frame, "
                   "%.0f accepted per frame" % (F, label, np.median(ts), np.median(ts) * 1e3 / F, float(nk.float().mean())))
    txt = "\n".join(out)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
