"""DBScan keypoint thinning on the GPU (ps_dbscan.h): call -> synchronised times of ps_dbscan_thin (host arrays in, survivors'
indices out) at N = 500 / 2000 / 5000 on the bench frames' kind of data, the same for the drop-in's ::DBScan::run from C++
(dbscan_dropin_times.cpp, compiled into a temporary directory), one 500-frame x 2000 batch through ps_dbscan_thin_device, and the
two worst cases (a dense blob, a long chain).  Medians; one line per measurement."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import api, device_batch  # noqa: E402


def frame(rng, n, frac=0.25):
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(np.float32)
    for i in range(1, n):
        if rng.random() < frac:
            a = rng.uniform(0, 2 * np.pi)
            xy[i] = xy[i - 1] + np.float32(0.5) * np.array([np.cos(a), np.sin(a)], np.float32)
    return xy


def host_time(ctx, xy, reps, eps=1.0, mp=2, ffc=1):
    ctx.dbscan_thin(xy, None, eps, mp, ffc)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        kept = ctx.dbscan_thin(xy, None, eps, mp, ffc)
        ts.append(time.perf_counter() - t)
    return np.median(ts) * 1e6, len(kept)


def main():
    rng = np.random.default_rng(2026)
    ctx = api.Context(0)
    out = []
    for n in (500, 2000, 5000):
        us, k = host_time(ctx, frame(rng, n), 50)
        out.append("ps_dbscan_thin N=%d eps=1 minPts=2 ffc=1: %.1f us call->synchronised (median of 50), %d kept" % (n, us, k))
    blob = rng.uniform(0, 0.7, (3000, 2)).astype(np.float32)
    us, k = host_time(ctx, blob, 5)
    out.append("worst case, dense 1-px blob N=3000: %.1f us (median of 5), %d kept" % (us, k))
    chain = np.stack([np.arange(5000) * 0.9, np.zeros(5000)], 1).astype(np.float32)
    us, k = host_time(ctx, chain, 5)
    out.append("worst case, 0.9-px chain N=5000: %.1f us (median of 5), %d kept" % (us, k))
    F, cap = 500, 2000
    xy = np.stack([frame(rng, cap) for _ in range(F)])
    dev = torch.device("cuda:0")
    txy = torch.from_numpy(xy).to(dev)
    cnt = torch.full((F,), cap, dtype=torch.int32, device=dev)
    device_batch.dbscan_thin_device(ctx, txy, cnt, None, 1.0, 2, 1)
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_batch.dbscan_thin_device(ctx, txy, cnt, None, 1.0, 2, 1)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    out.append("ps_dbscan_thin_device 500 frames x 2000: %.1f us per batch (median of 10, events) = %.2f us per frame"
               % (np.median(ts), np.median(ts) / F))
    root = os.path.abspath(".")
    lib = os.path.join(root, "putslam_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dbscan_dropin_times")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "include"), "-I",
                               os.path.join(lib, "csrc", "dropin"), os.path.join(root, "profiles", "scripts", "dbscan_dropin_times.cpp"),
                               "-o", exe, "-L", lib, "-lputslam_dropin", "-lputslam_hip", "-Wl,-rpath," + lib])
        out += subprocess.check_output([exe], text=True, timeout=120).strip().splitlines()
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
