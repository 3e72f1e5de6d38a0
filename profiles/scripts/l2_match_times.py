"""The float-descriptor matcher (ps_match_l2.h): its matrix-core prefilter against its value-exact twin, and the single call against
the host loop it replaces.

In one process, alternating regions, medians of five:
  * ps_match_l2_device on 64 and 499 pairs x 2000 keypoints x D = 64 / 128 with option "matcher_l2" = 1 (prefilter + exact) and
    = 0 (exact sweep), device events around the call; the two must return the same bytes;
  * ps_match_l2_f32 on one 2000 x 2000 pair, call -> returned, against a single-thread C++ restatement of the host loop
    (l2_host_loop.cpp, g++ -O2 -ffp-contract=off, compiled into a temporary directory); the two must return the same matches.
Scenes: putslam_amd.synth's SURF-like (D = 64) and SIFT-like (D = 128) rows, 70 % of a frame's rows noisy copies of the previous
frame's.  argv[1]: output file."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import api, synth  # noqa: E402
from putslam_amd.device_batch import FrameSetF32Device, PairBatchDevice, run_match_l2  # noqa: E402

N = 2000


def frames(kind, count, distinct=16):
    """`count` frames in which consecutive ones are linked: `distinct` linked frames walked forth and back."""
    rng = np.random.default_rng(2026)
    rows = [synth.float_rows(rng, N, kind)]
    for _ in range(distinct - 1):
        truth = np.where(rng.random(N) < 0.3, -1, rng.permutation(N))
        rows.append(synth.float_rows_linked(rng, rows[-1], truth, kind))
    walk = list(range(distinct)) + list(range(distinct - 2, 0, -1))
    return np.stack([rows[walk[i % len(walk)]] for i in range(count)])


def batch_ms(ctx, fs, batch, form):
    ctx.set_option("matcher_l2", form)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run_match_l2(ctx, fs, batch)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    out = []
    ctx = api.Context(0)
    out.append("device %s; %d keypoints a frame; medians of five, alternating regions" % (ctx.arch, N))
    out.append("")
    out.append("ps_match_l2_device (device events), ms per call and us per pair")
    out.append("%-6s %-5s %-26s %-26s %s" % ("pairs", "D", "prefilter + exact (1)", "exact sweep (0)", "sweep / prefilter"))
    for kind in ("surf", "sift"):
        D = synth.FLOAT_DIM[kind]
        for P in (64, 499):
            desc = frames(kind, P + 1)
            fs = FrameSetF32Device(desc, None, np.full(P + 1, N, np.int32))
            pairs = np.stack([np.arange(P), np.arange(1, P + 1)], axis=1).astype(np.int32)
            b1, b0 = PairBatchDevice(pairs, N), PairBatchDevice(pairs, N)
            batch_ms(ctx, fs, b1, 1)
            batch_ms(ctx, fs, b0, 0)       # warm-up: the arena grows here
            t1, t0 = [], []
            for _ in range(5):
                t1.append(batch_ms(ctx, fs, b1, 1))
                t0.append(batch_ms(ctx, fs, b0, 0))
            g1, g0 = b1.download(), b0.download()
            same = np.array_equal(g1["numMatches"], g0["numMatches"]) and all(
                g1["matches"][p, :g1["numMatches"][p]].tobytes() == g0["matches"][p, :g0["numMatches"][p]].tobytes() for p in range(P))
            m1, m0 = float(np.median(t1)), float(np.median(t0))
            out.append("%-6d %-5d %8.3f ms %8.2f us    %8.3f ms %8.2f us    %.2f x   %s, %d matches a pair" %
                       (P, D, m1, 1e3 * m1 / P, m0, 1e3 * m0 / P, m0 / m1, "same bytes" if same else "BYTES DIFFER",
                        int(g1["numMatches"].mean())))
            del fs, b1, b0
    ctx.set_option("matcher_l2", 1)
    out.append("")
    out.append("ps_match_l2_f32, one 2000 x 2000 pair (call -> returned, uploads included) against the single-thread host loop")
    root = os.path.abspath(".")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "l2_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               os.path.join(root, "profiles", "scripts", "l2_host_loop.cpp"), "-o", so])
        H = C.CDLL(so)
        H.l2_match_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        for kind in ("surf", "sift"):
            q, t, _ = synth.float_scene(kind, N, N, index=5)
            idx, dist = np.zeros((N, 2), np.int32), np.zeros(N, np.float32)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            ctx.match_l2(q, t)
            tg, th = [], []
            for _ in range(5):
                s = time.perf_counter()
                m = ctx.match_l2(q, t)
                tg.append(time.perf_counter() - s)
                s = time.perf_counter()
                n = H.l2_match_host(vp(q), N, vp(t), N, q.shape[1], vp(idx), vp(dist))
                th.append(time.perf_counter() - s)
            same = n == len(m) and np.array_equal(idx[:n, 0], m["queryIdx"]) and np.array_equal(idx[:n, 1], m["trainIdx"]) and \
                dist[:n].tobytes() == m["distance"].tobytes()
            out.append("D = %-4d GPU %8.3f ms   host loop %9.1f ms   %7.0f x   %s, %d matches" %
                       (q.shape[1], 1e3 * np.median(tg), 1e3 * np.median(th), np.median(th) / np.median(tg),
                        "same matches" if same else "MATCHES DIFFER", n))
    text = "\n".join(out) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
