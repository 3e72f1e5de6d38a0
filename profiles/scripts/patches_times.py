"""Sub-pixel matching on patches (ps_patch_align, ps_patches.h) against what a host can do without it, in
one process, alternating, medians, call -> synchronised, at 1 / 64 / 499 pairs x 150 / 500 points on 640 x 480 frames, grey and
colour, patch 13, 50 iterations, 0.04 (the shipped PatchesParams):
 (a) ps_patch_align on resident frames and points, fused (the model built from the old slot): one call then a synchronise, timed
     with the host's clock through the Python wrapper -- for the small shapes that is launch and wrapper latency, not kernel time --
     and QUEUED equal calls behind one another with one synchronise, per call: the window that holds enough work;
 (b) the host form ps_optimize_locations for ONE pair, uploads and downloads included;
 (c) THE CONTROL: the single-thread C++ restatement (patches_host_loop.cpp over csrc/ps_patches_host.h, g++ -O2
     -ffp-contract=off) on the same inputs, on host arrays: no transfer at all is charged to it.
(a) and (c) give the same bytes (asserted).  With every line: the share of points per status and the mean iteration count.  One more line per
channel count takes 64 x 500 with minSqrtIncrement 0: every point runs to the iteration limit.
Nothing is asserted about the times: the table is written whichever way it comes out.
Usage: python profiles/scripts/patches_times.py [out.txt]   (without a path: the next free profiles/rNNa/patches.txt)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402
from putslam_amd import api  # noqa: E402
from putslam_amd import device_batch as D  # noqa: E402
from putslam_amd._abi import PsPatchParams, patch_params  # noqa: E402

ROWS, COLS, FRAMES = 480, 640, 4
SHIFTS = [(0, 0), (1, 2), (3, 1), (2, 4)]          # frame f is the texture read at this offset (rows, cols)
REPEATS, CONTROL_REPEATS, QUEUED = 5, 3, 10


def build_control(root):
    so = os.path.join(tempfile.mkdtemp(), "patches_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "putslam_amd", "csrc"), os.path.join(root, "profiles", "scripts", "patches_host_loop.cpp"), "-o", so])
    fn = C.CDLL(so).patches_host_align
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(PsPatchParams), C.c_void_p,
                                                                                        C.c_void_p]
    return fn


def frames(cn, rng):
    pad = 8
    planes = []
    for _ in range(cn):
        f = rng.random((ROWS + 2 * pad, COLS + 2 * pad))
        for _ in range(4):
            f = sum(np.roll(np.roll(f, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)) / 9.0
        planes.append(np.round(16 + 223 * (f - f.min()) / (f.max() - f.min())).astype(np.uint8))
    tex = np.stack(planes, -1)
    out = np.stack([tex[pad - s[0]:pad - s[0] + ROWS, pad - s[1]:pad - s[1] + COLS] for s in SHIFTS])
    return np.ascontiguousarray(out if cn == 3 else out[..., 0])


def scene(P, n, rng):
    """P pairs (f, f + 1); old positions anywhere a 13 x 13 patch fits with a margin, starts up to a pixel off the truth"""
    pairs = np.array([(p % FRAMES, (p + 1) % FRAMES) for p in range(P)], np.int32)
    old = np.stack([rng.uniform(16, COLS - 16, (P, n)), rng.uniform(16, ROWS - 16, (P, n))], -1)
    flow = np.array([[SHIFTS[b][1] - SHIFTS[a][1], SHIFTS[b][0] - SHIFTS[a][0]] for a, b in pairs], np.float64)
    new = old + flow[:, None, :] + rng.uniform(-1, 1, (P, n, 2))
    return pairs, np.ascontiguousarray(old), np.ascontiguousarray(new), np.full(P, n, np.int32)


def next_free(profiles):
    """profiles/rNNa/patches.txt for the first NN above every round directory there is"""
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)", d) for d in os.listdir(profiles)) if m]
    return os.path.join(profiles, "r%02da" % (max(rounds + [0]) + 1), "patches.txt")


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    control = build_control(root)
    ctx = api.Context(0)
    rng = np.random.default_rng(5)
    prm = patch_params()
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    dev = torch.device("cuda:0")
    lines = ["patch %d, %d iterations; 640 x 480; medians of %d (control: %d), [min .. max]" % (prm.patchSize, prm.maxIter, REPEATS, CONTROL_REPEATS)]
    def measure(cn, imgs, dimgs, P, n, prm, label):
        row, frame = COLS * cn, ROWS * COLS * cn
        pairs, old, new, counts = scene(P, n, rng)
        dpairs, dold, dcounts = torch.from_numpy(pairs).to(dev), torch.from_numpy(old).to(dev), torch.from_numpy(counts).to(dev)
        dstart = torch.from_numpy(new).to(dev)
        # newPts is refined in place, so every queued call of a window gets its own copy of the starts: QUEUED equal calls of work
        dnews = [torch.empty_like(dstart) for _ in range(QUEUED)]
        dst, dit = torch.zeros((P, n), dtype=torch.uint8, device=dev), torch.zeros((P, n), dtype=torch.int32, device=dev)
        hst, hit = np.zeros((P, n), np.uint8), np.zeros((P, n), np.int32)
        torch.cuda.synchronize()                 # (the calls below run on the context's own stream)

        def device(calls):
            for t_ in dnews[:calls]:
                t_.copy_(dstart)                 # (the starts are put back before the clock starts)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for t_ in dnews[:calls]:
                D.align_patches(ctx, dimgs, dpairs, dold, t_, dcounts, prm, status=dst, iterations=dit, use_torch_stream=False)
            ctx.synchronize()
            return (time.perf_counter() - t) / calls

        def control_run():
            h = new.copy()
            t = time.perf_counter()
            rc = control(pv(imgs), row, frame, FRAMES, ROWS, COLS, cn, pv(pairs), pv(old), pv(h), pv(counts), P, n, C.byref(prm), pv(hst), pv(hit))
            dt = time.perf_counter() - t
            assert rc == 0
            return dt, h

        device(QUEUED)
        _, h = control_run()                     # warm, and the same bytes
        assert dnews[-1].cpu().numpy().tobytes() == h.tobytes() and dst.cpu().numpy().tobytes() == hst.tobytes(), (cn, n, P)
        assert dit.cpu().numpy().tobytes() == hit.tobytes(), (cn, n, P)
        t1, tq, tc = [], [], []
        for r in range(REPEATS):
            t1.append(device(1))
            tq.append(device(QUEUED))
            if r < CONTROL_REPEATS:
                tc.append(control_run()[0])
        m1, mq, mc = float(np.median(t1)), float(np.median(tq)), float(np.median(tc))
        share = np.bincount(hst.reshape(-1), minlength=7) / hst.size
        line = ("%s, %d channel(s), %3d pairs x %3d points: (a) device, one call then synchronise %.3f ms [%.3f .. %.3f]; %d calls queued, one "
                "synchronise, per call %.3f ms [%.3f .. %.3f]; (c) control %.3f ms [%.3f .. %.3f]; (c) / (a queued) = %.1f%s"
                % (label, cn, P, n, m1 * 1e3, min(t1) * 1e3, max(t1) * 1e3, QUEUED, mq * 1e3, min(tq) * 1e3, max(tq) * 1e3, mc * 1e3, min(tc) * 1e3,
                   max(tc) * 1e3, mc / mq, "" if mq <= mc else "   (a) LOSES to the control"))
        if P == 1:
            tb = []
            for _ in range(REPEATS + 1):
                t = time.perf_counter()
                got = ctx.optimize_locations(imgs[pairs[0, 0]], imgs[pairs[0, 1]], old[0], new[0], prm)
                tb.append(time.perf_counter() - t)
            assert got[0].tobytes() == h[0].tobytes()
            line += "; (b) host form, one pair, transfers included %.3f ms [%.3f .. %.3f]" % (float(np.median(tb[1:])) * 1e3, min(tb[1:]) * 1e3,
                                                                                              max(tb[1:]) * 1e3)
        line += "\n      status shares 0..6: %s; mean iterations %.2f" % (" ".join("%.3f" % s for s in share), float(hit.mean()))
        lines.append(line)
        print(line, flush=True)

    for cn in (1, 3):
        imgs = frames(cn, rng)
        dimgs = torch.from_numpy(imgs).to(dev)
        for n in (150, 500):
            for P in (1, 64, 499):
                measure(cn, imgs, dimgs, P, n, prm, "shipped 0.04")
        # minSqrtIncrement 0: no increment is below it, every point that stays inside runs all 50 steps
        measure(cn, imgs, dimgs, 64, 500, patch_params(13, 50, 0.0), "to the limit (0.0)")
    out = sys.argv[1] if len(sys.argv) > 1 else next_free(os.path.join(root, "profiles"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("written to", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
