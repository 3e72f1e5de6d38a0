"""The measurements of a map batch as Edge3D data (ps_measurement_edges, ps_uncertainty.h) against what a
host can do without it, in one process, alternating, medians of five, call -> synchronised, at 1 / 64 / 499 pairs x about 150 / 500
inliers (the printed figure is the measured mean), for uncertainty models 0, 1 and 2, on 640 x 480 colour and depth frames:
 (a) ps_map_pairs_device, then ps_measurement_edges behind it on the same stream, synchronise, download of the edges block;
 (b) THE CONTROL: ps_map_pairs_device, synchronise, download of the masks, the matches, the counts, the depth and the colour
     frames, a single-thread C++ restatement of the loop (uncertainty_host_loop.cpp, g++ -O2 -ffp-contract=off), upload of the
     result.
(a) and (b) give the same bytes (asserted).  Nothing is asserted about the times: the table is written whichever way it comes out.
Usage: python profiles/scripts/uncertainty_times.py [out.txt]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402
from putslam_amd import api, synth  # noqa: E402
from putslam_amd import device_batch as D  # noqa: E402
from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, frame_geometry, make_config,  # noqa: E402
                              sensor_model)

ROWS, COLS, FRAMES = 480, 640, 4
REPEATS = 5
MEMBERS = ("count", "map_row", "cur_row", "uv", "position", "normal", "gradient", "info")


def build_control(root):
    so = os.path.join(tempfile.mkdtemp(), "uncertainty_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "putslam_amd", "csrc"), os.path.join(root, "profiles", "scripts", "uncertainty_host_loop.cpp"), "-o", so])
    fn = C.CDLL(so).unc_host_edges
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                   C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13
    return fn


def scene(P, n, rng):
    """FRAMES frames of n key points and their views a centimetre off; P pairs (f, f); positions inside the image"""
    seq = synth.make_sequence(FRAMES, n, config=3, index=900 + n)
    vdesc = seq["desc"] ^ np.packbits(rng.random((FRAMES, n, 256)) < 0.03, axis=2)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)
    level = np.zeros((FRAMES, n), np.int32)
    frames, views = D.FrameSetDevice(seq["desc"], seq["pts"], [n] * FRAMES), D.FrameSetDevice(vdesc, vpos, [n] * FRAMES)
    pairs = np.array([(p % FRAMES, p % FRAMES) for p in range(P)], np.int32)
    batch = D.MapBatchDevice(views, level, frames, level, pairs, 2 * n)
    xyu = (rng.random((FRAMES, n, 2)) * [COLS - 1, ROWS - 1]).astype(np.float32)
    return batch, xyu, np.ascontiguousarray(seq["pts"], np.float32), pairs


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    control = build_control(root)
    ctx = api.Context(0)
    rng = np.random.default_rng(3)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    geo, sens = frame_geometry(TUM_FR1_K, (0.0,) * 5, 5000.0), sensor_model(scaleUncertaintyNormal=3.0, scaleUncertaintyGradient=0.25)
    depth = rng.integers(2000, 20000, size=(FRAMES, ROWS, COLS)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.1] = 0
    images = rng.integers(0, 256, size=(FRAMES, ROWS, COLS, 3)).astype(np.uint8)
    ddep, dimg = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(images).cuda()
    frame_of = torch.arange(FRAMES, dtype=torch.int32, device="cuda:0")
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lines = []
    for n in (150, 500):
        for P in (1, 64, 499):
            batch, xyu, fpts, pairs = scene(P, n, rng)
            dxyu = torch.from_numpy(xyu).cuda()
            cap = batch.cap
            out = D.MeasurementEdges(P, cap, "cuda:0")
            host = dict(count=np.zeros(P, np.int32), map_row=np.zeros((P, cap), np.int32), cur_row=np.zeros((P, cap), np.int32),
                        uv=np.zeros((P, cap, 2), np.float32), position=np.zeros((P, cap, 3)), normal=np.zeros((P, cap, 3)),
                        gradient=np.zeros((P, cap, 3)), info=np.zeros((P, cap, 9)))
            up = {k: torch.zeros(v.shape, dtype=getattr(out, k).dtype, device="cuda:0") for k, v in host.items()}
            frame_host = np.arange(FRAMES, dtype=np.int32)
            torch.cuda.synchronize()                    # (the calls below run on the context's own stream)
            for model in (0, 1, 2):
                def device():
                    D.run_map_pairs(ctx, prm, cfg, TUM_FR1_K, batch, use_torch_stream=False)
                    D.measurement_edges(ctx, batch, dxyu, geo, ddep, dimg, sens, model, frame_of, out=out, use_torch_stream=False)
                    ctx.synchronize()
                    return out.download()

                def control_run():
                    D.run_map_pairs(ctx, prm, cfg, TUM_FR1_K, batch, use_torch_stream=False)
                    ctx.synchronize()
                    res = batch.download()
                    dep, img = ddep.cpu().numpy(), dimg.cpu().numpy()
                    matches, num, mask = (np.ascontiguousarray(res[k]) for k in ("matches", "numMatches", "inlierMask"))
                    control(C.byref(geo), C.byref(sens), model, pv(img), COLS * 3, ROWS * COLS * 3, FRAMES, pv(dep), COLS * 2, ROWS * COLS * 2, FRAMES,
                            ROWS, COLS, pv(frame_host), pv(pairs), P, FRAMES, FRAMES, n, cap, pv(matches), pv(num), pv(mask), pv(fpts), pv(xyu),
                            *[pv(host[k]) for k in MEMBERS])
                    for k in MEMBERS:
                        up[k].copy_(torch.from_numpy(host[k]))
                    torch.cuda.synchronize()
                    return host

                for k in host:
                    host[k][...] = 0
                a, b = device(), control_run()          # warm, and the same bytes
                for k in MEMBERS:
                    assert a[k].tobytes() == b[k].tobytes(), (n, P, model, k)
                ta, tb = [], []
                for _ in range(REPEATS):
                    t = time.perf_counter()
                    device()
                    ta.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    control_run()
                    tb.append(time.perf_counter() - t)
                ma, mb = float(np.median(ta)), float(np.median(tb))
                lines.append("%3d pairs x %3d key points (%.0f inliers a pair), model %d: (a) device %.3f ms [%.3f .. %.3f], (b) control %.3f ms "
                             "[%.3f .. %.3f], (b) / (a) = %.2f%s" % (P, n, float(a["count"].mean()), model, ma * 1e3, min(ta) * 1e3, max(ta) * 1e3, mb * 1e3,
                                                                    min(tb) * 1e3, max(tb) * 1e3, mb / ma, "" if ma <= mb else "   (a) LOSES to the control"))
                print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
