"""The per-frame front end as one call (ps_front_end_frames, ps_frame_assembly.h) against the same steps as they could be run before it.

In one process, 640 x 480 colour, the shipped parameters (ORB 500 / 1.2 / 8 / 20, grid 1 x 1, maximalTrackedFeatures 500, DBScanEps 1,
TUM fr1 camera and distortion), device-resident batches of 1, 64 and 499 frames; ms per call, warmed, median [least .. greatest] of
five, (a) and (b) alternating:
  (a) ps_front_end_frames: images and depth in, frame set out, call -> synchronised;
  (b) THE CONTROL, what a host had to do without it: ps_orb_detect_frames, ps_dbscan_thin_device, torch.gather,
      ps_orb_pyramids_build_device, ps_describe_features_device; synchronise; download of the positions, the kept indices and the
      counts; per frame ps_remove_image_distortion + ps_keypoints2Dto3D (host pointers) on the described positions; upload of the
      points; synchronised;
  (c) the two new launches alone, ps_gather_keypoints and ps_assemble_frames, on the arrays (b) left, timed with device events.
(a) and (b) must produce the same descriptors, points and counts.  Scene: orb_detect_times.py's; depth: a tilted plane with noise
and holes.  argv[1]: output file."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import api, device_batch  # noqa: E402
from putslam_amd._abi import TUM_DEPTH_SCALE, TUM_FR1_DIST, TUM_FR1_K, frame_geometry, front_end_params  # noqa: E402

ROWS, COLS, CN = 480, 640, 3
REPS = 5
CAP = 500
EPS = 1.0      # putslammatcherOpenCVParameters.xml:70


def scene(seed):
    rng = np.random.RandomState(seed)
    img = np.full((ROWS, COLS), 100, np.int32)
    for _ in range(1500):
        x0, y0, w, h = rng.randint(0, COLS), rng.randint(0, ROWS), rng.randint(2, 80), rng.randint(2, 60)
        img[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256)
    return np.clip(img + rng.randint(-6, 7, size=img.shape), 0, 255).astype(np.uint8)


def frames(F):
    base = np.stack([scene(1), scene(2), scene(3)], axis=2)
    rng = np.random.RandomState(4)
    v, u = np.mgrid[0:ROWS, 0:COLS]
    depth = (4000 + 12 * u + 9 * v + rng.randint(0, 40, size=(ROWS, COLS))).astype(np.uint16)
    depth[rng.rand(ROWS, COLS) < 0.08] = 0
    return (np.stack([np.roll(base, (3 * f, 5 * f), axis=(0, 1)) for f in range(F)]),
            np.stack([np.roll(depth, (3 * f, 5 * f), axis=(0, 1)) for f in range(F)]))


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def fmt(ts):
    ts = sorted(ts)
    return "%9.3f [%8.3f .. %8.3f]" % (ts[len(ts) // 2], ts[0], ts[-1])


def main():
    args = sys.argv[1:]
    dev = torch.device("cuda:0")
    ctx = api.Context(0)
    prm = front_end_params(dbscan_eps=EPS)
    geo = frame_geometry(TUM_FR1_K, TUM_FR1_DIST, TUM_DEPTH_SCALE)
    out = ["640 x 480 x 3, the shipped parameters; ms per call, warmed, median [least .. greatest] of %d; (b) is the control" % REPS, ""]
    all_img, all_dep = frames(499)
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for F in (1, 64, 499):
            himg, hdep = all_img[:F], all_dep[:F]
            imgs, deps = torch.from_numpy(himg).to(dev), torch.from_numpy(hdep.view(np.int16)).to(dev)
            # (a)
            fe = device_batch.FrontEnd(ctx, ROWS, COLS, CN, F, prm)
            rows = device_batch.FrameRowsDevice(F, CAP, dev, side=())

            def run_a():
                device_batch.front_end_frames_batch(ctx, fe, imgs, deps, geo, CAP, out=rows)

            # (b)
            det = device_batch.OrbDetector(ctx, ROWS, COLS, CN, F, prm.detect)
            pyr = device_batch.OrbPyramids(ctx, ROWS, COLS, CN, F, prm.describe)
            slots = torch.arange(F, dtype=torch.int32, device=dev)
            blocks = device_batch.detect_features_orb_batch(ctx, det, imgs, prm.detect, CAP)
            dblocks = [torch.zeros((F, CAP, 32), dtype=torch.uint8, device=dev), torch.zeros((F, CAP), dtype=torch.int32, device=dev),
                       torch.zeros((F,), dtype=torch.int32, device=dev)]
            left = {}

            def run_b():
                xy, resp, ang, octv, cnt = device_batch.detect_features_orb_batch(ctx, det, imgs, prm.detect, CAP, *blocks)
                kept, nkept = device_batch.dbscan_thin_device(ctx, xy, cnt, octv, EPS, 2, 1)
                ix = kept.long().clamp_(0, CAP - 1)     # (the rows beyond nkept are not written)
                gxy, gang, goct = torch.gather(xy, 1, ix[..., None].expand(-1, -1, 2)), torch.gather(ang, 1, ix), torch.gather(octv, 1, ix)
                pyr.build(imgs)
                desc, kidx, nk = device_batch.describe_features_batch(ctx, pyr, slots, gxy, gang, goct, nkept, *dblocks)
                torch.cuda.synchronize()
                hxy, hk, hn = gxy.cpu().numpy(), kidx.cpu().numpy(), nk.cpu().numpy()
                pts = np.zeros((F, CAP, 3), np.float32)
                for f in range(F):
                    n = int(hn[f])
                    if n:
                        und = ctx.remove_image_distortion(hxy[f][hk[f, :n]], TUM_FR1_K, TUM_FR1_DIST)
                        pts[f, :n] = ctx.keypoints2Dto3D(und, hdep[f], TUM_FR1_K, TUM_DEPTH_SCALE)
                left.update(pts=torch.from_numpy(pts).to(dev), desc=desc, nk=nk, kept=kept, nkept=nkept, gxy=gxy, kidx=kidx, det=(xy, resp, ang, octv))

            run_a(), run_b()
            ta, tb = [], []
            for _ in range(REPS):
                ta.append(wall_ms(run_a))
                tb.append(wall_ms(run_b))
            torch.cuda.synchronize()
            n = left["nk"].cpu().numpy()
            assert rows.nkpts.cpu().numpy().tolist() == n.tolist()
            cols = torch.arange(CAP, device=dev)[None, :, None] < left["nk"][:, None, None]
            assert torch.equal(torch.where(cols, rows.desc, 0), torch.where(cols, left["desc"], 0))
            assert torch.equal(torch.where(cols, rows.pts, 0).view(torch.int32), torch.where(cols, left["pts"], 0).view(torch.int32))
            # (c)
            xy, resp, ang, octv = left["det"]
            g = [torch.zeros_like(t) for t in (xy, resp, ang, octv)] + [torch.zeros((F,), dtype=torch.int32, device=dev)]
            asm = device_batch.FrameRowsDevice(F, CAP, dev)

            def run_gather():
                ctx.gather_keypoints(left["kept"].data_ptr(), left["nkept"].data_ptr(), F, CAP, xy.data_ptr(), resp.data_ptr(), ang.data_ptr(),
                                     octv.data_ptr(), *[t.data_ptr() for t in g])

            def run_assemble():
                device_batch.assemble_frames(ctx, geo, deps, g[0], left["kidx"], left["nk"], g[2], g[1], g[3], out=asm)

            ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            run_gather(), run_assemble()
            tg, ts = [ev_ms(run_gather) for _ in range(REPS)], [ev_ms(run_assemble) for _ in range(REPS)]
            a_med, b_med = sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]
            lines = ["%3d frames resident, %d .. %d rows a frame (same descriptors, points and counts from (a) and (b))" % (F, n.min(), n.max()),
                     "    (a) ps_front_end_frames                    %s   %9.2f us a frame" % (fmt(ta), a_med * 1e3 / F),
                     "    (b) control: separate calls + host step    %s   %9.2f us a frame   (b) / (a) = %.2f" % (fmt(tb), b_med * 1e3 / F, b_med / a_med),
                     "    (c) ps_gather_keypoints alone              %s" % fmt(tg),
                     "        ps_assemble_frames alone, every output %s" % fmt(ts), ""]
            for line in lines:
                print(line, flush=True)
            out.extend(lines)
            fe.close(), det.close(), pyr.close()
            del imgs, deps, rows, asm, blocks, dblocks, left, g
    if args:
        open(args[0], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
