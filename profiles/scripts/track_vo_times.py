"""The tracking VO step as one call (ps_track_vo_pairs, ps_track_vo.h) against the same steps as a host could run them before it.

In one process, 640 x 480 x 3, winSize 7, maxLevels 3, 30 iterations, errorVersion 0 / RANSAC <= 487, the TUM fr1 camera and
distortion; 1 / 64 / 499 pairs x 150 / 500 previous points, device resident (every pair tracks its own points between the same two
slots); ms per call, warmed, median [least .. greatest] of five, (a) and (b) alternating:
  (a) ps_track_vo_pairs: previous rows in, rows and poses out, call -> synchronised;
  (b) THE CONTROL, what a host could do without it: ps_klt_track_device + ps_klt_select_device; synchronise; download of the tracked
      positions, the kept indices, the matches and the counts; per pair ps_remove_image_distortion + ps_keypoints2Dto3D +
      ps_ransac_rigid3d with seed + p (host pointers); synchronised;
  (c) the new launches alone on the arrays (a) left, timed with device events: ps_assemble_tracked, and ps_ransac_match_lists (its
      record builder and the scoring and selection launches behind it).
(a) and (b) must produce the same points, masks and poses, byte for byte.  argv[1]: output file."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import api, device_batch  # noqa: E402
from putslam_amd._abi import (DMATCH_DTYPE, EST_RANSAC, TUM_DEPTH_SCALE, TUM_FR1_DIST, TUM_FR1_K, default_ransac_params, frame_geometry,  # noqa: E402
                              klt_params, make_config, track_vo_params)

ROWS, COLS, CN = 480, 640, 3
REPS = 5
SHIFT = (2.3, -1.6)
SEED = 5


def texture(shift, seed=3, terms=40):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    x, y = x + shift[0], y + shift[1]
    out = np.zeros((ROWS, COLS, CN))
    for c in range(CN):
        for _ in range(terms):
            fx, fy = rng.uniform(-0.45, 0.45, 2)
            out[:, :, c] += rng.uniform(0.3, 1.0) * np.cos(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
    return np.clip(np.rint(127.5 + out * (110.0 / np.sqrt(terms))), 0, 255).astype(np.uint8)


def depth(shift):
    v, u = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    d = 5000 + 9 * (u - shift[0]) + 6 * (v - shift[1])
    d[(np.floor(u / 40) + np.floor(v / 40)) % 11 == 0] = 0      # holes
    return np.clip(np.rint(d), 0, 65535).astype(np.uint16)


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
    geo = frame_geometry(TUM_FR1_K, TUM_FR1_DIST, TUM_DEPTH_SCALE)
    prm = default_ransac_params(0)
    cfg, _ = make_config(EST_RANSAC, 487, seed=SEED)
    klt, tp = klt_params(7, 3, 30, 0.01), track_vo_params()
    himg = np.stack([texture((0, 0)), texture((-SHIFT[0], -SHIFT[1]))])
    hdep = np.stack([depth((0, 0)), depth(SHIFT)])
    out = ["640 x 480 x %d, winSize 7, maxLevels 3, 30 iterations, E0 / RANSAC <= 487; ms per call, warmed, median [least .. greatest] of %d; "
           "(b) is the control" % (CN, REPS), ""]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        pyr = device_batch.KltPyramids(ctx, ROWS, COLS, CN, 2, 7, 3)
        pyr.build(torch.from_numpy(himg).to(dev))
        deps = torch.from_numpy(hdep.view(np.int16)).to(dev)
        for P in (1, 64, 499):
            for n in (150, 500):
                rng = np.random.RandomState(P * 1000 + n)
                hxy = (rng.rand(P, n, 2) * [COLS - 40, ROWS - 40] + 20).astype(np.float32)
                hpts = np.zeros((P, n, 3), np.float32)
                for p in range(P):
                    hpts[p] = ctx.keypoints2Dto3D(ctx.remove_image_distortion(hxy[p], TUM_FR1_K, TUM_FR1_DIST), hdep[0], TUM_FR1_K, TUM_DEPTH_SCALE)
                rows = device_batch.TrackedRows.from_host(dev, hxy, hpts, np.full(P, n, np.int32))
                pairs = torch.from_numpy(np.tile(np.array([[0, 1]], np.int32), (P, 1))).to(dev)
                res = device_batch.TrackVoDevice(P, n, dev, ())
                left = {}

                def run_a():
                    device_batch.track_vo_pairs(ctx, pyr, deps, geo, pairs, rows, prm, cfg, tp, klt, out=res)

                blocks = [torch.zeros((P, n, 2), dtype=torch.float32, device=dev), torch.zeros((P, n), dtype=torch.uint8, device=dev),
                          torch.zeros((P, n), dtype=torch.float32, device=dev)]

                def run_b():
                    nxt, status, err = device_batch.track_klt_pairs(ctx, pyr, pairs, rows.xy, rows.counts, klt, *blocks)
                    matches, num, kept_pts, kept_idx = device_batch.select_tracked(ctx, nxt, status, err, rows.counts, tp.trackingErrorThreshold,
                                                                                   tp.minimalReprojDistanceNewTrackingFeatures)
                    torch.cuda.synchronize()
                    hk, hm, hn = kept_pts.cpu().numpy(), matches.cpu().numpy().view(DMATCH_DTYPE).reshape(P, n), num.cpu().numpy()
                    pts, mask, pose = np.zeros((P, n, 3), np.float32), np.zeros((P, n), np.uint8), np.zeros((P, 16), np.float32)
                    for p in range(P):
                        k = int(hn[p])
                        und = ctx.remove_image_distortion(hk[p, :k], TUM_FR1_K, TUM_FR1_DIST)
                        pts[p, :k] = ctx.keypoints2Dto3D(und, hdep[1], TUM_FR1_K, TUM_DEPTH_SCALE)
                        r = ctx.ransac_rigid3d(prm, make_config(EST_RANSAC, 487, seed=SEED + p)[0], TUM_FR1_K, hpts[p], pts[p, :k], hm[p, :k])
                        mask[p, :k], pose[p] = r["mask"], r["pose"].T.reshape(16)
                    left.update(pts=pts, mask=mask, pose=pose, num=hn)

                run_a(), run_b()
                ta, tb = [], []
                for _ in range(REPS):
                    ta.append(wall_ms(run_a))
                    tb.append(wall_ms(run_b))
                got = res.download()
                assert got["numMatches"].tolist() == left["num"].tolist()
                accepted = int(got["stats"]["accepted"].sum())
                for p in range(P):
                    k = int(left["num"][p])
                    assert got["rows"]["pts"][p, :k].tobytes() == left["pts"][p, :k].tobytes(), p
                    assert got["inlierMask"][p, :k].tobytes() == left["mask"][p, :k].tobytes(), p
                assert got["pose"].tobytes() == left["pose"].tobytes()
                # (c)
                asm = device_batch.TrackedRows(P, n, dev, ())
                frame = torch.ones(P, dtype=torch.int32, device=dev)
                sets_p, sets_c = device_batch.PointSets(rows.pts, rows.counts), device_batch.PointSets(res.rows.pts, res.rows.counts)
                pr = device_batch.PairResultsDevice(P, n, dev)
                m4 = res.matches.view(torch.int32)

                def run_assemble():
                    device_batch.assemble_tracked(ctx, geo, deps, frame, res.next_pts, res.kept_idx, res.num_matches, None, asm)

                def run_lists():
                    device_batch.ransac_match_lists(ctx, prm, cfg, TUM_FR1_K, sets_p, sets_c, m4, res.num_matches, None, pr)

                run_assemble(), run_lists()
                ts, tl = [ev_ms(run_assemble) for _ in range(REPS)], [ev_ms(run_lists) for _ in range(REPS)]
                assert torch.equal(pr.pose, res.pose) and torch.equal(pr.mask, res.mask)
                a_med, b_med = sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]
                kk = left["num"]
                lines = ["%3d pairs x %3d points, %d .. %d tracked, %d accepted (same points, masks and poses from (a) and (b))" % (P, n, kk.min(), kk.max(), accepted),
                         "    (a) ps_track_vo_pairs                       %s   %9.2f us a pair" % (fmt(ta), a_med * 1e3 / P),
                         "    (b) control: device tracking + host loop    %s   %9.2f us a pair   (b) / (a) = %.2f" % (fmt(tb), b_med * 1e3 / P, b_med / a_med),
                         "    (c) ps_assemble_tracked alone               %s" % fmt(ts),
                         "        ps_ransac_match_lists alone             %s" % fmt(tl), ""]
                for line in lines:
                    print(line, flush=True)
                out.extend(lines)
        pyr.close()
    if args:
        open(args[0], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
