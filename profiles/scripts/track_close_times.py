"""The whole tracked frame on the device (ps_track_vo_pairs + ps_track_close_pairs, ps_track_close.h) against what a host could do
with the first half alone.

In one process, 640 x 480 x 3, winSize 7, maxLevels 3, 30 iterations, errorVersion 0 / RANSAC <= 487, the TUM fr1 camera and
distortion, eight ORB levels; 1 / 64 / 499 pairs x 150 / 500 previous points, device resident (every pair tracks its own points
between the same two slots); the candidates are one sandbox of the current image (ps_track_candidates, outside the timed window of
both) and every pair is due ("refill") or none is ("no refill"); ms per call, warmed, median [least .. greatest] of five, (a) and
(b) alternating:
  (a) ps_track_vo_pairs + ps_track_close_pairs, call -> synchronised;
  (b) THE CONTROL, what a host can do without the second call: ps_track_vo_pairs; synchronise; download of the rows; per pair a
      numpy merge (the greedy loop, one vector test a candidate) and the levels (thresholds, vectorised); upload; ps_describe_features_device;
      download of keptIdx and the descriptors; the gather on the host;
  (c) the two new launches alone on the arrays (a) left, timed with device events: ps_track_merge_rows and ps_close_tracked_rows.
(a) and (b) must produce the same rows, descriptors and source indices, byte for byte.  argv[1]: output file."""
import ctypes as C
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from putslam_amd import _lib, api, device_batch  # noqa: E402
from putslam_amd._abi import (EST_RANSAC, TUM_DEPTH_SCALE, TUM_FR1_DIST, TUM_FR1_K, default_ransac_params, frame_geometry, front_end_params,  # noqa: E402
                              klt_params, make_config, track_close_params, track_vo_params)

ROWS, COLS, CN = 480, 640, 3
REPS = 5
SHIFT = (2.3, -1.6)
SEED = 5
MIN_DIST = 3.0
NAMES = ("xy", "xy_undist", "pts", "angle", "response", "octave", "det_dist")


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


def norm3(p):
    """float products, float sums left to right, the float root, widened"""
    s = (p[:, 0] * p[:, 0]).astype(np.float32)
    s = (s + (p[:, 1] * p[:, 1]).astype(np.float32)).astype(np.float32)
    s = (s + (p[:, 2] * p[:, 2]).astype(np.float32)).astype(np.float32)
    return np.sqrt(s).astype(np.float32).astype(np.float64)


def host_merge(have, cand, bound):
    """mergeTrackedFeatures on the undistorted positions: the accepted candidates, in order"""
    cur = np.zeros((len(have) + len(cand), 2), np.float32)
    cur[:len(have)] = have
    n, acc = len(have), []
    for i in range(len(cand)):
        d = (cur[:n] - cand[i]).astype(np.float64)
        if not ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < bound).any():
            cur[n] = cand[i]
            n += 1
            acc.append(i)
    return np.asarray(acc, np.int64)


def main():
    args = sys.argv[1:]
    dev = torch.device("cuda:0")
    ctx = api.Context(0)
    L = _lib.load()
    geo = frame_geometry(TUM_FR1_K, TUM_FR1_DIST, TUM_DEPTH_SCALE)
    prm = default_ransac_params(0)
    cfg, _ = make_config(EST_RANSAC, 487, seed=SEED)
    klt, tp = klt_params(7, 3, 30, 0.01), track_vo_params(25.0, MIN_DIST)
    t7 = (C.c_double * 7)()
    assert L.ps_level_thresholds(t7) == 0
    thresholds = np.array(list(t7))
    powers = np.array([math.pow(1.2, o) for o in range(8)])
    bound = float(L.ps_sqrt_bound_f64(MIN_DIST))
    himg = np.stack([texture((0, 0)), texture((-SHIFT[0], -SHIFT[1]))])
    hdep = np.stack([depth((0, 0)), depth(SHIFT)])
    out = ["640 x 480 x %d, winSize 7, maxLevels 3, 30 iterations, E0 / RANSAC <= 487, 8 ORB levels; ms per call, warmed, median [least .. greatest] "
           "of %d; (b) is the control" % (CN, REPS), ""]
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        dimg = torch.from_numpy(himg).to(dev)
        deps = torch.from_numpy(hdep.view(np.int16)).to(dev)
        pyr = device_batch.KltPyramids(ctx, ROWS, COLS, CN, 2, 7, 3)
        pyr.build(dimg)
        orb = device_batch.OrbPyramids(ctx, ROWS, COLS, CN, 2)
        orb.build(dimg)
        fe = device_batch.FrontEnd(ctx, ROWS, COLS, CN, 1, front_end_params())
        cand = device_batch.track_candidates(ctx, fe, dimg[1:2], deps[1:2], geo)
        torch.cuda.synchronize()
        hc = cand.download()
        nc, ccap = int(hc["nkpts"][0]), cand.max_kpts
        for P in (1, 64, 499):
            for n in (150, 500):
                rng = np.random.RandomState(P * 1000 + n)
                hxy = (rng.rand(P, n, 2) * [COLS - 40, ROWS - 40] + 20).astype(np.float32)
                hpts = np.zeros((P, n, 3), np.float32)
                for p in range(P):
                    hpts[p] = ctx.keypoints2Dto3D(ctx.remove_image_distortion(hxy[p], TUM_FR1_K, TUM_FR1_DIST), hdep[0], TUM_FR1_K, TUM_DEPTH_SCALE)
                rows = device_batch.TrackedRows.from_host(dev, hxy, hpts, np.full(P, n, np.int32), angle=(rng.rand(P, n) * 360).astype(np.float32),
                                                          response=rng.randn(P, n).astype(np.float32),
                                                          octave=rng.randint(0, 8, size=(P, n)).astype(np.int32),
                                                          det_dist=np.stack([norm3(q) for q in hpts]) * (0.6 + 1.1 * rng.rand(P, n)))
                pairs = torch.from_numpy(np.tile(np.array([[0, 1]], np.int32), (P, 1))).to(dev)
                slots = torch.ones(P, dtype=torch.int32, device=dev)
                frame0 = torch.zeros(P, dtype=torch.int32, device=dev)
                res = device_batch.TrackVoDevice(P, n, dev)
                res_b = device_batch.TrackVoDevice(P, n, dev)
                ocap = n + ccap
                tc = device_batch.TrackClose(ctx, P, ocap)
                closed = device_batch.ClosedRows(P, ocap, dev)
                for due in (True, False):
                    ctp = track_close_params(n + 1 if due else 0, MIN_DIST)
                    left = {}

                    def run_a():
                        device_batch.track_vo_pairs(ctx, pyr, deps, geo, pairs, rows, prm, cfg, tp, klt, out=res)
                        device_batch.track_close_pairs(ctx, tc, orb, slots, res.rows, cand, frame0, ctp, out=closed)

                    def run_b():
                        device_batch.track_vo_pairs(ctx, pyr, deps, geo, pairs, rows, prm, cfg, tp, klt, out=res_b)
                        torch.cuda.synchronize()
                        h = res_b.rows.download()
                        merged = {k: np.zeros((P, ocap) + h[k].shape[2:], h[k].dtype) for k in NAMES}
                        level, src, count = np.zeros((P, ocap), np.int32), np.zeros((P, ocap), np.int32), np.zeros(P, np.int32)
                        for p in range(P):
                            k = int(h["counts"][p])
                            acc = host_merge(h["xy_undist"][p, :k], hc["xy_undist"][0, :nc], bound) if k < ctp.minimalTrackedFeatures else np.zeros(0, np.int64)
                            m = k + len(acc)
                            for name in NAMES:
                                merged[name][p, :k] = h[name][p, :k]
                                merged[name][p, k:m] = hc[name][0][acc]
                            src[p, :k], src[p, k:m], count[p] = np.arange(k), n + acc, m
                            with np.errstate(all="ignore"):
                                x = powers[merged["octave"][p, :m]] * merged["det_dist"][p, :m] / norm3(merged["pts"][p, :m])
                            lv = (x[:, None] >= thresholds[None, :]).sum(axis=1)
                            level[p, :m] = np.where(np.isfinite(x), lv, 0)
                        up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
                        desc, kept, num = device_batch.describe_features_batch(ctx, orb, slots, up(merged["xy"]), up(merged["angle"]), up(level),
                                                                               up(count))
                        torch.cuda.synchronize()
                        hk, hn, hd = kept.cpu().numpy(), num.cpu().numpy(), desc.cpu().numpy()
                        rows_b = {name: [merged[name][p][hk[p, :hn[p]]] for p in range(P)] for name in NAMES}
                        left.update(rows=rows_b, src=[src[p][hk[p, :hn[p]]] for p in range(P)], num=hn, desc=hd, merged=count)

                    run_a(), run_b()
                    ta, tb = [], []
                    for _ in range(REPS):
                        ta.append(wall_ms(run_a))
                        tb.append(wall_ms(run_b))
                    got = closed.download()
                    assert got["rows"]["counts"].tolist() == left["num"].tolist()
                    for p in range(P):
                        k = int(left["num"][p])
                        assert got["desc"][p, :k].tobytes() == left["desc"][p, :k].tobytes(), p
                        assert got["src_idx"][p, :k].tobytes() == left["src"][p].astype(np.int32).tobytes(), p
                        for name in NAMES:
                            assert got["rows"][name][p, :k].tobytes() == left["rows"][name][p].tobytes(), (p, name)
                    assert got["refill"].tolist() == [1 if due else 0] * P
                    # (c)
                    run_pass = lambda mask: device_batch.track_close_pairs(ctx, tc, orb, slots, res.rows, cand, frame0, ctp, out=closed, passes=mask)   # noqa: E731
                    tm, tg = [ev_ms(lambda: run_pass(1)) for _ in range(REPS)], [ev_ms(lambda: run_pass(8)) for _ in range(REPS)]
                    a_med, b_med = sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]
                    kk, mm = left["num"], left["merged"]
                    lines = ["%3d pairs x %3d points, %s (%d candidates): %d .. %d merged rows, %d .. %d closed (same rows, descriptors and "
                             "source indices from (a) and (b))" % (P, n, "refill" if due else "no refill", nc, mm.min(), mm.max(), kk.min(), kk.max()),
                             "    (a) ps_track_vo_pairs + ps_track_close_pairs  %s   %9.2f us a pair" % (fmt(ta), a_med * 1e3 / P),
                             "    (b) control: first half + host loop           %s   %9.2f us a pair   (b) / (a) = %.2f" % (fmt(tb), b_med * 1e3 / P, b_med / a_med),
                             "    (c) ps_track_merge_rows alone                 %s" % fmt(tm),
                             "        ps_close_tracked_rows alone               %s" % fmt(tg), ""]
                    for line in lines:
                        print(line, flush=True)
                    out.extend(lines)
                tc.close()
        for h in (pyr, orb, fe):
            h.close()
    if args:
        open(args[0], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
