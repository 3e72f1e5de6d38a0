"""Loop-closure candidates verified in one batch (ps_pose_sets_device + ps_loop_pairs_device, ps_loop_closure.h) against the host
path they replace, in one process, alternating regions, medians of five: 50 candidates that share the current pose (FABMAP's
queue), sets of 100, 500 and 2000 features, ten of the 50 true loops, E0 / RANSAC with H = 1157.
 (a) per candidate, through the same build's single-pair calls: the two gates, a host gather of both feature sets (numpy, the
     observation indices of every pose precomputed -- kinder than the reference's copy of whole MapFeatures under a mutex),
     ps_match_hamming256 and ps_ransac_rigid3d with seed + l (host pointers: upload, kernels, download);
 (b) the two device calls on the resident store, call -> synchronised, output blocks allocated beforehand; each call alone too.
 (c) ps_pose_sets_device alone on a store of 2^20 features (four observations each, 400 poses) with S = 1 and S = 100: the
     store is read twice whatever S is.
Usage: python profiles/scripts/loop_pairs_times.py [output file]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import loop_closure_ref as lref  # noqa: E402
import map_view_ref as vref  # noqa: E402
from putslam_amd import api  # noqa: E402
from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402

H_LC, L = 1157, 50


def scene(n, seed):
    """51 poses of n features each over a pool of 8 n features: pose 0 is the current one, poses 1 .. 10 are true loops of it
    (the same features, points under a rigid motion + 3 mm, 8 % of the descriptor bits flipped), poses 11 .. 50 unrelated."""
    rng = np.random.default_rng(seed)
    F, S = 8 * n, L + 1
    cur = np.sort(rng.choice(F, n, replace=False))
    feat, pose, desc, pts = [], [], [], []
    d0, p0 = rng.integers(0, 256, (n, 32), dtype=np.uint8), lref.random_points3d(rng, n)
    for q in range(S):
        if q == 0:
            f, d, p = cur, d0, p0
        elif q <= 10:
            R, t = vref.rotation(rng.normal(size=3), rng.uniform(0.02, 0.2)), rng.uniform(-0.3, 0.3, 3)
            f, d, p = cur, d0 ^ np.packbits(rng.random((n, 256)) < 0.08, axis=1), p0 @ R.T + t + rng.normal(0, 0.003, (n, 3))
        else:
            f, d, p = np.sort(rng.choice(F, n, replace=False)), rng.integers(0, 256, (n, 32), dtype=np.uint8), lref.random_points3d(rng, n)
        feat.append(f)
        pose.append(np.full(n, q))
        desc.append(d)
        pts.append(p)
    feat, pose, desc, pts = np.concatenate(feat), np.concatenate(pose), np.concatenate(desc), np.concatenate(pts)
    order = np.lexsort((pose, feat))                               # feature-major, ascending pose id
    start = np.zeros(F + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(feat, minlength=F))
    O = len(order)
    store = dict(pos=rng.uniform(-2, 2, (F, 3)), obs_start=start, obs_pose=pose[order].astype(np.int32), obs_desc=desc[order],
                 obs_octave=np.zeros(O, np.int32), obs_det_dist=np.ones(O), num_poses=S)
    return store, pts[order], np.stack([np.zeros(L, np.int32), np.arange(1, S, dtype=np.int32)], axis=1)


def host_path(ctx, store, p3d, members, cand, prm, seed):
    """(a): the loop of FeaturesMap::loopClosure over the queue, one candidate at a time."""
    closed = 0
    for l, (qa, qb) in enumerate(cand):
        ia, ib = members[qa], members[qb]
        if not (len(ia) > 35 and len(ib) > 35) or len(ia) < 10 or len(ib) < 10:
            continue
        da, db = store["obs_desc"][ia], store["obs_desc"][ib]
        pa, pb = p3d[ia].astype(np.float32), p3d[ib].astype(np.float32)
        m = ctx.match_hamming256(da, db)
        if len(m) == 0:
            continue
        cfg, _ = make_config(EST_RANSAC, H_LC, seed=seed + l)
        r = ctx.ransac_rigid3d(prm, cfg, TUM_FR1_K, pa, pb, m)
        closed += float(r["stats"]["pointInlierRatio"]) > 0.4
    return closed


def medians(fa, fb, regions=5):
    fa()
    fb()
    a, b = [], []
    for _ in range(regions):
        t = time.perf_counter()
        fa()
        a.append(time.perf_counter() - t)
        t = time.perf_counter()
        fb()
        b.append(time.perf_counter() - t)
    return float(np.median(a)), float(np.median(b))


def timed(f, reps=7):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    import torch
    from putslam_amd._abi import PsPoseSetRequest
    from putslam_amd.device_batch import LoopBatchDevice, PoseSetsDevice
    ctx = api.Context(0)
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=11)
    out = []
    for n in (100, 500, 2000):
        store, p3d, cand = scene(n, n)
        poses = np.arange(L + 1, dtype=np.int32)
        members = [np.nonzero(store["obs_pose"] == q)[0] for q in poses]
        sd = lref.store_device(store)
        p3d_d, poses_d = torch.from_numpy(p3d).to(sd.device), torch.from_numpy(poses).to(sd.device)
        sets = PoseSetsDevice(L + 1, n, sd.device)
        batch = LoopBatchDevice(sets, cand)
        st, rq, os_ = sd.view(), PsPoseSetRequest(p3d_d.data_ptr(), poses_d.data_ptr(), L + 1, 0), sets.out_struct()
        b_, r_ = batch.batch_struct(), batch.results_struct()
        torch.cuda.synchronize()

        def dev_sets():
            ctx.pose_sets_device(st, rq, os_)
            ctx.synchronize()

        def dev_pairs():
            ctx.loop_pairs_device(prm, cfg, TUM_FR1_K, b_, r_)
            ctx.synchronize()

        def dev_both():
            ctx.pose_sets_device(st, rq, os_)
            ctx.loop_pairs_device(prm, cfg, TUM_FR1_K, b_, r_)
            ctx.synchronize()

        closed = []
        a, b = medians(lambda: closed.append(host_path(ctx, store, p3d, members, cand, prm, 11)), dev_both)
        g = batch.download()
        agree = "both sides close %d" % closed[-1] if int(g["closed"].sum()) == closed[-1] else \
            "THE SIDES DISAGREE: host %d, device %d closed" % (closed[-1], int(g["closed"].sum()))
        out.append("%4d features a set, %d candidates sharing the current pose (10 true loops): (a) host gather + single-pair calls "
                   "%.2f ms (%.0f us a candidate), (b) ps_pose_sets_device + ps_loop_pairs_device %.3f ms (%.1f us a candidate; the "
                   "sets alone %.3f ms, the verifier alone %.3f ms), (a)/(b) = %.1f; %s"
                   % (n, L, a * 1e3, a / L * 1e6, b * 1e3, b / L * 1e6, timed(dev_sets) * 1e3, timed(dev_pairs) * 1e3, a / b, agree))
    # (c) the read cost does not grow with S
    rng = np.random.default_rng(20)
    store = vref.make_store(rng, 1 << 20, 400, obs_per_feature=4)
    sd = lref.store_device(store)
    p3d_d = torch.from_numpy(lref.random_points3d(rng, len(store["obs_pose"]))).to(sd.device)
    st = sd.view()
    for S in (1, 100):
        poses_d = torch.arange(S, dtype=torch.int32, device=sd.device)
        sets = PoseSetsDevice(S, 16384, sd.device)
        rq, os_ = PsPoseSetRequest(p3d_d.data_ptr(), poses_d.data_ptr(), S, 0), sets.out_struct()
        torch.cuda.synchronize()

        def call():
            ctx.pose_sets_device(st, rq, os_)
            ctx.synchronize()

        t = timed(call)
        cnt = sets.set_count.cpu().numpy()[:S]
        assert (cnt > 0).all()
        out.append("store of 2^20 features x 4 observations, 400 poses: ps_pose_sets_device with S = %3d (%d members a set on average) "
                   "%.3f ms" % (S, int(cnt.mean()), t * 1e3))
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        open(sys.argv[1], "w").write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
