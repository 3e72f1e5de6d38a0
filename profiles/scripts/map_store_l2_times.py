"""The resident store with float descriptor rows (ps_map_views_l2_device, ps_pose_sets_l2_device, ps_loop_pairs_l2_device;
ps_map_store_f32.h) in one process, alternating regions, medians of five, for dim 64 and 128:
 views   499 views x 2000 candidates (ten observations a feature), the views then matched against 499 frames of 400 keypoints:
   (a) ps_map_views_l2_device, alone and followed by ps_map_pairs_l2_device;
   (b) ps_map_views_device on the same index arrays (32-byte rows);
   (c) the host path (a) replaces: a numpy gather of every view's rows (the chosen observations precomputed -- kinder than
       walking the map), the upload of desc / pts / level / nkpts, then the same ps_map_pairs_l2_device.
 loops   50 candidates that share the current pose, sets of 100 / 500 / 2000 features, ten true loops, E0 / RANSAC, H = 1157:
   (a) ps_pose_sets_l2_device + ps_loop_pairs_l2_device;
   (b) ps_pose_sets_device + ps_loop_pairs_device on the same index arrays;
   (c) per candidate a numpy gather of both sets, ps_match_l2_f32 and ps_ransac_rigid3d with seed + l (host pointers).
Every GPU step runs under a time limit of its own: a step that exceeds it ends the process (status 124), nothing is started after it.
Usage: python profiles/scripts/map_store_l2_times.py [output file]"""
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import loop_closure_ref as lref  # noqa: E402
import map_store_f32_ref as fref  # noqa: E402
import map_view_ref as vref  # noqa: E402
from putslam_amd import api  # noqa: E402
from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, PS_VIEW_REQUIRE_VISIBLE, TUM_FR1_K, PsMapViewRequest,  # noqa: E402
                              PsPoseSetRequest, default_ransac_params, make_config)

H_LC, L, V, NCAND, NFRAME = 1157, 50, 499, 2000, 400


class limit:
    """with limit(seconds, what): the block is one GPU step; past its limit the process ends at once."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self.expired, (what, seconds))
        self.t.daemon = True

    @staticmethod
    def expired(what, seconds):
        sys.stderr.write("map_store_l2_times: '%s' exceeded its limit of %d s\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def medians(steps, seconds, regions=5):
    """steps: dict name -> callable; every region runs each once, in turn.  Medians in seconds."""
    ts = {k: [] for k in steps}
    for r in range(regions + 1):                   # (the first region warms up and is dropped)
        for k, f in steps.items():
            with limit(seconds, k):
                t = time.perf_counter()
                f()
                dt = time.perf_counter() - t
            if r:
                ts[k].append(dt)
    return {k: float(np.median(v)) for k, v in ts.items()}


# ---------------------------------------------------------------- views
def views(ctx, dim, out):
    import torch
    from putslam_amd.device_batch import FrameSetF32Device, MapBatchF32Device, MapStoreDevice, MapViewsDevice, MapViewsF32Device
    rng = np.random.default_rng(dim)
    store, cam_inv, ang, cand, cc = vref.timing_scene(NCAND, V, seed=V)
    fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), dim))
    sd = fref.store_device(fs)
    sb = MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                        store["obs_det_dist"], store["num_poses"])
    dev = sd.device
    d = dict(cam=np.ascontiguousarray(cam_inv.transpose(0, 2, 1)).reshape(-1, 16), ang=np.ascontiguousarray(ang), cand=cand, cc=cc)
    d = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    rq = PsMapViewRequest()
    rq.camInv, rq.poseAngle, rq.cand, rq.candCounts = (d[k].data_ptr() for k in ("cam", "ang", "cand", "cc"))
    rq.maxAngle, rq.fx, rq.fy, rq.cx, rq.cy, rq.imageW, rq.imageH = (0.5,) + vref.K_TUM + vref.IMAGE
    rq.V, rq.candCapacity, rq.flags = V, NCAND, PS_VIEW_REQUIRE_VISIBLE
    vf, vb = MapViewsF32Device(V, NCAND, dim, dev), MapViewsDevice(V, NCAND, dev)
    st_f, os_f, st_b, os_b = sd.view(), vf.out_struct(), sb.view(), vb.out_struct()
    torch.cuda.synchronize()
    with limit(120, "first views call"):
        ctx.map_views_l2_device(st_f, rq, os_f)
        ctx.synchronize()
    g = vf.download()
    nk = g["nkpts"].astype(np.int64)
    # frames near the views; the host path's inputs: the chosen observations, the points and the levels, precomputed
    fdesc, fpts = np.zeros((V, NFRAME, dim), np.float32), np.zeros((V, NFRAME, 3), np.float32)
    flev, fn = np.zeros((V, NFRAME), np.int32), np.minimum(nk, NFRAME).astype(np.int32)
    for v in range(V):
        if fn[v] == 0:
            continue
        src = rng.choice(nk[v], fn[v], replace=False)
        fdesc[v, :fn[v]] = g["desc"][v, src] + rng.normal(0, 0.01, (fn[v], dim)).astype(np.float32)
        fpts[v, :fn[v]] = g["pts"][v, src] + rng.normal(0, 0.01, (fn[v], 3)).astype(np.float32)
        flev[v, :fn[v]] = g["mapLevel"][v, src]
    frames = FrameSetF32Device(fdesc, fpts, fn)
    pairs = np.stack([np.arange(V), np.arange(V)], axis=1).astype(np.int32)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    batch_dev = MapBatchF32Device(vf, vf.map_level, frames, flev, pairs, NCAND)
    h = dict(desc=np.zeros((V, NCAND, dim), np.float32), pts=g["pts"].copy(), level=g["mapLevel"].copy(), nkpts=g["nkpts"].copy())
    up = FrameSetF32Device(h["desc"], h["pts"], h["nkpts"])
    up_level = torch.zeros((V, NCAND), dtype=torch.int32, device=dev)
    batch_host = MapBatchF32Device(up, up_level, frames, flev, pairs, NCAND)
    obs, rows = g["obsIdx"], fs["rows"]
    bv_d, bv_h = batch_dev.batch_view(), batch_host.batch_view()
    rv_d, rv_h = batch_dev.view(), batch_host.view()
    torch.cuda.synchronize()

    def a_views():
        ctx.map_views_l2_device(st_f, rq, os_f)
        ctx.synchronize()

    def a_chain():
        ctx.map_views_l2_device(st_f, rq, os_f)
        ctx.map_pairs_l2_device(prm, cfg, TUM_FR1_K, bv_d, rv_d)
        ctx.synchronize()

    def b_views():
        ctx.map_views_device(st_b, rq, os_b)
        ctx.synchronize()

    def c_gather():
        for v in range(V):
            h["desc"][v, :nk[v]] = rows[obs[v, :nk[v]]]
        up.desc.copy_(torch.from_numpy(h["desc"]))
        up.pts.copy_(torch.from_numpy(h["pts"]))
        up_level.copy_(torch.from_numpy(h["level"]))
        up.nkpts.copy_(torch.from_numpy(h["nkpts"]))
        torch.cuda.synchronize()

    def c_chain():
        c_gather()
        ctx.map_pairs_l2_device(prm, cfg, TUM_FR1_K, bv_h, rv_h)
        ctx.synchronize()

    ctx.set_stream(0)
    m = medians(dict(a_views=a_views, a_chain=a_chain, b_views=b_views, c_gather=c_gather, c_chain=c_chain), 120)
    ga, gh = batch_dev.download(), batch_host.download()
    same = ga["numMatches"].tobytes() == gh["numMatches"].tobytes() and ga["pose"].tobytes() == gh["pose"].tobytes()
    out.append("views, dim %3d, %d views x %d candidates (%d kept on average), frames of %d: (a) ps_map_views_l2_device %.3f ms "
               "(%.2f us/view), + ps_map_pairs_l2_device %.3f ms; (b) ps_map_views_device on the same index arrays %.3f ms (%.2f us/view); "
               "(c) numpy gather + upload %.1f ms, + ps_map_pairs_l2_device %.1f ms; (c)/(a) chain = %.1f; %s"
               % (dim, V, NCAND, int(nk.mean()), NFRAME, m["a_views"] * 1e3, m["a_views"] / V * 1e6, m["a_chain"] * 1e3,
                  m["b_views"] * 1e3, m["b_views"] / V * 1e6, m["c_gather"] * 1e3, m["c_chain"] * 1e3, m["c_chain"] / m["a_chain"],
                  "both chains give the same bytes" if same else "THE CHAINS DISAGREE"))


# ---------------------------------------------------------------- loops
def loop_scene(n, dim, seed):
    """profiles/scripts/loop_pairs_times.py's scene (51 poses of n features over a pool of 8 n, poses 1 .. 10 true loops of pose
    0) with float rows beside the binary ones: a true loop's rows are the current pose's plus small Gaussian noise."""
    rng = np.random.default_rng(seed)
    F, S = 8 * n, L + 1
    cur = np.sort(rng.choice(F, n, replace=False))
    feat, pose, desc, rows, pts = [], [], [], [], []
    d0, r0, p0 = rng.integers(0, 256, (n, 32), dtype=np.uint8), fref.unit_rows(rng, n, dim), lref.random_points3d(rng, n)
    for q in range(S):
        if q == 0:
            f, d, r, p = cur, d0, r0, p0
        elif q <= 10:
            R, t = vref.rotation(rng.normal(size=3), rng.uniform(0.02, 0.2)), rng.uniform(-0.3, 0.3, 3)
            f, d = cur, d0 ^ np.packbits(rng.random((n, 256)) < 0.08, axis=1)
            r = (r0 + rng.normal(0, 0.02 / np.sqrt(dim), (n, dim))).astype(np.float32)
            p = p0 @ R.T + t + rng.normal(0, 0.003, (n, 3))
        else:
            f, d = np.sort(rng.choice(F, n, replace=False)), rng.integers(0, 256, (n, 32), dtype=np.uint8)
            r, p = fref.unit_rows(rng, n, dim), lref.random_points3d(rng, n)
        feat.append(f)
        pose.append(np.full(n, q))
        desc.append(d)
        rows.append(r)
        pts.append(p)
    feat, pose, desc, rows, pts = (np.concatenate(x) for x in (feat, pose, desc, rows, pts))
    order = np.lexsort((pose, feat))
    start = np.zeros(F + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(feat, minlength=F))
    O = len(order)
    store = dict(pos=rng.uniform(-2, 2, (F, 3)), obs_start=start, obs_pose=pose[order].astype(np.int32), obs_desc=desc[order],
                 obs_octave=np.zeros(O, np.int32), obs_det_dist=np.ones(O), num_poses=S)
    return fref.float_store(store, rows[order]), pts[order], np.stack([np.zeros(L, np.int32), np.arange(1, S, dtype=np.int32)], axis=1)


def host_path(ctx, fs, p3d, members, cand, prm, seed):
    closed = 0
    for l, (qa, qb) in enumerate(cand):
        ia, ib = members[qa], members[qb]
        if not (len(ia) > 35 and len(ib) > 35) or len(ia) < 10 or len(ib) < 10:
            continue
        m = ctx.match_l2(fs["rows"][ia], fs["rows"][ib])
        if len(m) == 0:
            continue
        cfg, _ = make_config(EST_RANSAC, H_LC, seed=seed + l)
        r = ctx.ransac_rigid3d(prm, cfg, TUM_FR1_K, p3d[ia].astype(np.float32), p3d[ib].astype(np.float32), m)
        closed += float(r["stats"]["pointInlierRatio"]) > 0.4
    return closed


def loops(ctx, dim, n, out):
    import torch
    from putslam_amd.device_batch import LoopBatchDevice, LoopBatchF32Device, PoseSetsDevice, PoseSetsF32Device
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, _ = make_config(EST_RANSAC, H_LC, seed=11)
    fs, p3d, cand = loop_scene(n, dim, n + dim)
    poses = np.arange(L + 1, dtype=np.int32)
    members = [np.nonzero(fs["obs_pose"] == q)[0] for q in poses]
    sd, sb = fref.store_device(fs), lref.store_device(fs)
    p3d_d, poses_d = torch.from_numpy(p3d).to(sd.device), torch.from_numpy(poses).to(sd.device)
    rq = PsPoseSetRequest(p3d_d.data_ptr(), poses_d.data_ptr(), L + 1, 0)
    sets_f, sets_b = PoseSetsF32Device(L + 1, n, dim, sd.device), PoseSetsDevice(L + 1, n, sd.device)
    bf, bb = LoopBatchF32Device(sets_f, cand), LoopBatchDevice(sets_b, cand)
    st_f, os_f, st_b, os_b = sd.view(), sets_f.out_struct(), sb.view(), sets_b.out_struct()
    b_f, r_f, b_b, r_b = bf.batch_struct(), bf.results_struct(), bb.batch_struct(), bb.results_struct()
    torch.cuda.synchronize()
    closed = []

    def a_sets():
        ctx.pose_sets_l2_device(st_f, rq, os_f)
        ctx.synchronize()

    def a_both():
        ctx.pose_sets_l2_device(st_f, rq, os_f)
        ctx.loop_pairs_l2_device(prm, cfg, TUM_FR1_K, b_f, r_f)
        ctx.synchronize()

    def b_sets():
        ctx.pose_sets_device(st_b, rq, os_b)
        ctx.synchronize()

    def b_both():
        ctx.pose_sets_device(st_b, rq, os_b)
        ctx.loop_pairs_device(prm, cfg, TUM_FR1_K, b_b, r_b)
        ctx.synchronize()

    ctx.set_stream(0)
    m = medians(dict(a_sets=a_sets, a_both=a_both, b_sets=b_sets, b_both=b_both,
                     c_host=lambda: closed.append(host_path(ctx, fs, p3d, members, cand, prm, 11))), 180)
    g = bf.download()
    agree = "both sides close %d" % closed[-1] if int(g["closed"].sum()) == closed[-1] else \
        "THE SIDES DISAGREE: host %d, device %d closed" % (closed[-1], int(g["closed"].sum()))
    out.append("loops, dim %3d, %4d features a set, %d candidates (10 true loops): (a) ps_pose_sets_l2_device + ps_loop_pairs_l2_device "
               "%.3f ms (%.1f us a candidate; the sets alone %.3f ms); (b) the binary calls on the same index arrays %.3f ms (the sets "
               "alone %.3f ms); (c) host gather + ps_match_l2_f32 + ps_ransac_rigid3d per candidate %.2f ms; (c)/(a) = %.1f; %s"
               % (dim, n, L, m["a_both"] * 1e3, m["a_both"] / L * 1e6, m["a_sets"] * 1e3, m["b_both"] * 1e3, m["b_sets"] * 1e3,
                  m["c_host"] * 1e3, m["c_host"] / m["a_both"], agree))


def main():
    ctx = api.Context(0)
    out = []
    for dim in (64, 128):
        views(ctx, dim, out)
        for n in (100, 500, 2000):
            loops(ctx, dim, n, out)
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
        open(sys.argv[1], "w").write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
