"""CPU answer and scenes for the device-built map views (ps_map_views_device / ps_frame_levels_device / ps_view_angles).

`build_view` is a sequential restatement of what the reference's host does per frame and per visible map feature, in the
reference's loop order with its roundings: FeaturesMap::findNearestFrame (src/Map/featuresMap.cpp:528-563),
PUTSLAM::removeMapFeaturesWithoutGoodObservationAngle (src/PUTSLAM/PUTSLAM.cpp:932-950), moveMapFeaturesToLocalCordinateSystem
(PUTSLAM.cpp:28-51), DepthSensorModel::inverseModel (src/Grabber/depthSensorModel.cpp:18-25) and the predicted level of
Matcher::matchXYZ (src/Matcher/matcher.cpp:681-692).  Levels come from ps_predicted_level itself (the host's libm), angles from
math.acos: no thresholds, no tables.  Like every restatement of this project it is RESTATED, not compiled against the real
Eigen / OpenCV: the order of Eigen's 4 x 4 product, of Vector3f's reductions and the acos overload are readings.

`build_view_fast` is a second formulation -- the observation choice as an argmin over a masked (candidates x observations)
matrix, the arithmetic vectorised -- for stores too large for the Python loop; tests/test_map_view_host.py holds the two against
each other.
"""
import math

import numpy as np

from putslam_amd import _lib
from putslam_amd._abi import PS_LEVEL_OCTAVE_MAX, PS_LEVEL_OCTAVE_MIN, PS_VIEW_INVALID

K_TUM = (525.0, 525.0, 319.5, 239.5)
IMAGE = (640.0, 480.0)
K_EDGE = (512.0, 512.0, 320.0, 240.0)     # u = 0 and u = imageW are reached exactly at p0 = -+0.625, p2 = 1


def predicted_level(octave, det_dist, cur_dist):
    return int(_lib.load().ps_predicted_level(int(octave), float(det_dist), float(cur_dist)))


# ---------------------------------------------------------------- angles
def view_angles(cur_pose, poses):
    """featuresMap.cpp:534-556: the view vectors are the third rotation columns (featureGlob has an identity rotation), float
    casts, Vector3f dot / norm summed a0*b0 + (a1*b1 + a2*b2), acos in double."""
    f = np.float32
    out = np.zeros(len(poses), np.float64)
    with np.errstate(all="ignore"):
        a = [f(cur_pose[i][2]) for i in range(3)]
        na = np.sqrt(f(a[0] * a[0]) + f(f(a[1] * a[1]) + f(a[2] * a[2])))
        for q, P in enumerate(poses):
            b = [f(P[i][2]) for i in range(3)]
            dot = f(b[0] * a[0]) + f(f(b[1] * a[1]) + f(b[2] * a[2]))
            nb = np.sqrt(f(b[0] * b[0]) + f(f(b[1] * b[1]) + f(b[2] * b[2])))
            r = float(f(dot / f(nb * na)))
            out[q] = abs(math.acos(r)) if -1.0 <= r <= 1.0 else float("nan")      # (C's acos: NaN outside [-1, 1] and for NaN)
    return out


# ---------------------------------------------------------------- one view, sequentially
def _rows(store, feat, obs, p, uv, ang, level):
    n = len(feat)
    obs = np.asarray(obs, np.int32).reshape(n)
    p = np.asarray(p, np.float64).reshape(n, 3)
    return dict(featIdx=np.asarray(feat, np.int32).reshape(n), obsIdx=obs, posCam=p, uv=np.asarray(uv, np.float64).reshape(n, 2),
                angle=np.asarray(ang, np.float64).reshape(n), mapLevel=np.asarray(level, np.int32).reshape(n),
                pts=p.astype(np.float32), desc=store["obs_desc"][obs].reshape(n, 32))


def build_view(store, M, ang, max_angle, K, image, cand, require_visible):
    """Rows of one view in candidate order, or None for an invalid view (a candidate index outside the store, a pose id outside
    the table, a malformed observation range, an emitted feature whose octave lies outside the level table)."""
    pos, start, pose_of = store["pos"], store["obs_start"], store["obs_pose"]
    F, O, N = len(pos), len(pose_of), store["num_poses"]
    fx, fy, cx, cy = (np.float64(x) for x in K)
    W, H = np.float64(image[0]), np.float64(image[1])
    M = np.asarray(M, np.float64)
    feat, obs, ps, uvs, angs, lvls = [], [], [], [], [], []
    bad = False
    with np.errstate(all="ignore"):
        for f in cand:
            f = int(f)
            if f < 0 or f >= F:
                bad = True
                continue
            s, e = int(start[f]), int(start[f + 1])
            if s < 0 or e < s or e > O:
                bad = True
                continue
            best, chosen = 10.0, -1                       # featuresMap.cpp:537
            for o in range(s, e):                         # :543, the std::map's order
                q = int(pose_of[o])
                if q < 0 or q >= N:
                    bad = True
                    continue
                a = float(ang[q])
                if a < best:                              # :552
                    best, chosen = a, o
            if chosen < 0 or best > max_angle:            # :558-561, PUTSLAM.cpp:940
                continue
            x, y, z = pos[f]
            p = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]      # PUTSLAM.cpp:38-40
            u = ((fx * p[0]) / p[2]) + cx                 # depthSensorModel.cpp:20
            v = ((fy * p[1]) / p[2]) + cy
            if u < 0 or u > W or v < 0 or v > H or p[2] < 0.8 or p[2] > 6.0:
                u = v = np.float64(-1.0)
            if require_visible and u == -1:               # featuresMap.cpp:474
                continue
            octave = int(store["obs_octave"][chosen])
            if octave < PS_LEVEL_OCTAVE_MIN or octave > PS_LEVEL_OCTAVE_MAX:
                bad = True
                continue
            cur = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])       # matcher.cpp:685-687
            feat.append(f)
            obs.append(chosen)
            ps.append(p)
            uvs.append((u, v))
            angs.append(best)
            lvls.append(predicted_level(octave, store["obs_det_dist"][chosen], cur))
    return None if bad else _rows(store, feat, obs, ps, uvs, angs, lvls)


def build_view_fast(store, M, ang, max_angle, K, image, cand, require_visible):
    """The same answer, formulated differently: the chosen observation is the argmin of a (candidates x observations) matrix in
    which absent entries, NaNs and angles not below 10 are masked out (numpy's argmin returns the first minimum: the strict
    comparison of the walk)."""
    pos, start, pose_of = store["pos"], store["obs_start"].astype(np.int64), store["obs_pose"]
    F, O, N = len(pos), len(pose_of), store["num_poses"]
    cand = np.asarray(cand, np.int64)
    if len(cand) == 0:
        return _rows(store, [], [], [], [], [], [])
    if (cand < 0).any() or (cand >= F).any():
        return None
    s, e = start[cand], start[cand + 1]
    if (s < 0).any() or (e < s).any() or (e > O).any():
        return None
    cnt = e - s
    width = max(int(cnt.max()), 1)
    k = np.arange(width)[None, :]
    there = k < cnt[:, None]
    idx = np.where(there, s[:, None] + k, 0)
    q = pose_of[idx] if O else np.zeros_like(idx)
    if (there & ((q < 0) | (q >= N))).any():
        return None
    with np.errstate(all="ignore"):
        a = np.asarray(ang, np.float64)[np.clip(q, 0, max(N - 1, 0))] if N else np.full(idx.shape, np.nan)
        A = np.where(there & (a < 10.0), a, np.inf)
        j = np.argmin(A, axis=1)
        rows = np.arange(len(cand))
        best = A[rows, j]
        keep = (best < np.inf) & ~(best > max_angle)
        chosen = idx[rows, j]
        x, y, z = pos[cand, 0], pos[cand, 1], pos[cand, 2]
        M = np.asarray(M, np.float64)
        p = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]
        u = ((np.float64(K[0]) * p[0]) / p[2]) + np.float64(K[2])
        v = ((np.float64(K[1]) * p[1]) / p[2]) + np.float64(K[3])
        out = (u < 0) | (u > image[0]) | (v < 0) | (v > image[1]) | (p[2] < 0.8) | (p[2] > 6.0)
        u, v = np.where(out, -1.0, u), np.where(out, -1.0, v)
        if require_visible:
            keep &= ~(u == -1)
        cur = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
    sel = np.nonzero(keep)[0]
    ch = chosen[sel]
    octave = store["obs_octave"][ch]
    if ((octave < PS_LEVEL_OCTAVE_MIN) | (octave > PS_LEVEL_OCTAVE_MAX)).any():
        return None
    det = store["obs_det_dist"][ch]
    L = _lib.load()
    lv = [L.ps_predicted_level(int(o), float(d), float(c)) for o, d, c in zip(octave, det, cur[sel])]
    return _rows(store, cand[sel], ch, np.stack([p[0][sel], p[1][sel], p[2][sel]], axis=1), np.stack([u[sel], v[sel]], axis=1),
                 best[sel], lv)


def build_views(store, cam_inv, pose_angle, max_angle, K, image, max_kpts, cand=None, cand_counts=None, require_visible=False,
                fast=False):
    """One answer per view: dict(viewCount, nkpts, rows or None).  cand (V, capacity) + cand_counts (V,), or None = every
    feature in index order."""
    one = build_view_fast if fast else build_view
    out = []
    for v in range(len(cam_inv)):
        if cand is None:
            c = np.arange(len(store["pos"]))
        else:
            n = int(cand_counts[v])
            if n < 0 or n > cand.shape[1]:
                out.append(dict(viewCount=PS_VIEW_INVALID, nkpts=0, rows=None))
                continue
            c = cand[v, :n]
        rows = one(store, cam_inv[v], pose_angle[v], max_angle, K, image, c, require_visible)
        if rows is None:
            out.append(dict(viewCount=PS_VIEW_INVALID, nkpts=0, rows=None))
        elif len(rows["featIdx"]) > max_kpts:
            out.append(dict(viewCount=-len(rows["featIdx"]), nkpts=0, rows=None))
        else:
            out.append(dict(viewCount=len(rows["featIdx"]), nkpts=len(rows["featIdx"]), rows=rows))
    return out


ROW_KEYS = ("desc", "pts", "mapLevel", "featIdx", "obsIdx", "posCam", "uv", "angle")


def compare(got, want, what=""):
    """got: MapViewsDevice.download(); want: build_views' list.  Bytes, rows up to the count."""
    assert len(got["viewCount"]) >= len(want)
    for v, w in enumerate(want):
        tag = (what, v)
        assert int(got["viewCount"][v]) == w["viewCount"], (tag, int(got["viewCount"][v]), w["viewCount"])
        assert int(got["nkpts"][v]) == w["nkpts"], (tag, int(got["nkpts"][v]), w["nkpts"])
        n = w["nkpts"]
        if n:
            for k in ROW_KEYS:
                assert got[k][v, :n].tobytes() == w["rows"][k].tobytes(), (tag, k)


def rows_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(a[k].tobytes() == b[k].tobytes() for k in ROW_KEYS)


# ---------------------------------------------------------------- the frame side
def frame_levels(pts, nkpts, octave, det_dist):
    """matcher.cpp:639-652 with curDist = Vector3f::norm in float; -1 for an octave outside the level table; rows beyond a
    frame's count are left at the marker -9."""
    f = np.float32
    out = np.full(octave.shape, -9, np.int32)
    for fr in range(pts.shape[0]):
        for i in range(int(nkpts[fr])):
            p = pts[fr, i]
            with np.errstate(all="ignore"):
                nrm = np.sqrt(f(p[0] * p[0]) + f(f(p[1] * p[1]) + f(p[2] * p[2])))
            o = int(octave[fr, i])
            ok = PS_LEVEL_OCTAVE_MIN <= o <= PS_LEVEL_OCTAVE_MAX
            out[fr, i] = predicted_level(o, det_dist[fr, i], float(nrm)) if ok else -1
    return out


# ---------------------------------------------------------------- scenes
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def make_poses(rng, n, max_rot=0.7, max_shift=0.4):
    P = np.zeros((n, 4, 4))
    for i in range(n):
        P[i] = np.eye(4)
        P[i, :3, :3] = rotation(rng.normal(size=3), rng.uniform(0, max_rot))
        P[i, :3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return P


def make_store(rng, F, num_poses, max_obs=12, obs_per_feature=None):
    """A random front-end map: positions in a box in front of the cameras, 0 .. max_obs observations a feature (or exactly
    obs_per_feature) at ascending distinct pose ids, octaves 0 .. 7, detection distances near the feature's depth."""
    pos = np.stack([rng.uniform(-2.5, 2.5, F), rng.uniform(-2.0, 2.0, F), rng.uniform(0.4, 7.0, F)], axis=1)
    cnt = np.full(F, obs_per_feature) if obs_per_feature is not None else rng.integers(0, max_obs + 1, F)
    cnt = np.minimum(cnt, num_poses).astype(np.int64)
    start = np.zeros(F + 1, np.int32)
    start[1:] = np.cumsum(cnt)
    O = int(start[-1])
    # ascending distinct pose ids per feature: a random first id, then random positive steps that stay inside the table
    for_f = np.repeat(np.arange(F), cnt)
    pose = np.zeros(O, np.int32)
    if O:
        width = int(cnt.max())
        step = max(1, (num_poses - 1) // max(width, 1))
        inc = rng.integers(1, step + 1, O).astype(np.int64)
        cum = np.cumsum(inc)
        first_of = start[:-1][for_f].astype(np.int64)
        rel = cum - cum[first_of]                                  # 0 for a feature's first observation
        span = np.zeros(F, np.int64)
        np.maximum.at(span, for_f, rel)
        base = (rng.random(F) * (num_poses - span)).astype(np.int64)
        pose = (base[for_f] + rel).astype(np.int32)
    desc = rng.integers(0, 256, (O, 32), dtype=np.uint8)
    octave = rng.integers(0, 8, O).astype(np.int32)
    det = (np.linalg.norm(pos[for_f], axis=1) * rng.uniform(0.6, 1.6, O)).astype(np.float64)
    return dict(pos=pos, obs_start=start, obs_pose=pose, obs_desc=desc, obs_octave=octave, obs_det_dist=det,
                num_poses=int(num_poses))


def make_request(rng, store, V, poses=None, nan_entries=0):
    """V camera poses near the origin: (cam_inv (V, 4, 4), pose_angle (V, num_poses)) with the angle table of view_angles;
    nan_entries of every view's table are replaced by NaN."""
    N = store["num_poses"]
    poses = make_poses(rng, N) if poses is None else poses
    cams = make_poses(rng, V, max_rot=0.5, max_shift=0.3)
    cam_inv = np.stack([np.linalg.inv(c) for c in cams]) if V else np.zeros((0, 4, 4))
    ang = np.stack([view_angles(c, poses) for c in cams]) if V else np.zeros((0, N))
    for v in range(V):
        if nan_entries and N:
            ang[v, rng.integers(0, N, nan_entries)] = np.nan
    return cam_inv, ang, cams, poses


def ragged_candidates(rng, F, V, capacity, counts=None):
    """(cand (V, capacity) int32 ascending feature ids, cand_counts (V,)); slots beyond a view's count hold -7 (never read)."""
    cand = np.full((V, capacity), -7, np.int32)
    cc = np.zeros(V, np.int32)
    for v in range(V):
        n = int(counts[v]) if counts is not None else int(rng.integers(0, min(capacity, F) + 1))
        cc[v] = n
        cand[v, :n] = np.sort(rng.choice(F, n, replace=False))
    return cand, cc


def frames_from_views(rng, views, sources, nkpts, cap):
    """Frames for the chain test: frame f's keypoints sit near rows of view sources[f] (noise 2 cm), 5 % of the descriptor bits
    flipped, octaves 0 .. 7 and detection distances that put the predicted level within -2 .. 2 of the view's."""
    F = len(nkpts)
    pos = np.zeros((F, cap, 3), np.float32)
    desc = np.zeros((F, cap, 32), np.uint8)
    octave = np.zeros((F, cap), np.int32)
    det = np.ones((F, cap), np.float64)
    for f, n in enumerate(nkpts):
        w = views[sources[f]]
        if n == 0:
            continue
        if w["nkpts"] == 0:
            pos[f, :n] = (rng.uniform(-1, 1, (n, 3)) + [0, 0, 2.5]).astype(np.float32)
            desc[f, :n] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            continue
        src = rng.integers(0, w["nkpts"], n)
        pos[f, :n] = (w["rows"]["pts"][src] + rng.normal(0, 0.02, (n, 3))).astype(np.float32)
        desc[f, :n] = w["rows"]["desc"][src] ^ np.packbits(rng.random((n, 256)) < 0.05, axis=1)
        octave[f, :n] = rng.integers(0, 8, n)
        target = w["rows"]["mapLevel"][src] + rng.integers(-2, 3, n)
        det[f, :n] = np.linalg.norm(pos[f, :n].astype(np.float64), axis=1) * 1.2 ** (target - octave[f, :n] - 0.5)
    return dict(pos=pos, desc=desc, octave=octave, det=det, nkpts=np.asarray(nkpts, np.int32), cap=cap)


def views_as_scene(views, cap):
    """build_views' answers in the layout of tests/map_pairs_ref.py's scenes (pos / desc / level / nkpts / cap)."""
    V = len(views)
    pos = np.zeros((V, cap, 3), np.float32)
    desc = np.zeros((V, cap, 32), np.uint8)
    level = np.zeros((V, cap), np.int32)
    for v, w in enumerate(views):
        n = w["nkpts"]
        if n:
            pos[v, :n], desc[v, :n], level[v, :n] = w["rows"]["pts"], w["rows"]["desc"], w["rows"]["mapLevel"]
    return dict(pos=pos, desc=desc, level=level, nkpts=np.array([w["nkpts"] for w in views], np.int32), cap=cap)


# ---------------------------------------------------------------- level edges
def level_edge_inputs(t, octaves=(0, 3, -2, 7)):
    """(octave, detDist, want) triples whose x = (pow(1.2, octave) * detDist) / 2.0 is exactly t[k] (want "on") or the double
    below it ("below"), for a feature at camera-frame position (0, 0, 2): curDist = sqrt(4) = 2 exactly.  Octave 0 always has
    both (x = detDist / 2 is exact); other octaves are searched over the last places of detDist."""
    out = []
    for k, tk in enumerate(t):
        below = np.nextafter(tk, 0.0)
        for o in octaves:
            T = math.pow(1.2, o)
            d0 = 2.0 * tk / T
            found = {}
            d = d0
            for _ in range(16):
                d = np.nextafter(d, 0.0)
            for _ in range(33):
                x = (T * d) / 2.0
                if x == tk and "on" not in found:
                    found["on"] = d
                if x == below:
                    found["below"] = d
                d = np.nextafter(d, np.inf)
            for kind, dd in found.items():
                out.append((o, float(dd), k, kind))
    return out


# ---------------------------------------------------------------- timing: the host loop the call replaces, and the call
def build_host_loop(outdir):
    """profiles/scripts/map_views_host_loop.cpp (a single-threaded C++ loop over the same store layout) compiled at -O2."""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(outdir), "libmap_views_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(root, "profiles", "scripts", "map_views_host_loop.cpp"),
                           "-o", so])
    lib = C.CDLL(so)
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    lib.host_build_views.argtypes = [vp] * 6 + [i32, vp, vp, i32, vp, vp, i32, i32] + [f64] * 7 + [i32, i32, vp, vp, vp, vp]
    return lib


def timing_scene(n_cand, V, seed, obs=10, num_poses=200):
    """A store of 4 x n_cand features with `obs` observations each, V views with n_cand candidates each."""
    from putslam_amd import api
    rng = np.random.default_rng(seed)
    store = make_store(rng, 4 * n_cand, num_poses, obs_per_feature=obs)
    poses = make_poses(rng, num_poses)
    cams = make_poses(rng, V, max_rot=0.5, max_shift=0.3)
    cam_inv = np.stack([np.linalg.inv(c) for c in cams])
    ang = np.stack([api.view_angles(c, poses) for c in cams])
    cand = np.stack([np.sort(rng.choice(4 * n_cand, n_cand, replace=False)) for _ in range(V)]).astype(np.int32)
    return store, cam_inv, ang, cand, np.full(V, n_cand, np.int32)


class ViewTiming:
    """(a) the host loop + the upload of the views it built (pageable buffers into preallocated device tensors, synchronised);
    (b) ONE ps_map_views_device call on the resident store with the request resident too, call -> synchronised."""

    def __init__(self, ctx, lib, scene, max_angle=0.5, K=K_TUM, image=IMAGE, require_visible=False):
        import torch
        from putslam_amd._abi import PS_VIEW_REQUIRE_VISIBLE, PsMapViewRequest
        from putslam_amd.device_batch import MapStoreDevice, MapViewsDevice
        self.ctx, self.lib, self.torch = ctx, lib, torch
        store, cam_inv, ang, cand, cc = scene
        self.store, self.V, self.cap = store, len(cam_inv), int(cand.shape[1])
        self.h = dict(cam=np.ascontiguousarray(cam_inv.transpose(0, 2, 1)).reshape(-1, 16), ang=np.ascontiguousarray(ang),
                      cand=np.ascontiguousarray(cand), cc=np.ascontiguousarray(cc))
        self.par = (float(max_angle),) + tuple(float(x) for x in K) + (float(image[0]), float(image[1]))
        self.vis = 1 if require_visible else 0
        V, cap = self.V, self.cap
        self.hb = dict(desc=np.zeros((V, cap, 32), np.uint8), pts=np.zeros((V, cap, 3), np.float32), nkpts=np.zeros(V, np.int32),
                       level=np.zeros((V, cap), np.int32))
        self.sd = MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                                 store["obs_det_dist"], store["num_poses"])
        dev = self.sd.device
        self.up = {k: torch.zeros(v.shape, dtype=getattr(torch, str(v.dtype)), device=dev) for k, v in self.hb.items()}
        self.d = {k: torch.from_numpy(v).to(dev) for k, v in self.h.items()}
        self.out = MapViewsDevice(V, cap, dev)
        rq = PsMapViewRequest()
        rq.camInv, rq.poseAngle, rq.cand, rq.candCounts = (self.d[k].data_ptr() for k in ("cam", "ang", "cand", "cc"))
        rq.maxAngle, rq.fx, rq.fy, rq.cx, rq.cy, rq.imageW, rq.imageH = self.par
        rq.V, rq.candCapacity, rq.flags = V, cap, PS_VIEW_REQUIRE_VISIBLE if require_visible else 0
        self.rq, self.st, self.os = rq, self.sd.view(), self.out.out_struct()
        torch.cuda.synchronize()

    def host(self):
        import ctypes as C
        import time
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        s, h, b = self.store, self.h, self.hb
        t = time.perf_counter()
        rc = self.lib.host_build_views(p(s["pos"]), p(s["obs_start"]), p(s["obs_pose"]), p(s["obs_desc"]), p(s["obs_octave"]),
                                       p(s["obs_det_dist"]), len(s["pos"]), p(h["cam"]), p(h["ang"]), s["num_poses"], p(h["cand"]),
                                       p(h["cc"]), self.cap, self.V, *self.par, self.vis, self.cap, p(b["desc"]), p(b["pts"]),
                                       p(b["nkpts"]), p(b["level"]))
        t1 = time.perf_counter()
        for k, v in b.items():
            self.up[k].copy_(self.torch.from_numpy(v))
        self.torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rc == 0
        return t2 - t, t1 - t

    def device(self):
        import time
        t = time.perf_counter()
        self.ctx.map_views_device(self.st, self.rq, self.os)
        self.ctx.synchronize()
        return time.perf_counter() - t

    def medians(self, regions=5):
        """Medians over alternating regions: (host loop + upload, host loop alone, one device call), seconds."""
        self.host()
        self.device()
        a, a0, b = [], [], []
        for _ in range(regions):
            x, y = self.host()
            a.append(x)
            a0.append(y)
            b.append(self.device())
        return float(np.median(a)), float(np.median(a0)), float(np.median(b))

    def check(self):
        """The two sides built the same views (the host loop has the store's own octaves: no table, the same levels)."""
        g = self.out.download()
        up = {k: v.cpu().numpy() for k, v in self.up.items()}
        assert np.array_equal(g["nkpts"], up["nkpts"]) and np.array_equal(g["viewCount"], up["nkpts"])
        for v in range(self.V):
            n = int(up["nkpts"][v])
            assert g["desc"][v, :n].tobytes() == up["desc"][v, :n].tobytes() and g["pts"][v, :n].tobytes() == up["pts"][v, :n].tobytes()
            assert g["mapLevel"][v, :n].tobytes() == up["level"][v, :n].tobytes()
        return int(up["nkpts"].mean())
