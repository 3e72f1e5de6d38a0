"""CPU answer and scenes for the batched map matching (ps_match_xyz_device / ps_map_pairs_device).

The answer is composed from what the oracle already exports -- oracle.match_xyz, then oracle.ransac_rigid3d with seed + p --
plus the batch's own rules: the per-pair capacity, and the selection of the retry ladder (PUTSLAM.cpp:788-798).
Scenes follow tests/test_gpu_parity.py::test_match_xyz_parity: map features near observed keypoints.
"""
import ctypes as C
import time

import numpy as np

from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, STATS_DTYPE, TUM_FR1_K, make_config


def ladder_try(radius, ratio, k):
    """(radius, ratio) of try k = 1, 2, ... (matcher.cpp:617-622)."""
    if k > 1:
        return radius + 0.02 * (k - 1), max(0.1, ratio - 0.05 * (k - 1))
    return radius, ratio


def ladder_pick(ratios, min_ratio=0.1):
    """0-based try the loop of PUTSLAM.cpp:788-798 ends on; NaN (no matches) is the reference's -1.0."""
    for k, r in enumerate(ratios):
        if (-1.0 if r != r else r) >= min_ratio:
            return k
    return len(ratios) - 1


def make_frames(rng, oracle, nkpts, cap):
    """Frames: positions in front of the camera, random descriptors, predicted levels."""
    F = len(nkpts)
    pos = np.zeros((F, cap, 3), np.float32)
    desc = np.zeros((F, cap, 32), np.uint8)
    level = np.zeros((F, cap), np.int32)
    for f, n in enumerate(nkpts):
        p = (rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 2.5]).astype(np.float32)
        pos[f, :n] = p
        desc[f, :n] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        octv = rng.integers(0, 8, n)
        level[f, :n] = [oracle.predicted_level(o, np.linalg.norm(q) * rng.uniform(0.8, 1.25), np.linalg.norm(q))
                        for o, q in zip(octv, p)]
    return dict(pos=pos, desc=desc, level=level, nkpts=np.asarray(nkpts, np.int32), cap=cap)


def make_views(rng, frames, nkpts, cap, source, sigma=0.05, shift=0.0):
    """Map views: view v's features sit near keypoints of frame source[v] (noise sigma, optional displacement along x),
    5 % of the descriptor bits flipped, levels off by -2 ... 2."""
    V = len(nkpts)
    pos = np.zeros((V, cap, 3), np.float32)
    desc = np.zeros((V, cap, 32), np.uint8)
    level = np.zeros((V, cap), np.int32)
    for v, n in enumerate(nkpts):
        f = source[v]
        nf = int(frames["nkpts"][f])
        if n == 0:
            continue
        if nf == 0:
            pos[v, :n] = (rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 2.5]).astype(np.float32)
            desc[v, :n] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            level[v, :n] = rng.integers(0, 8, n)
            continue
        src = rng.integers(0, nf, n)
        pos[v, :n] = (frames["pos"][f, src] + rng.normal(0, sigma, (n, 3)) + [shift, 0, 0]).astype(np.float32)
        desc[v, :n] = frames["desc"][f, src] ^ np.packbits(rng.random((n, 256)) < 0.05, axis=1)
        level[v, :n] = np.clip(frames["level"][f, src] + rng.integers(-2, 3, n), 0, 7)
    return dict(pos=pos, desc=desc, level=level, nkpts=np.asarray(nkpts, np.int32), cap=cap)


def canon_stats(st):
    """Stats as bytes, with every NaN pointInlierRatio as one bit pattern (the contract says NaN; 0 / 0 has either sign)."""
    st = np.array(st, STATS_DTYPE).reshape(-1).copy()
    st["pointInlierRatio"][np.isnan(st["pointInlierRatio"])] = np.nan
    return st.tobytes()


class Ref:
    """Oracle answers for pairs of one (views, frames) scene, cached: match lists per (view, frame, radius, ratio)."""

    def __init__(self, oracle, views, frames):
        self.o, self.views, self.frames = oracle, views, frames
        self._m = {}

    def side(self, s, i):
        n = int(s["nkpts"][i])
        return s["pos"][i, :n], s["desc"][i, :n], s["level"][i, :n]

    def matches(self, v, f, radius, ratio):
        key = (int(v), int(f), float(radius), float(ratio))
        if key not in self._m:
            mp, md, ml = self.side(self.views, v)
            cp, cd, cl = self.side(self.frames, f)
            if len(mp) == 0 or len(cp) == 0:
                self._m[key] = np.zeros(0, DMATCH_DTYPE)
            else:
                self._m[key] = self.o.match_xyz(mp, md, ml, cp, cd, cl, float(radius), float(ratio))
        return self._m[key]

    def pair(self, params, estimator, H, seed, K, v, f, radius, ratio, max_matches):
        """One pair: dict(numMatches, matches, mask, pose (16, column-major), stats)."""
        m = self.matches(v, f, radius, ratio)
        count = len(m)
        if count > max_matches:         # the capacity rule: -(count), and the estimator sees no matches
            m, n = np.zeros(0, DMATCH_DTYPE), -count
        else:
            n = count
        cfg, _ = make_config(estimator, H, seed=seed)
        r = self.o.ransac_rigid3d(params, cfg, K, self.side(self.views, v)[0], self.side(self.frames, f)[0], m)
        return dict(numMatches=n, matches=m, mask=r["mask"][:len(m)], pose=np.ascontiguousarray(r["pose"].T).reshape(16),
                    stats=r["stats"])

    def batch(self, params, estimator, H, seed, K, pairs, radius, ratio, max_matches):
        out = []
        for p, (v, f) in enumerate(pairs):
            r = radius[p] if np.ndim(radius) else radius
            a = ratio[p] if np.ndim(ratio) else ratio
            out.append(self.pair(params, estimator, H, seed + p, K, v, f, r, a, max_matches))
        return out


def compare(got, ref, lo=0, what=""):
    """got: download() of a MapBatchDevice (or a slice of it from pair lo on); ref: list of Ref.pair answers.  Bytes."""
    for i, r in enumerate(ref):
        p = lo + i
        tag = (what, p)
        assert int(got["numMatches"][p]) == r["numMatches"], (tag, int(got["numMatches"][p]), r["numMatches"])
        n = max(r["numMatches"], 0)
        assert got["matches"][p, :n].tobytes() == r["matches"].tobytes(), tag
        assert got["inlierMask"][p, :n].tobytes() == r["mask"].tobytes(), tag
        assert got["pose"][p].tobytes() == r["pose"].astype(np.float32).tobytes(), (tag, got["pose"][p], r["pose"])
        assert canon_stats(got["stats"][p]) == canon_stats(r["stats"]), (tag, got["stats"][p], r["stats"])


def sphere_edge_points(bound, want):
    """A float32 point q with  q0*q0 + (q1*q1 + q2*q2) == want  in float32 arithmetic (the kernel's order), near sqrt(bound)
    along x: found by a search over the last places of x and a small y.  None if the search fails."""
    want = np.float32(want)
    x0 = np.float32(np.sqrt(np.float64(bound)))
    xs = [x0]
    for _ in range(40):
        xs.append(np.nextafter(xs[-1], np.float32(0)))
    x = x0
    for _ in range(40):
        x = np.nextafter(x, np.float32(np.inf))
        xs.append(x)
    for x in xs:
        for ye in range(0, 400):
            y = np.float32(ye) * np.float32(1e-5) * x0
            s = np.float32(x * x) + np.float32(np.float32(y * y) + np.float32(0.0))
            if np.float32(s) == want:
                return np.array([x, y, 0.0], np.float32)
    return None


# ---------------------------------------------------------------- timing: the host loop the batch replaces, and the batch
TIMING_VIEWS = 8


def timing_scene(ctx, n, seed):
    """TIMING_VIEWS views on as many frames of n keypoints (levels from ctx.predicted_level)."""
    rng = np.random.default_rng(seed)
    frames = make_frames(rng, ctx, [n] * TIMING_VIEWS, n)
    views = make_views(rng, frames, [n] * TIMING_VIEWS, n, source=list(range(TIMING_VIEWS)), sigma=0.05)
    return views, frames


class HostLoop:
    """What a host had before the batch: per pair ps_match_xyz, then ps_ransac_rigid3d on the downloaded matches -- host
    pointers, preallocated buffers, straight through ctypes (no numpy conversions in the timed region)."""

    def __init__(self, ctx, views, frames, prm):
        self.ctx, self.v, self.f, self.prm = ctx, views, frames, prm
        n = views["cap"]
        self.m = np.zeros(16 * n, DMATCH_DTYPE)
        self.inl = np.zeros(16 * n, DMATCH_DTYPE)
        self.mask = np.zeros(16 * n, np.uint8)
        self.pose = np.zeros(16, np.float32)
        self.st = np.zeros(1, STATS_DTYPE)
        self.K = np.ascontiguousarray(TUM_FR1_K, np.float32)

    def pair(self, v, f, radius, ratio, seed):
        L, h, p = self.ctx._L, self.ctx._h, lambda a: a.ctypes.data_as(C.c_void_p)
        vw, fr = self.v, self.f
        nm, nc = int(vw["nkpts"][v]), int(fr["nkpts"][f])
        n = C.c_int(0)
        rc = L.ps_match_xyz(h, p(vw["pos"][v]), p(vw["desc"][v]), 32, p(vw["level"][v]), nm, p(fr["pos"][f]), p(fr["desc"][f]), 32,
                            p(fr["level"][f]), nc, radius, ratio, p(self.m), len(self.m), C.byref(n))
        assert rc == 0
        cfg, _ = make_config(EST_RANSAC, 487, seed=seed)
        ninl = C.c_int(0)
        rc = L.ps_ransac_rigid3d(h, C.byref(self.prm), C.byref(cfg), p(self.K), p(vw["pos"][v]), nm, p(fr["pos"][f]), nc, p(self.m),
                                 n.value, p(self.pose), p(self.inl), C.byref(ninl), p(self.mask), p(self.st))
        assert rc == 0
        return float(self.st[0]["pointInlierRatio"])

    def run(self, pairs, radius=0.12, ratio=0.55, seed=1):
        t = time.perf_counter()
        for i, (v, f) in enumerate(pairs):
            self.pair(int(v), int(f), radius, ratio, seed + i)
        return time.perf_counter() - t


def batch_time(ctx, prm, cfg, b):
    """One ps_map_pairs_device call on a MapBatchDevice, call -> synchronised, seconds."""
    from putslam_amd.device_batch import run_map_pairs
    t = time.perf_counter()
    run_map_pairs(ctx, prm, cfg, TUM_FR1_K, b, use_torch_stream=False)
    ctx.synchronize()
    return time.perf_counter() - t


def host_against_batch(ctx, prm, cfg, views, frames, vs, fs, P, max_matches, regions=5):
    """Medians of `regions` alternating regions: (seconds of the host loop, seconds of one device call, the batch)."""
    from putslam_amd.device_batch import MapBatchDevice
    pairs = np.array([(p % TIMING_VIEWS, p % TIMING_VIEWS) for p in range(P)], np.int32)
    b = MapBatchDevice(vs, views["level"], fs, frames["level"], pairs, max_matches)
    host = HostLoop(ctx, views, frames, prm)
    host.run(pairs[:4])
    batch_time(ctx, prm, cfg, b)
    ta, tb = [], []
    for _ in range(regions):
        ta.append(host.run(pairs))
        tb.append(batch_time(ctx, prm, cfg, b))
    return float(np.median(ta)), float(np.median(tb)), b
