"""Thin Python access to the C ABI (include/putslam_hip.h) for tests, the bench and Python callers.

Every function here ends in a HIP kernel launch inside libputslam_hip.so; nothing is computed
in Python/numpy and nothing falls back to the CPU.  The C++ drop-in classes that mirror the
reference's Matcher / RANSAC / TransformEst surface live in putslam_amd/csrc/dropin/.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (DMATCH_DTYPE, STATS_DTYPE, PS_ERR_BUSY, PS_MAX_KPTS, PS_OK, PS_SET_INVALID, PsExclusionRule, PsFrameSet,  # noqa: F401
                   PsFrameSetF32, PsHostPairResults, PsLoopBatch, PsLoopBatchF32, PsLoopResults, PsMapBatch, PsMapBatchF32, PsPairResults, PsMapStore,
                   PsMapStoreF32, PsMapViewOut, PsMapViewOutF32, PsMapViewRequest, PsPoseSetOut, PsPoseSetOutF32, PsPoseSetRequest, PsRansacConfig, PsRansacParams, default_ransac_params, make_config,
                   PsImageSet, PsKltParams, klt_params, PsDetectParams, detect_params, PsOrbParams, orb_params,
                   PsOrbDetectParams, orb_detect_params, PsDepthSet, PsFrameGeometry, PsFrameRowsOut, PsFrontEndParams, front_end_params,
                   PsPointSets, PsTrackedCarry, PsTrackedRows, PsTrackVoParams, PsTrackVoIn, PsTrackVoOut, track_vo_params,
                   PsTrackCandidates, PsTrackCloseParams, PsTrackCloseOut, track_close_params, PsSensorModel, PsUncertaintyOut,
                   PsMeasurementEdgesOut, sensor_model, PsPatchParams, PsPatchModel, patch_params)


class PsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"putslam_hip error {code}: {msg}")
        self.code = code


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _v(ptr):
    """A raw address as c_void_p; 0 / None: NULL."""
    return C.c_void_p(ptr or None)


def _host_image(a):
    """(image, channels) as the host forms of the image front end take one: (rows, cols) or (rows, cols, channels) uint8 whose rows
    may lie any stride apart (a region of a larger image) while a row itself is dense -- used where it lies; anything else is
    copied into a dense uint8 array."""
    a = np.asarray(a, np.uint8)
    assert a.ndim in (2, 3)
    cn = 1 if a.ndim == 2 else a.shape[2]
    dense = a.shape[1] * cn
    if not (a.strides[0] >= dense and (a.ndim == 2 and a.strides[1] == 1 or a.ndim == 3 and a.strides[1:] == (cn, 1))):
        a = np.ascontiguousarray(a)
    return a, cn


def retry_with_reported_capacity(run, cap, limit=None):
    """run(cap) -> (result, rows needed): the convention of the device batches, whose negative counts report the rows an
    overflowed output wanted.  If more were needed than `cap` (at most `limit`, if given), run is repeated ONCE with that
    many.  Returns (the last result, the capacity it ran with)."""
    result, need = run(cap)
    if limit is not None:
        need = min(need, limit)
    if need > cap:
        cap = need
        result, _ = run(cap)
    return result, cap


def dbscan_bound(eps):
    """ps_debug_dbscan_bound: the least double s* with (double)(float)sqrt(s*) >= eps (DBScan's predicate is s < s*)."""
    return float(_lib.load().ps_debug_dbscan_bound(float(eps)))


def map_sphere_bound(radius):
    """ps_map_sphere_bound: the least float B with  (float)|a - b| < radius  <=>  squared sum < B  (PsMapBatch.radiusBound)."""
    return float(_lib.load().ps_map_sphere_bound(float(radius)))


def sqrt_bound_f64(d):
    """ps_sqrt_bound_f64: the least double s with sqrt(s) >= d (sqrt(t) < d  <=>  t < s)."""
    return float(_lib.load().ps_sqrt_bound_f64(float(d)))


def _rule(rc, rule):
    if rc != PS_OK:
        raise PsError(rc, "exclusion rule constructor failed")
    return rule


def rule_new_map_features(min_euclid=0.03, min_image=2.0, max_add=200):
    """PsExclusionRule of PUTSLAM::chooseFeaturesToAddToMap (PUTSLAM.cpp:98-178); the thresholds are rounded to float as there."""
    r = PsExclusionRule()
    return _rule(_lib.load().ps_exclusion_rule_new_map_features(float(min_euclid), float(min_image), int(max_add), C.byref(r)), r)


def rule_merge_tracked(min_reproj):
    """PsExclusionRule of Matcher::mergeTrackedFeatures (matcher.cpp:97-130)."""
    r = PsExclusionRule()
    return _rule(_lib.load().ps_exclusion_rule_merge_tracked(float(min_reproj), C.byref(r)), r)


def rule_too_close(min_euclid, min_reproj):
    """PsExclusionRule of Matcher::removeTooCloseFeatures (matcher.cpp:886-974)."""
    r = PsExclusionRule()
    return _rule(_lib.load().ps_exclusion_rule_too_close(float(min_euclid), float(min_reproj), C.byref(r)), r)


def level_thresholds():
    """ps_level_thresholds: t[k], k = 0 .. 6, the least double x with ceil(log(x) / log(1.2)) > k under the host's libm; the
    predicted level of x is the number of t[k] it reaches (finite x).  Raises if the host's log is not clean around one of them."""
    t = (C.c_double * 7)()
    rc = _lib.load().ps_level_thresholds(t)
    if rc != PS_OK:
        raise PsError(rc, "ps_level_thresholds: the host's libm is not monotone around a switching point")
    return np.array(t[:], np.float64)


def view_angles(cur_pose, poses):
    """ps_view_angles: the angle table of FeaturesMap::findNearestFrame (featuresMap.cpp:534-556) for one current pose.
    cur_pose (4, 4), poses (N, 4, 4): matrices in the usual row / column indexing (stored column-major for the call)."""
    cur = np.ascontiguousarray(np.asarray(cur_pose, np.float64).reshape(4, 4).T)
    ps = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
    out = np.zeros(ps.shape[0], np.float64)
    rc = _lib.load().ps_view_angles(_p(cur), _p(ps), ps.shape[0], _p(out))
    if rc != PS_OK:
        raise PsError(rc, "ps_view_angles failed")
    return out


def ladder_try(radius, ratio, k):
    """(sphere radius, accept ratio) of try k = 1, 2, ... of Matcher::matchXYZ (matcher.cpp:617-622)."""
    if k > 1:
        return radius + 0.02 * (k - 1), max(0.1, ratio - 0.05 * (k - 1))
    return radius, ratio


def ladder_pick(ratios, min_ratio=0.1):
    """The try the loop of PUTSLAM.cpp:788-798 ends on (0-based): the first whose inlier ratio is not below min_ratio, else
    the last.  A NaN ratio (no matches) counts as the reference's -1.0 (matcher.cpp:755-756)."""
    for k, r in enumerate(ratios):
        if (-1.0 if r != r else r) >= min_ratio:
            return k
    return len(ratios) - 1


class Context:
    """One HIP stream + scratch arena (PsContext).  Not shared between threads."""

    def __init__(self, device=0, lib=None):
        self._L = _lib.load() if lib is None else _lib.load_path(lib)   # (lib: another build, A/B timing only)
        h = C.c_void_p()
        rc = self._L.ps_context_create(int(device), C.byref(h))
        if rc != PS_OK:
            raise PsError(rc, "ps_context_create failed (no usable HIP device? there is no CPU fallback)")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.ps_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != PS_OK:
            raise PsError(rc, self._L.ps_last_error(self._h).decode())

    @property
    def arch(self):
        return self._L.ps_device_arch(self._h).decode()

    def pack_records(self, pose_ptr, stats_ptr, valid, pairs, records_ptr, stream_ptr=0):
        """ps_pack_records_device: the 72-byte per-pair records of the multi-GPU gather (pose + numInliers + numMatchesIn as 18 floats),
        one launch on `stream_ptr` (0: the context's stream); rows [valid, pairs) are zero-filled.  Device pointers."""
        self._chk(self._L.ps_pack_records_device(self._h, C.c_void_p(stream_ptr), C.c_void_p(pose_ptr), C.c_void_p(stats_ptr),
                                                 int(valid), int(pairs), C.c_void_p(records_ptr)))

    def set_stream(self, stream_ptr):
        self._chk(self._L.ps_context_set_stream(self._h, C.c_void_p(stream_ptr)))

    @property
    def stream_ptr(self):
        """The hipStream_t the context's calls are queued on (ps_context_stream)."""
        return int(self._L.ps_context_stream(self._h) or 0)

    def synchronize(self):
        self._chk(self._L.ps_context_synchronize(self._h))

    def set_option(self, name, value):
        """Kernel variant switches (include/putslam_hip.h: ps_context_set_option), e.g. ("matcher", 0 | 1)."""
        self._chk(self._L.ps_context_set_option(self._h, name.encode(), int(value)))

    def score_stats(self):
        """(parked, evaluations) of the last fast scoring launch (needs set_option("score_stats", 1))."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.ps_debug_score_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def score_stats_ex(self):
        """All eight counters of the last scoring step (ps_debug_score_stats_ex): parked, evaluations made, reserved x 6."""
        out = (C.c_uint64 * 8)()
        self._chk(self._L.ps_debug_score_stats_ex(self._h, out))
        return [int(v) for v in out]

    def stage_survivors(self, P):
        """(2, P) hypotheses of every pair that survived stages 1 and 2 of the last staged scoring step."""
        out = np.zeros((2, int(P)), np.int32)
        self._chk(self._L.ps_debug_stage_survivors(self._h, int(P), out.ctypes.data))
        return out

    def stage_order(self, P, cap):
        """(perm (P, cap), front (P,)): the order stages 1+ of the last staged scoring step swept the matches in."""
        perm = np.zeros((int(P), int(cap)), np.int32)
        front = np.zeros(int(P), np.int32)
        self._chk(self._L.ps_debug_stage_order(self._h, int(P), int(cap), perm.ctypes.data, front.ctypes.data))
        return perm, front

    def stamps(self):
        """Shader-clock stamps of kernels 2 and 4 of the last call (needs set_option("stamps", 1)); ps_debug_stamps."""
        out = (C.c_uint64 * 16)()
        self._chk(self._L.ps_debug_stamps(self._h, out))
        return [int(v) for v in out]

    def get_option(self, name):
        v = self._L.ps_context_get_option(self._h, name.encode())
        if v < 0:
            raise ValueError(f"unknown option {name!r}")
        return v

    def enable_timing(self, on=True):
        self._chk(self._L.ps_context_enable_timing(self._h, 1 if on else 0))

    def last_kernel_times_ms(self):
        ms = np.zeros(8, np.float32)
        n = self._L.ps_last_kernel_times_ms(self._h, _p(ms))
        if n < 0:
            self._chk(n)
        names = kernel_names()
        return {names[i] if i < len(names) else f"k{i}": float(ms[i]) for i in range(n)}

    def kernel_time_totals(self):
        """{kernel name: (sum of launch durations in ms, launches)} over the calls since enable_timing()."""
        sums = np.zeros(8, np.float64)
        cnt = np.zeros(8, np.int32)
        n = self._L.ps_kernel_time_totals(self._h, _p(sums), _p(cnt))
        if n < 0:
            self._chk(n)
        names = kernel_names()
        return {names[i]: (float(sums[i]), int(cnt[i])) for i in range(n) if cnt[i] > 0}

    # ---- A1 ----
    def match_hamming256(self, query, train):
        """MatcherOpenCV::performMatching (matcherOpenCV.cpp:198-206): query=prev rows, train=cur rows (uint8, 32 cols)."""
        assert query.dtype == np.uint8 and train.dtype == np.uint8
        nq, nt = query.shape[0], train.shape[0]
        out = np.zeros(max(nq, 1), DMATCH_DTYPE)
        n = C.c_int(0)
        qs = query.strides[0] if nq else 32
        ts = train.strides[0] if nt else 32
        self._chk(self._L.ps_match_hamming256(self._h, _p(query), nq, qs, _p(train), nt, ts, _p(out), C.byref(n)))
        return out[: n.value].copy()

    def match_l2(self, query, train):
        """MatcherOpenCV::performMatching (matcherOpenCV.cpp:198-206) with the SURF / SIFT matcher, BFMatcher(NORM_L2, crossCheck)
        (matcherOpenCV.cpp:100-102): query = prev rows, train = cur rows (float32, the same number of columns, 1 .. 512)."""
        assert query.dtype == np.float32 and train.dtype == np.float32 and query.ndim == 2 and train.ndim == 2
        nq, nt, dim = query.shape[0], train.shape[0], query.shape[1]
        assert train.shape[1] == dim and (nq == 0 or query.strides[1] == 4) and (nt == 0 or train.strides[1] == 4)
        out = np.zeros(max(nq, 1), DMATCH_DTYPE)
        n = C.c_int(0)
        qs = query.strides[0] if nq else dim * 4
        ts = train.strides[0] if nt else dim * 4
        self._chk(self._L.ps_match_l2_f32(self._h, _p(query), nq, qs, _p(train), nt, ts, dim, _p(out), C.byref(n)))
        return out[: n.value].copy()

    def l2_stats(self):
        """(train rows swept exactly, candidate evaluations, rows whose candidate list overflowed) of the last float matching call
        that ran the prefilter with option "l2_stats" on."""
        out = (C.c_uint64 * 3)()
        self._chk(self._L.ps_debug_l2_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def debug_l2_band(self, query, train):
        """The prefilter's s~ and E for every (train row, query row) of one pair: two (nt, nq) float32 arrays (dim 64 / 128)."""
        query = np.ascontiguousarray(query, np.float32)
        train = np.ascontiguousarray(train, np.float32)
        nq, nt, dim = query.shape[0], train.shape[0], query.shape[1]
        s, e = np.zeros((nt, nq), np.float32), np.zeros((nt, nq), np.float32)
        self._chk(self._L.ps_debug_l2_band(self._h, _p(query), nq, dim * 4, _p(train), nt, dim * 4, dim, _p(s), _p(e)))
        return s, e

    # ---- A4..A9, A11 ----
    def ransac_rigid3d(self, params, cfg, K, prev, cur, matches):
        """RANSAC::estimateTransformation (RANSAC.cpp:50-174) / RANSAC_USAC (USAC_wrapper.cpp:104-151)."""
        prev = np.ascontiguousarray(prev, np.float32)
        cur = np.ascontiguousarray(cur, np.float32)
        matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        m = matches.shape[0]
        pose = np.zeros(16, np.float32)
        inl = np.zeros(max(m, 1), DMATCH_DTYPE)
        ninl = C.c_int(0)
        mask = np.zeros(max(m, 1), np.uint8)
        stats = np.zeros(1, STATS_DTYPE)
        self._chk(self._L.ps_ransac_rigid3d(self._h, C.byref(params), C.byref(cfg), _p(K), _p(prev), prev.shape[0],
                                            _p(cur), cur.shape[0], _p(matches), m, _p(pose), _p(inl), C.byref(ninl),
                                            _p(mask), _p(stats)))
        return dict(pose=pose.reshape(4, 4).T.copy(), inliers=inl[: ninl.value].copy(), mask=mask[:m].copy(),
                    stats=stats[0].copy())

    def debug_ransac_counts(self, params, cfg, K, prev, cur, matches):
        prev = np.ascontiguousarray(prev, np.float32)
        cur = np.ascontiguousarray(cur, np.float32)
        matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        counts = np.zeros(max(cfg.numHypotheses, 1), np.int32)
        n = C.c_int(0)
        self._chk(self._L.ps_debug_ransac_counts(self._h, C.byref(params), C.byref(cfg), _p(K), _p(prev),
                                                 prev.shape[0], _p(cur), cur.shape[0], _p(matches),
                                                 matches.shape[0], _p(counts), C.byref(n)))
        return counts[: n.value].copy()

    def debug_keys_clean(self):
        """Words of the keys block that are not all-ones at rest (ps_debug_keys_clean): must be 0."""
        bad = C.c_uint64(0)
        self._chk(self._L.ps_debug_keys_clean(self._h, C.byref(bad)))
        return int(bad.value)

    def debug_limits(self, estimator, min_ratio, H, M):
        out = np.zeros(M, np.int32)
        self._chk(self._L.ps_debug_limits(self._h, int(estimator), float(min_ratio), int(H), int(M), _p(out)))
        return out

    def debug_fastdiv(self, seed=1, blocks=2048, per_thread=2048):
        bad, n = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.ps_debug_fastdiv(self._h, int(seed), int(blocks), int(per_thread), C.byref(bad), C.byref(n)))
        return bad.value, n.value

    def debug_mathcheck(self, mode, elements, seed=1):
        """(mismatches, tested): ps_debug_mathcheck -- the prologue's exact short sqrt / reciprocal / quotient forms vs the operators."""
        bad, n = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.ps_debug_mathcheck(self._h, int(mode), int(seed), int(elements), C.byref(bad), C.byref(n)))
        return bad.value, n.value

    # ---- A7 ----
    def umeyama_f32(self, src, dst):
        """src, dst: (nsets, k, 3) or (k, 3). Returns (T (nsets,4,4) row/col matrices, valid (nsets,))."""
        src = np.ascontiguousarray(src, np.float32)
        dst = np.ascontiguousarray(dst, np.float32)
        single = src.ndim == 2
        if single:
            src, dst = src[None], dst[None]
        nsets, k = src.shape[0], src.shape[1]
        T = np.zeros((nsets, 16), np.float32)
        valid = np.zeros(nsets, np.int32)
        self._chk(self._L.ps_umeyama_f32(self._h, _p(src), _p(dst), k, nsets, _p(T), _p(valid)))
        T = T.reshape(nsets, 4, 4).transpose(0, 2, 1).copy()
        return (T[0], bool(valid[0])) if single else (T, valid.astype(bool))

    # ---- A10 ----
    def kabsch_f64(self, A, B, ld=None):
        """KabschEst::computeTransformation (kabschEst.cpp:24-68). A, B (n,3). Returns 4x4 mapping A onto B.
        ld=None: the arrays are copied to dense column-major storage.  ld given: A and B already are views of column-major
        storage with that leading dimension -- (n,3) float64 with strides (8, 8*ld), e.g. buf.reshape(3, ld)[:, :n].T -- and
        are handed over as they lie."""
        if ld is None:
            A = np.asfortranarray(A, np.float64)
            B = np.asfortranarray(B, np.float64)
            n = A.shape[0]
            ld = max(n, 1)
        else:
            n, ld = A.shape[0], int(ld)
            for M in (A, B):
                if not (M.dtype == np.float64 and M.shape == (n, 3) and ld >= max(n, 1) and M.strides[1] == 8 * ld
                        and (n <= 1 or M.strides[0] == 8)):
                    raise ValueError("kabsch_f64: A, B must be (n,3) float64 views of column-major storage with leading dimension ld")
        T = np.zeros(16, np.float64)
        self._chk(self._L.ps_kabsch_f64(self._h, _p(A), _p(B), n, ld, _p(T)))
        return T.reshape(4, 4).T.copy()

    # ---- A3 ----
    def keypoints2Dto3D(self, xy, depth, K, scale):
        xy = np.ascontiguousarray(xy, np.float32)
        K = np.ascontiguousarray(K, np.float32)
        assert depth.dtype == np.uint16 and depth.ndim == 2
        out = np.zeros((xy.shape[0], 3), np.float32)
        self._chk(self._L.ps_keypoints2Dto3D(self._h, _p(xy), xy.shape[0], _p(depth), depth.shape[0], depth.shape[1],
                                             depth.strides[0], _p(K), float(scale), _p(out)))
        return out

    def remove_image_distortion(self, xy, K, dist5):
        """RGBD::removeImageDistortion (RGBD.cpp:254-314)."""
        xy = np.ascontiguousarray(xy, np.float32)
        K = np.ascontiguousarray(K, np.float32)
        d = np.ascontiguousarray(dist5, np.float64)
        out = np.zeros_like(xy)
        self._chk(self._L.ps_remove_image_distortion(self._h, _p(xy), xy.shape[0], _p(K), _p(d), _p(out)))
        return out

    def dbscan_thin(self, xy, octave=None, eps=10.0, min_pts=2, features_from_cluster=1):
        """DBScan(eps, minPts, featuresFromCluster).run (src/Matcher/dbscan.cpp; defaults: the reference constructor's):
        the indices, ascending int32, of the keypoints it leaves in the vector.  xy: n x 2 float32 (a view with any row
        stride, e.g. the pt fields of a structured keypoint array), octave: n int32 or None (no -5 rule)."""
        xy = np.asarray(xy, np.float32)
        assert xy.ndim == 2 and xy.shape[1] == 2
        if xy.strides[1] != 4 or xy.strides[0] < 8 or xy.strides[0] % 4:
            xy = np.ascontiguousarray(xy)
        n = xy.shape[0]
        if octave is not None:
            octave = np.asarray(octave, np.int32).reshape(n)
            if octave.strides[0] < 4 or octave.strides[0] % 4:
                octave = np.ascontiguousarray(octave)
        kept = np.zeros(max(n, 1), np.int32)
        nk = C.c_int(0)
        self._chk(self._L.ps_dbscan_thin(self._h, _p(xy), xy.strides[0] if n else 8, _p(octave),
                                         octave.strides[0] if octave is not None and n else 4, n, float(eps), int(min_pts),
                                         int(features_from_cluster), _p(kept), C.byref(nk)))
        return kept[:nk.value].copy()

    def dbscan_thin_device(self, xy_ptr, octave_ptr, counts_ptr, frames, capacity, kept_ptr, nkept_ptr, eps=10.0, min_pts=2,
                           features_from_cluster=1):
        """ps_dbscan_thin_device on device pointers (asynchronous on the context's stream): device_batch.dbscan_thin_device."""
        self._chk(self._L.ps_dbscan_thin_device(self._h, C.c_void_p(xy_ptr), C.c_void_p(octave_ptr or None),
                                                C.c_void_p(counts_ptr), int(frames), int(capacity), float(eps), int(min_pts),
                                                int(features_from_cluster), C.c_void_p(kept_ptr), C.c_void_p(nkept_ptr)))

    # ---- spatial-exclusion filters (ps_exclusion.h) ----
    def exclude(self, rule, cand3, cand2, exist3=None, exist2=None):
        """ps_exclude: the indices, ascending int32, of the candidates `rule` (PsExclusionRule) accepts.  cand3 (n, 3) / cand2
        (n, 2) float32, exist3 (m, 3) / exist2 (m, 2) float32 or None; an array the rule does not read may be None."""
        def arr(a, w):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            assert a.ndim == 2 and a.shape[1] == w
            return a
        cand3, cand2, exist3, exist2 = arr(cand3, 3), arr(cand2, 2), arr(exist3, 3), arr(exist2, 2)
        n = (cand2 if cand2 is not None else cand3).shape[0]
        m = 0 if exist3 is None and exist2 is None else (exist2 if exist2 is not None else exist3).shape[0]
        assert all(a is None or a.shape[0] == n for a in (cand3, cand2)) and all(a is None or a.shape[0] == m for a in (exist3, exist2))
        kept = np.zeros(max(n, 1), np.int32)
        nk = C.c_int(0)
        self._chk(self._L.ps_exclude(self._h, C.byref(rule), _p(cand3), _p(cand2), n, _p(exist3), _p(exist2), m, _p(kept),
                                     C.byref(nk)))
        return kept[:nk.value].copy()

    def choose_new_features(self, feature3D, undistorted2D, map3D, map2D, min_euclid=0.03, min_image=2.0, max_add=200):
        """PUTSLAM::chooseFeaturesToAddToMap (PUTSLAM.cpp:98-178) from addedCounter = 0: the indices of the features it adds.
        map3D / map2D: the float casts of the visible map features' position and (u, v)."""
        return self.exclude(rule_new_map_features(min_euclid, min_image, max_add), feature3D, undistorted2D, map3D, map2D)

    def merge_tracked_features(self, undistorted2D, sandbox_undistorted2D, min_reproj):
        """Matcher::mergeTrackedFeatures (matcher.cpp:97-130): the indices of the sandbox features that are appended."""
        return self.exclude(rule_merge_tracked(min_reproj), None, sandbox_undistorted2D, None, undistorted2D)

    def remove_too_close_features(self, features3D, undistorted2D, min_euclid, min_reproj):
        """Matcher::removeTooCloseFeatures (matcher.cpp:886-974): the indices of the features that stay."""
        return self.exclude(rule_too_close(min_euclid, min_reproj), features3D, undistorted2D)

    def exclude_device(self, rule, cand3_ptr, cand2_ptr, cand_counts_ptr, cand_capacity, exist3_ptr, exist2_ptr, exist_counts_ptr,
                       exist_capacity, frames, kept_ptr, nkept_ptr):
        """ps_exclude_device on device pointers (asynchronous on the context's stream): device_batch.exclude_device."""
        self._chk(self._L.ps_exclude_device(self._h, C.byref(rule), _v(cand3_ptr), _v(cand2_ptr), _v(cand_counts_ptr),
                                            int(cand_capacity), _v(exist3_ptr), _v(exist2_ptr), _v(exist_counts_ptr),
                                            int(exist_capacity), int(frames), _v(kept_ptr), _v(nkept_ptr)))

    # ---- pyramidal Lucas-Kanade tracking (ps_klt.h) ----
    def _klt_pair(self, prev_img, next_img, prev_pts, params, next_pts):
        """The shared opening of the two host forms: (params, the ten leading arguments of either call, n, and next_pts / status /
        err of max(n, 1) rows, next_pts holding the initial flow if one was given)."""
        params = params or klt_params()
        (prev_img, cn), (next_img, _) = _host_image(prev_img), _host_image(next_img)
        assert prev_img.shape == next_img.shape
        if next_img.strides[0] != prev_img.strides[0]:   # (the call takes one row stride for both)
            prev_img, next_img = np.ascontiguousarray(prev_img), np.ascontiguousarray(next_img)
        prev_pts = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        n = prev_pts.shape[0]
        m = max(n, 1)
        nxt = np.zeros((m, 2), np.float32)
        if next_pts is not None:
            nxt[:n] = np.asarray(next_pts, np.float32).reshape(n, 2)
        head = (self._h, _p(prev_img), _p(next_img), prev_img.shape[0], prev_img.shape[1], cn, prev_img.strides[0], _p(prev_pts), _p(nxt), n)
        return params, head, n, nxt, np.zeros(m, np.uint8), np.zeros(m, np.float32)

    def calc_optical_flow_pyr_lk(self, prev_img, next_img, prev_pts, params: PsKltParams = None, next_pts=None):
        """cv::calcOpticalFlowPyrLK (ps_calc_optical_flow_pyr_lk) on numpy arrays: images (rows, cols) or (rows, cols, 3) uint8,
        prev_pts (n, 2) float32, next_pts the initial flow under PS_KLT_USE_INITIAL_FLOW.  params: _abi.klt_params(...), default
        the shipped OpenCVParams.  Returns (nextPts (n, 2) float32, status (n,) uint8, err (n,) float32)."""
        params, head, n, nxt, status, err = self._klt_pair(prev_img, next_img, prev_pts, params, next_pts)
        self._chk(self._L.ps_calc_optical_flow_pyr_lk(*head, _p(status), _p(err), C.byref(params)))
        return nxt[:n], status[:n], err[:n]

    def perform_tracking(self, prev_img, next_img, prev_pts, tracking_error_threshold, min_reproj_distance,
                         params: PsKltParams = None, next_pts=None):
        """MatcherOpenCV::performTracking (ps_perform_tracking) on numpy arrays: track, gate by error, drop the worse of two
        features that end closer than min_reproj_distance, compact.  Returns a dict: matches (k,) DMATCH_DTYPE = (i, j, 0, 0),
        kept_pts (k, 2), kept_idx (k,) -- what the caller compacts keyPoints / detDists with --, and next_pts / status / err of
        all n points."""
        params, head, n, nxt, status, err = self._klt_pair(prev_img, next_img, prev_pts, params, next_pts)
        m = max(n, 1)
        matches, kept_pts, kept_idx = np.zeros(m, DMATCH_DTYPE), np.zeros((m, 2), np.float32), np.zeros(m, np.int32)
        nk = C.c_int(0)
        self._chk(self._L.ps_perform_tracking(*head, C.byref(params), float(tracking_error_threshold), float(min_reproj_distance),
                                              _p(status), _p(err), _p(matches), C.byref(nk), _p(kept_pts), _p(kept_idx)))
        k = nk.value
        return dict(matches=matches[:k].copy(), kept_pts=kept_pts[:k].copy(), kept_idx=kept_idx[:k].copy(), next_pts=nxt[:n],
                    status=status[:n], err=err[:n])

    def klt_pyramids_create(self, rows, cols, channels, win_size, max_levels, slots):
        """ps_klt_pyramids_create: the handle of a device-resident pyramid set (device_batch.KltPyramids owns one)."""
        h = C.c_void_p()
        self._chk(self._L.ps_klt_pyramids_create(self._h, int(rows), int(cols), int(channels), int(win_size), int(max_levels),
                                                 int(slots), C.byref(h)))
        return h

    def klt_pyramids_build_device(self, pyr, images: PsImageSet, first_slot=0):
        self._chk(self._L.ps_klt_pyramids_build_device(self._h, pyr, C.byref(images), int(first_slot)))

    def klt_track_device(self, pyr, params: PsKltParams, pairs_ptr, prev_pts_ptr, counts_ptr, P, capacity, next_pts_ptr, status_ptr,
                         err_ptr):
        """ps_klt_track_device on device pointers (asynchronous on the context's stream): device_batch.track_klt_pairs."""
        self._chk(self._L.ps_klt_track_device(self._h, pyr, C.byref(params), _v(pairs_ptr), _v(prev_pts_ptr), _v(counts_ptr), int(P),
                                              int(capacity), _v(next_pts_ptr), _v(status_ptr), _v(err_ptr)))

    def klt_select_device(self, next_pts_ptr, status_ptr, err_ptr, counts_ptr, P, capacity, tracking_error_threshold,
                          min_reproj_distance, matches_ptr, num_matches_ptr, kept_pts_ptr, kept_idx_ptr):
        """ps_klt_select_device on device pointers (asynchronous on the context's stream): device_batch.select_tracked."""
        self._chk(self._L.ps_klt_select_device(self._h, _v(next_pts_ptr), _v(status_ptr), _v(err_ptr), _v(counts_ptr), int(P),
                                               int(capacity), float(tracking_error_threshold), float(min_reproj_distance),
                                               _v(matches_ptr), _v(num_matches_ptr), _v(kept_pts_ptr), _v(kept_idx_ptr)))

    def debug_klt_level(self, pyr, slot, level, channels):
        """ps_debug_klt_level: (image (rows + 2W, cols + 2W, cn) uint8, derivative (.., cn, 2) int16, (rows, cols)) of one stored
        level, border included."""
        dims = np.zeros(4, np.int32)
        self._chk(self._L.ps_debug_klt_level(self._h, pyr, int(slot), int(level), _p(dims), None, None))
        cn = int(channels)
        img = np.zeros((dims[2], dims[3], cn), np.uint8)
        der = np.zeros((dims[2], dims[3], cn, 2), np.int16)
        self._chk(self._L.ps_debug_klt_level(self._h, pyr, int(slot), int(level), _p(dims), _p(img), _p(der)))
        return img, der, (int(dims[0]), int(dims[1]))

    # ---- FAST-9/16 key point detection (ps_fast.h) ----
    def detect_features(self, image, params: PsDetectParams = None):
        """MatcherOpenCV::detectFeatures for detector = "FAST" (ps_detect_features) on a numpy image (rows, cols) or (rows, cols, 3)
        uint8, whose rows may lie any stride apart (a region of a larger image).  params: _abi.detect_params(...), default the
        shipped ones.  Returns (xy (n, 2) float32, response (n,) float32) in the final order: response descending, ties in
        raster order inside an ROI and in the order of the ROI loop across ROIs."""
        params = params or detect_params()
        image, cn = _host_image(image)
        cap = max(0, min(int(params.maximalTrackedFeatures), PS_MAX_KPTS))
        xy, response = np.zeros((max(cap, 1), 2), np.float32), np.zeros(max(cap, 1), np.float32)
        n = C.c_int(0)
        self._chk(self._L.ps_detect_features(self._h, _p(image), image.shape[0], image.shape[1], cn, image.strides[0], C.byref(params),
                                             _p(xy), _p(response), cap, C.byref(n)))
        return xy[:n.value].copy(), response[:n.value].copy()

    def fast_detector_create(self, rows, cols, channels, max_frames):
        """ps_fast_detector_create: the handle of a device-resident detector (device_batch.FastDetector owns one)."""
        h = C.c_void_p()
        self._chk(self._L.ps_fast_detector_create(self._h, int(rows), int(cols), int(channels), int(max_frames), C.byref(h)))
        return h

    def detect_features_device(self, det, images: PsImageSet, params: PsDetectParams, capacity, xy_ptr, response_ptr, counts_ptr,
                               passes=7):
        """ps_detect_features_device on device pointers (asynchronous on the context's stream): device_batch.detect_features_batch.
        passes other than 7: ps_debug_fast_passes, only the passes of the mask (1 score, 2 select, 4 join), for timing."""
        self._chk(self._L.ps_debug_fast_passes(self._h, det, C.byref(images), C.byref(params), int(capacity), _v(xy_ptr),
                                               _v(response_ptr), _v(counts_ptr), int(passes)))

    def debug_fast_maps(self, det, frame, rows, cols):
        """ps_debug_fast_maps: (grey, score, corner) of one frame of the detector's last call, (rows, cols) uint8 each."""
        maps = [np.zeros((int(rows), int(cols)), np.uint8) for _ in range(3)]
        self._chk(self._L.ps_debug_fast_maps(self._h, det, int(frame), _p(maps[0]), _p(maps[1]), _p(maps[2])))
        return tuple(maps)

    # ---- ORB key point detection (ps_orb_detect.h) ----
    def detect_features_orb(self, image, params: PsOrbDetectParams = None):
        """MatcherOpenCV::detectFeatures for detector = "ORB" (ps_detect_features_orb) on a numpy image (rows, cols) or (rows, cols, 3)
        uint8, whose rows may lie any stride apart (a region of a larger image).  params: _abi.orb_detect_params(...), default the
        shipped ones.  Returns (xy (n, 2) float32, response (n,) float32 -- Harris --, angle (n,) float32 degrees, octave (n,) int32)
        in the final order: response descending, ties in the order (level, raster position) inside an ROI and in the order of the
        ROI loop across ROIs."""
        params = params or orb_detect_params()
        image, cn = _host_image(image)
        cap = max(0, min(int(params.maximalTrackedFeatures), PS_MAX_KPTS))
        m = max(cap, 1)
        xy, response, angle, octave = np.zeros((m, 2), np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32)
        n = C.c_int(0)
        self._chk(self._L.ps_detect_features_orb(self._h, _p(image), image.shape[0], image.shape[1], cn, image.strides[0], C.byref(params),
                                                 _p(xy), _p(response), _p(angle), _p(octave), cap, C.byref(n)))
        k = n.value
        return xy[:k].copy(), response[:k].copy(), angle[:k].copy(), octave[:k].copy()

    def orb_detector_create(self, rows, cols, channels, params: PsOrbDetectParams, max_frames):
        """ps_orb_detector_create: the handle of a device-resident detector (device_batch.OrbDetector owns one)."""
        h = C.c_void_p()
        self._chk(self._L.ps_orb_detector_create(self._h, int(rows), int(cols), int(channels), C.byref(params), int(max_frames), C.byref(h)))
        return h

    def orb_detector_level(self, det, level):
        """ps_orb_detector_level: ((rows, cols), scale float32) of one level of an ROI's pyramid."""
        dims, scale = np.zeros(2, np.int32), C.c_float(0)
        if self._L.ps_orb_detector_level(det, int(level), _p(dims), C.byref(scale)) != PS_OK:
            raise PsError(-1, "ps_orb_detector_level: no such level")
        return (int(dims[0]), int(dims[1])), np.float32(scale.value)

    def orb_detect_frames(self, det, images: PsImageSet, params: PsOrbDetectParams, capacity, xy_ptr, response_ptr, angle_ptr, octave_ptr,
                          counts_ptr, passes=63):
        """ps_orb_detect_frames on device pointers (asynchronous on the context's stream): device_batch.detect_features_orb_batch.
        passes other than 63: ps_debug_orb_detect_passes, only the passes of the mask, for timing."""
        args = (self._h, det, C.byref(images), C.byref(params), int(capacity), _v(xy_ptr), _v(response_ptr), _v(angle_ptr), _v(octave_ptr),
                _v(counts_ptr))
        if passes == 63:
            self._chk(self._L.ps_orb_detect_frames(*args))
        else:
            self._chk(self._L.ps_debug_orb_detect_passes(*args, int(passes)))

    def debug_orb_detect_level(self, det, slot, level):
        """ps_debug_orb_detect_level: dict(raw, score (rows_l, cols_l) uint8; yx (n,) uint32 = y << 16 | x, response, angle (n,)
        float32, kept (n,) uint8) of one level of one slot of the detector's last call: the survivors of the first cut in raster
        order, kept = 1 where the second cut keeps them."""
        (rows, cols), _ = self.orb_detector_level(det, level)
        raw, score = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
        n = C.c_int32(0)
        self._chk(self._L.ps_debug_orb_detect_level(self._h, det, int(slot), int(level), _p(raw), _p(score), C.byref(n), None, None, None, None, 0))
        m = max(n.value, 1)
        yx, resp, ang, kept = np.zeros(m, np.uint32), np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.uint8)
        self._chk(self._L.ps_debug_orb_detect_level(self._h, det, int(slot), int(level), None, None, C.byref(n), _p(yx), _p(resp), _p(ang),
                                                    _p(kept), m))
        k = n.value
        return dict(raw=raw, score=score, yx=yx[:k], response=resp[:k], angle=ang[:k], kept=kept[:k])

    # ---- ORB descriptor extraction (ps_orb.h) ----
    def describe_features(self, image, xy, angle=None, octave=None, params: PsOrbParams = None, pattern=None):
        """MatcherOpenCV::describeFeatures for descriptor = "ORB" (ps_describe_features) on a numpy image (rows, cols) or
        (rows, cols, 3) uint8 whose rows may lie any stride apart.  xy (n, 2) float32; angle (n,) degrees, default -1 (what the FAST
        detector leaves); octave (n,) int32, default 0.  params: _abi.orb_params(...), default cv::ORB::create()'s; pattern (256, 4)
        int8 in -15 .. 15, default the library's.  Returns (desc (k, 32) uint8, kept_idx (k,) int32): the described key points
        grouped by octave, input order inside an octave; kept_idx[j] is the input index of row j."""
        params = params or orb_params()
        image, cn = _host_image(image)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = xy.shape[0]
        angle = np.full(n, -1.0, np.float32) if angle is None else np.ascontiguousarray(angle, np.float32).reshape(n)
        octave = np.zeros(n, np.int32) if octave is None else np.ascontiguousarray(octave, np.int32).reshape(n)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(1024)
        desc, kept = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.int32)
        k = C.c_int(0)
        self._chk(self._L.ps_describe_features(self._h, _p(image), image.shape[0], image.shape[1], cn, image.strides[0], C.byref(params),
                                               None if pat is None else _p(pat), _p(xy), _p(angle), _p(octave), n, _p(desc), _p(kept),
                                               C.byref(k)))
        return desc[:k.value].copy(), kept[:k.value].copy()

    def orb_pyramids_create(self, rows, cols, channels, params: PsOrbParams, pattern, slots):
        """ps_orb_pyramids_create: the handle of a device-resident pyramid set (device_batch.OrbPyramids owns one)."""
        h = C.c_void_p()
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(1024)
        self._chk(self._L.ps_orb_pyramids_create(self._h, int(rows), int(cols), int(channels), C.byref(params),
                                                 None if pat is None else _p(pat), int(slots), C.byref(h)))
        return h

    def orb_pyramids_build_device(self, pyr, images: PsImageSet, first_slot=0):
        self._chk(self._L.ps_orb_pyramids_build_device(self._h, pyr, C.byref(images), int(first_slot)))

    def describe_features_device(self, pyr, slots_ptr, xy_ptr, angle_ptr, octave_ptr, counts_ptr, F, capacity, desc_ptr, kept_idx_ptr,
                                 num_kept_ptr, passes=31):
        """ps_describe_features_device on device pointers (asynchronous on the context's stream): device_batch.describe_features_batch.
        passes other than 31: ps_debug_orb_passes, only the placement (8) or the rows (16), for timing."""
        if passes == 31:
            self._chk(self._L.ps_describe_features_device(self._h, pyr, _v(slots_ptr), _v(xy_ptr), _v(angle_ptr), _v(octave_ptr),
                                                          _v(counts_ptr), int(F), int(capacity), _v(desc_ptr), _v(kept_idx_ptr),
                                                          _v(num_kept_ptr)))
        else:
            self._chk(self._L.ps_debug_orb_passes(self._h, pyr, None, 0, _v(slots_ptr), _v(xy_ptr), _v(angle_ptr), _v(octave_ptr),
                                                  _v(counts_ptr), int(F), int(capacity), _v(desc_ptr), _v(kept_idx_ptr), _v(num_kept_ptr),
                                                  int(passes) & 24))

    def debug_orb_passes_build(self, pyr, images: PsImageSet, first_slot, passes):
        """ps_debug_orb_passes with a build mask alone: 1 level 0, 2 the resizes, 4 the blurs (timing scripts)."""
        self._chk(self._L.ps_debug_orb_passes(self._h, pyr, C.byref(images), int(first_slot), None, None, None, None, None, 0, 0, None, None,
                                              None, int(passes) & 7))

    def orb_pyramids_level(self, pyr, level):
        """ps_orb_pyramids_level: ((rows, cols), scale float32) of one level."""
        dims, scale = np.zeros(2, np.int32), C.c_float(0)
        rc = self._L.ps_orb_pyramids_level(pyr, int(level), _p(dims), C.byref(scale))
        if rc != PS_OK:
            raise ValueError("ps_orb_pyramids_level: no such level")
        return (int(dims[0]), int(dims[1])), np.float32(scale.value)

    def debug_orb_level(self, pyr, slot, level):
        """ps_debug_orb_level: (raw, blurred) of one level of one slot, (rows_l, cols_l) uint8 each."""
        (r, c), _ = self.orb_pyramids_level(pyr, level)
        raw, blr = np.zeros((r, c), np.uint8), np.zeros((r, c), np.uint8)
        self._chk(self._L.ps_debug_orb_level(self._h, pyr, int(slot), int(level), _p(raw), _p(blr)))
        return raw, blr

    # ---- frame assembly and the front end (ps_frame_assembly.h) ----
    def gather_keypoints(self, idx_ptr, nidx_ptr, F, capacity, xy_in, response_in, angle_in, octave_in, xy_out, response_out, angle_out,
                         octave_out, counts_out):
        """ps_gather_keypoints on device pointers (asynchronous on the context's stream): device_batch.gather_keypoints."""
        self._chk(self._L.ps_gather_keypoints(self._h, _v(idx_ptr), _v(nidx_ptr), int(F), int(capacity), _v(xy_in), _v(response_in),
                                              _v(angle_in), _v(octave_in), _v(xy_out), _v(response_out), _v(angle_out), _v(octave_out),
                                              _v(counts_out)))

    def assemble_frames(self, geometry: PsFrameGeometry, depth: PsDepthSet, first_depth_frame, xy_ptr, kept_idx_ptr, num_kept_ptr, F,
                        capacity, out: PsFrameRowsOut):
        """ps_assemble_frames on device pointers (asynchronous on the context's stream): device_batch.assemble_frames."""
        self._chk(self._L.ps_assemble_frames(self._h, C.byref(geometry), C.byref(depth), int(first_depth_frame), _v(xy_ptr),
                                             _v(kept_idx_ptr), _v(num_kept_ptr), int(F), int(capacity), C.byref(out)))

    def front_end_create(self, rows, cols, channels, params: PsFrontEndParams, pattern, max_frames):
        """ps_front_end_create: the handle of a device-resident front end (device_batch.FrontEnd owns one)."""
        h = C.c_void_p()
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(1024)
        self._chk(self._L.ps_front_end_create(self._h, int(rows), int(cols), int(channels), C.byref(params),
                                              None if pat is None else _p(pat), int(max_frames), C.byref(h)))
        return h

    def front_end_frames(self, fe, images: PsImageSet, depth: PsDepthSet, geometry: PsFrameGeometry, capacity, desc_ptr,
                         out: PsFrameRowsOut):
        """ps_front_end_frames on device pointers (asynchronous on the context's stream): device_batch.front_end_frames_batch."""
        self._chk(self._L.ps_front_end_frames(self._h, fe, C.byref(images), C.byref(depth), C.byref(geometry), int(capacity),
                                              _v(desc_ptr), C.byref(out)))

    def front_end_frame(self, image, depth, geometry: PsFrameGeometry, params: PsFrontEndParams = None, pattern=None):
        """The whole per-frame front end of Matcher::detectInitFeatures / Matcher::match for detector and descriptor "ORB"
        (ps_front_end_frame) on a numpy image (rows, cols) or (rows, cols, 3) uint8 and its depth image (rows, cols) uint16, whose
        rows may lie any stride apart.  Returns a dict of the k described key points in the described order: desc (k, 32) uint8,
        pts (k, 3) float32, xy / xy_undist (k, 2) float32, angle / response (k,) float32, octave (k,) int32, src_idx (k,) int32 (the
        row among DBScan's survivors), det_dist (k,) float64."""
        params = params or front_end_params()
        image, cn = _host_image(image)
        depth = np.asarray(depth)
        assert depth.dtype == np.uint16 and depth.ndim == 2 and depth.shape == image.shape[:2]
        if depth.strides[1] != 2 or depth.strides[0] < depth.shape[1] * 2:
            depth = np.ascontiguousarray(depth)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(1024)
        cap = max(1, min(int(params.detect.maximalTrackedFeatures), PS_MAX_KPTS))
        a = dict(desc=np.zeros((cap, 32), np.uint8), pts=np.zeros((cap, 3), np.float32), xy=np.zeros((cap, 2), np.float32),
                 xy_undist=np.zeros((cap, 2), np.float32), angle=np.zeros(cap, np.float32), response=np.zeros(cap, np.float32),
                 octave=np.zeros(cap, np.int32), src_idx=np.zeros(cap, np.int32), det_dist=np.zeros(cap, np.float64))
        ptr = lambda k: a[k].ctypes.data   # noqa: E731
        out = PsFrameRowsOut(ptr("pts"), None, ptr("xy"), ptr("xy_undist"), ptr("angle"), ptr("response"), ptr("octave"), ptr("src_idx"),
                             ptr("det_dist"), None, None, None)
        n = C.c_int(0)
        self._chk(self._L.ps_front_end_frame(self._h, _p(image), _p(depth), image.shape[0], image.shape[1], cn, image.strides[0],
                                             depth.strides[0], C.byref(params), None if pat is None else _p(pat), C.byref(geometry),
                                             _p(a["desc"]), C.byref(out), cap, C.byref(n)))
        return {k: v[:n.value].copy() for k, v in a.items()}

    # ---- measurement uncertainty (ps_uncertainty.h) ----
    @staticmethod
    def _host_depth(depth):
        depth = np.asarray(depth)
        assert depth.dtype == np.uint16 and depth.ndim == 2
        if depth.strides[1] != 2 or depth.strides[0] < depth.shape[1] * 2:
            depth = np.ascontiguousarray(depth)
        return depth

    # ---- sub-pixel matching on patches (MatchingOnPatches)
    def compute_patch(self, img, pts, params=None):
        """MatchingOnPatches::computePatch (ps_compute_patch) for n points of one image: img (rows, cols) or (rows, cols, 3) uint8,
        pts (n, 2) float64.  params: _abi.patch_params(...), default the shipped PatchesParams.  Returns (patch (n, E) float64,
        status (n,) uint8: 5 where the taps leave the image -- that row is zero --, else 2 or 1)."""
        params = params or patch_params()
        img, cn = _host_image(img)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        n, E = pts.shape[0], params.patchSize ** 2
        patch, status = np.zeros((max(n, 1), E), np.float64), np.zeros(max(n, 1), np.uint8)
        self._chk(self._L.ps_compute_patch(self._h, _p(img), img.shape[0], img.shape[1], cn, img.strides[0], _p(pts), n, C.byref(params),
                                           _p(patch), _p(status)))
        return patch[:n], status[:n]

    def compute_patch_gradient(self, img, pts, params=None):
        """MatchingOnPatches::computeGradient (ps_compute_patch_gradient): returns (gx (n, E) float32, gy (n, E) float32, invHessian
        (n, 3, 3) float32, status (n,) uint8)."""
        params = params or patch_params()
        img, cn = _host_image(img)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        n, E, m = pts.shape[0], params.patchSize ** 2, max(pts.shape[0], 1)
        gx, gy, inv, status = np.zeros((m, E), np.float32), np.zeros((m, E), np.float32), np.zeros((m, 3, 3), np.float32), np.zeros(m, np.uint8)
        self._chk(self._L.ps_compute_patch_gradient(self._h, _p(img), img.shape[0], img.shape[1], cn, img.strides[0], _p(pts), n,
                                                    C.byref(params), _p(gx), _p(gy), _p(inv), _p(status)))
        return gx[:n], gy[:n], inv[:n], status[:n]

    def optimize_location(self, old_patch, new_img, new_pts, gx, gy, inv_hessian, params=None, old_img=None):
        """MatchingOnPatches::optimizeLocation (ps_optimize_location) on a given model, for n points: old_patch (n, E) float64, gx /
        gy (n, E) float32, inv_hessian (n, 3, 3) float32, new_pts (n, 2) float64 the starting guesses.  old_img is not read (the
        reference reads it nowhere either).  Returns (newPts (n, 2) float64, status (n,) uint8, iterations (n,) int32)."""
        params = params or patch_params()
        img, cn = _host_image(new_img)
        E = params.patchSize ** 2
        nxt = np.array(new_pts, np.float64).reshape(-1, 2)
        n, m = nxt.shape[0], max(nxt.shape[0], 1)
        old_patch = np.ascontiguousarray(old_patch, np.float64).reshape(n, E)
        gx, gy = np.ascontiguousarray(gx, np.float32).reshape(n, E), np.ascontiguousarray(gy, np.float32).reshape(n, E)
        inv = np.ascontiguousarray(inv_hessian, np.float32).reshape(n, 9)
        status, iters = np.zeros(m, np.uint8), np.zeros(m, np.int32)
        self._chk(self._L.ps_optimize_location(self._h, None, _p(old_patch), _p(img), img.shape[0], img.shape[1], cn, img.strides[0], _p(nxt),
                                               n, _p(gx), _p(gy), _p(inv), C.byref(params), _p(status), _p(iters)))
        return nxt, status[:n], iters[:n]

    def optimize_locations(self, old_img, new_img, old_pts, new_pts, params=None):
        """The three calls fused for n points of one image pair (ps_optimize_locations): old_pts / new_pts (n, 2) float64.  Returns
        (newPts (n, 2) float64, status (n,) uint8 -- _abi.PATCH_* --, iterations (n,) int32)."""
        params = params or patch_params()
        (old, cn), (new, _) = _host_image(old_img), _host_image(new_img)
        assert old.shape == new.shape
        if new.strides[0] != old.strides[0]:   # (the call takes one row stride for both)
            old, new = np.ascontiguousarray(old), np.ascontiguousarray(new)
        old_pts = np.ascontiguousarray(old_pts, np.float64).reshape(-1, 2)
        n, m = old_pts.shape[0], max(old_pts.shape[0], 1)
        nxt = np.array(new_pts, np.float64).reshape(n, 2)
        status, iters = np.zeros(m, np.uint8), np.zeros(m, np.int32)
        self._chk(self._L.ps_optimize_locations(self._h, _p(old), _p(new), old.shape[0], old.shape[1], cn, old.strides[0], _p(old_pts),
                                                _p(nxt), n, C.byref(params), _p(status), _p(iters)))
        return nxt, status[:n], iters[:n]

    def patch_models(self, images: PsImageSet, slots_ptr, pts_ptr, counts_ptr, P, capacity, params, model: PsPatchModel, status_ptr):
        """ps_patch_models on device pointers (asynchronous on the context's stream): device_batch.patch_models."""
        self._chk(self._L.ps_patch_models(self._h, C.byref(images), slots_ptr, pts_ptr, counts_ptr, int(P), int(capacity), C.byref(params),
                                          C.byref(model) if model is not None else None, status_ptr))

    def patch_align(self, images: PsImageSet, pairs_ptr, old_pts_ptr, new_pts_ptr, counts_ptr, P, capacity, params, model, status_ptr,
                    iterations_ptr):
        """ps_patch_align on device pointers (asynchronous on the context's stream): device_batch.align_patches."""
        self._chk(self._L.ps_patch_align(self._h, C.byref(images), pairs_ptr, old_pts_ptr, new_pts_ptr, counts_ptr, int(P), int(capacity),
                                         C.byref(params), C.byref(model) if model is not None else None, status_ptr, iterations_ptr))

    def compute_normals(self, xy, depth, geometry: PsFrameGeometry):
        """RGBD::computeNormal (RGBD.cpp:101-144) at n undistorted positions xy (n, 2) float32 of a depth image (rows, cols) uint16
        whose rows may lie any stride apart (ps_compute_normals): (n, 3) float64."""
        xy, depth = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), self._host_depth(depth)
        out = np.zeros((len(xy), 3), np.float64)
        self._chk(self._L.ps_compute_normals(self._h, C.byref(geometry), _p(depth), depth.shape[0], depth.shape[1], depth.strides[0], _p(xy),
                                             len(xy), _p(out)))
        return out

    def compute_rgb_gradients(self, xy, image, depth, geometry: PsFrameGeometry):
        """RGBD::computeRGBGradient (RGBD.cpp:147-187) at n positions of a 3-channel image (rows, cols, 3) uint8 and its depth image
        (ps_compute_rgb_gradients): (n, 3) float64."""
        xy, depth = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), self._host_depth(depth)
        image, cn = _host_image(image)
        assert image.shape[:2] == depth.shape
        out = np.zeros((len(xy), 3), np.float64)
        self._chk(self._L.ps_compute_rgb_gradients(self._h, C.byref(geometry), _p(image), cn, image.strides[0], _p(depth), depth.shape[0],
                                                   depth.shape[1], depth.strides[0], _p(xy), len(xy), _p(out)))
        return out

    def information_matrices(self, xy, pts, depth, geometry: PsFrameGeometry, sensor: PsSensorModel = None, model=0, image=None):
        """The 3 x 3 information matrix FeaturesMap::addFeatures / addMeasurements give every Edge3D (featuresMap.cpp:110-121,261-274)
        for n features at xy (n, 2) float32 with points pts (n, 3) float32 (ps_information_matrices): (n, 3, 3) float64.  model -1 the
        identity, 0 the image coordinates, 1 the normal, 2 the colour gradient (needs the 3-channel image); sensor: a PsSensorModel,
        default _abi.sensor_model()."""
        sensor = sensor or sensor_model()
        xy, depth = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), self._host_depth(depth)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        assert len(pts) == len(xy)
        img, cn = (None, 3) if image is None else _host_image(image)
        out = np.zeros((len(xy), 3, 3), np.float64)
        self._chk(self._L.ps_information_matrices(self._h, C.byref(geometry), C.byref(sensor), int(model), _p(img), cn,
                                                  0 if img is None else img.strides[0], _p(depth), depth.shape[0], depth.shape[1],
                                                  depth.strides[0], _p(xy), _p(pts), len(xy), _p(out)))
        return out

    def feature_uncertainty_device(self, geometry: PsFrameGeometry, sensor: PsSensorModel, model, images: PsImageSet, depth: PsDepthSet,
                                   image_frame_ptr, xy_ptr, pts_ptr, counts_ptr, F, capacity, out: PsUncertaintyOut):
        """ps_feature_uncertainty on device pointers (asynchronous on the context's stream): device_batch.feature_uncertainty."""
        self._chk(self._L.ps_feature_uncertainty(self._h, C.byref(geometry), None if sensor is None else C.byref(sensor), int(model),
                                                 None if images is None else C.byref(images), C.byref(depth), _v(image_frame_ptr),
                                                 _v(xy_ptr), _v(pts_ptr), _v(counts_ptr), int(F), int(capacity), C.byref(out)))

    def measurement_edges_device(self, geometry: PsFrameGeometry, sensor: PsSensorModel, model, images: PsImageSet, depth: PsDepthSet,
                                 image_frame_ptr, batch: "DeviceMapBatch", res: "DeviceResults", xy_undist_ptr, out: PsMeasurementEdgesOut):
        """ps_measurement_edges on device pointers (asynchronous on the context's stream): device_batch.measurement_edges."""
        mb, rs = batch.struct(), res.struct()
        self._chk(self._L.ps_measurement_edges(self._h, C.byref(geometry), None if sensor is None else C.byref(sensor), int(model),
                                               None if images is None else C.byref(images), C.byref(depth), _v(image_frame_ptr),
                                               C.byref(mb), C.byref(rs), _v(xy_undist_ptr), C.byref(out)))

    # ---- the tracking VO step ----
    def ransac_match_lists_device(self, params, cfg, K, prev: PsPointSets, cur: PsPointSets, pairs_ptr, matches_ptr, num_matches_ptr, P,
                                  cap, out: "DeviceResults"):
        """ps_ransac_match_lists on device pointers (asynchronous on the context's stream): device_batch.ransac_match_lists."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        res = out.struct()
        self._chk(self._L.ps_ransac_match_lists(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(prev), C.byref(cur), _v(pairs_ptr),
                                                _v(matches_ptr), _v(num_matches_ptr), int(P), int(cap), C.byref(res)))

    def assemble_tracked_device(self, geometry: PsFrameGeometry, depth: PsDepthSet, depth_frame_ptr, next_pts_ptr, kept_idx_ptr,
                                num_kept_ptr, P, capacity, carry: PsTrackedCarry, out: PsTrackedRows):
        """ps_assemble_tracked on device pointers (asynchronous on the context's stream): device_batch.assemble_tracked."""
        self._chk(self._L.ps_assemble_tracked(self._h, C.byref(geometry), C.byref(depth), _v(depth_frame_ptr), _v(next_pts_ptr),
                                              _v(kept_idx_ptr), _v(num_kept_ptr), int(P), int(capacity),
                                              None if carry is None else C.byref(carry), C.byref(out)))

    def track_vo_pairs_device(self, pyr, klt: PsKltParams, tp: PsTrackVoParams, params, cfg, geometry: PsFrameGeometry, depth: PsDepthSet,
                              vin: PsTrackVoIn, P, capacity, out: PsTrackVoOut):
        """ps_track_vo_pairs on device pointers (asynchronous on the context's stream): device_batch.track_vo_pairs."""
        self._chk(self._L.ps_track_vo_pairs(self._h, pyr, C.byref(klt), C.byref(tp), C.byref(params), C.byref(cfg), C.byref(geometry),
                                            C.byref(depth), C.byref(vin), int(P), int(capacity), C.byref(out)))

    def track_vo_pair(self, prev_img, next_img, depth, geometry: PsFrameGeometry, rows, params, cfg, tp: PsTrackVoParams = None,
                      klt: PsKltParams = None, next_pts=None):
        """The tracking VO step of Matcher::trackKLT (matcher.cpp:147-211) for one pair on numpy arrays (ps_track_vo_pair), uploads
        included, synchronous: images (rows, cols[, 3]) uint8, the current frame's depth (rows, cols) uint16, rows: a dict of the
        previous frame's rows -- xy (n, 2), pts (n, 3) and any of angle, response, octave, det_dist (n,).  Returns a dict: next_pts /
        status / err of all n points; matches (k,) DMATCH_DTYPE, kept_idx (k,), mask (k,); rows -- the frame's rows in the same
        form, the previous rows of the next call --; pose (4, 4), stats."""
        tp, klt = tp or track_vo_params(), klt or klt_params()
        prev_img, cn = _host_image(prev_img)
        next_img, cn2 = _host_image(next_img)
        assert prev_img.shape == next_img.shape and cn == cn2
        if next_img.strides[0] != prev_img.strides[0]:
            prev_img, next_img = np.ascontiguousarray(prev_img), np.ascontiguousarray(next_img)
        depth = np.asarray(depth)
        assert depth.dtype == np.uint16 and depth.shape == prev_img.shape[:2]
        if depth.strides[1] != 2 or depth.strides[0] < depth.shape[1] * 2:
            depth = np.ascontiguousarray(depth)
        xy = np.ascontiguousarray(rows["xy"], np.float32).reshape(-1, 2)
        n, m = xy.shape[0], max(xy.shape[0], 1)
        pts = np.ascontiguousarray(rows["pts"], np.float32).reshape(n, 3)
        types = dict(angle=np.float32, response=np.float32, octave=np.int32, det_dist=np.float64)
        carried = {k: np.ascontiguousarray(rows[k], t).reshape(n) for k, t in types.items() if k in rows}
        o = dict(next_pts=np.zeros((m, 2), np.float32), status=np.zeros(m, np.uint8), err=np.zeros(m, np.float32), matches=np.zeros(m, DMATCH_DTYPE),
                 kept_idx=np.zeros(m, np.int32), mask=np.zeros(m, np.uint8), pose=np.zeros(16, np.float32), stats=np.zeros(1, STATS_DTYPE),
                 xy=np.zeros((m, 2), np.float32), xy_undist=np.zeros((m, 2), np.float32), pts=np.zeros((m, 3), np.float32))
        o.update({k: np.zeros(m, t) for k, t in types.items() if k in carried})
        if next_pts is not None:
            o["next_pts"][:n] = np.asarray(next_pts, np.float32).reshape(n, 2)
        ptr = lambda d, k: d[k].ctypes.data if k in d else None   # noqa: E731
        vin = PsTrackVoIn(None, None, xy.ctypes.data, pts.ctypes.data, None,
                          PsTrackedCarry(ptr(carried, "angle"), ptr(carried, "response"), ptr(carried, "octave"), ptr(carried, "det_dist")))
        out = PsTrackVoOut(ptr(o, "next_pts"), ptr(o, "status"), ptr(o, "err"), ptr(o, "matches"), None, ptr(o, "kept_idx"),
                           PsTrackedRows(ptr(o, "xy"), ptr(o, "xy_undist"), ptr(o, "pts"), None, ptr(o, "angle"), ptr(o, "response"),
                                         ptr(o, "octave"), ptr(o, "det_dist")), ptr(o, "mask"), ptr(o, "pose"), ptr(o, "stats"))
        k = C.c_int(0)
        self._chk(self._L.ps_track_vo_pair(self._h, _p(prev_img), _p(next_img), _p(depth), prev_img.shape[0], prev_img.shape[1], cn,
                                           prev_img.strides[0], depth.strides[0], C.byref(klt), C.byref(tp), C.byref(params), C.byref(cfg),
                                           C.byref(geometry), C.byref(vin), n, C.byref(out), C.byref(k)))
        k = k.value
        new = {name: o[name][:k].copy() for name in ("xy", "xy_undist", "pts") + tuple(carried)}
        return dict(next_pts=o["next_pts"][:n], status=o["status"][:n], err=o["err"][:n], matches=o["matches"][:k].copy(),
                    kept_idx=o["kept_idx"][:k].copy(), mask=o["mask"][:k].copy(), rows=new, pose=o["pose"].reshape(4, 4).T.copy(),
                    stats=o["stats"][0].copy())

    # ---- closing the tracking VO step ----
    def track_candidates_device(self, fe, images: PsImageSet, depth: PsDepthSet, geometry: PsFrameGeometry, capacity, out: PsFrameRowsOut):
        """ps_track_candidates on device pointers (asynchronous on the context's stream): device_batch.track_candidates."""
        self._chk(self._L.ps_track_candidates(self._h, fe, C.byref(images), C.byref(depth), C.byref(geometry), int(capacity), C.byref(out)))

    def track_close_create(self, max_pairs, max_rows):
        """ps_track_close_create: the handle of the intermediates of ps_track_close_pairs (device_batch.TrackClose owns one)."""
        h = C.c_void_p()
        self._chk(self._L.ps_track_close_create(self._h, int(max_pairs), int(max_rows), C.byref(h)))
        return h

    def track_close_pairs_device(self, tc, pyr, slots_ptr, tp: PsTrackCloseParams, tracked: PsTrackedRows, cand: PsTrackCandidates,
                                 cand_frame_ptr, P, capacity, out_capacity, out: PsTrackCloseOut, passes=15):
        """ps_track_close_pairs on device pointers (asynchronous on the context's stream): device_batch.track_close_pairs.  passes
        other than 15: ps_debug_track_close_passes (timing scripts)."""
        args = (self._h, tc, pyr, _v(slots_ptr), C.byref(tp), C.byref(tracked), None if cand is None else C.byref(cand), _v(cand_frame_ptr),
                int(P), int(capacity), int(out_capacity), C.byref(out))
        self._chk(self._L.ps_track_close_pairs(*args) if passes == 15 else self._L.ps_debug_track_close_passes(*args, int(passes)))

    def track_close_pair(self, image, depth, geometry: PsFrameGeometry, rows, params: PsFrontEndParams = None, tp: PsTrackCloseParams = None,
                         pattern=None):
        """The second half of Matcher::trackKLT (matcher.cpp:213-381) for one frame on numpy arrays (ps_track_close_pair), uploads
        included, synchronous: image (rows, cols[, 3]) uint8 and its depth (rows, cols) uint16, rows: a dict of the tracked rows --
        xy, xy_undist (n, 2), pts (n, 3), angle, response, octave, det_dist (n,) -- as Context.track_vo_pair returns them (with
        xy_undist).  Returns a dict: desc (k, 32) uint8, rows -- the closed rows in the same form, the previous rows of the next
        frame --, src_idx (k,) int32 (a candidate's is max(n, 1) + i) and refill (0 not due, 1 merged)."""
        params, tp = params or front_end_params(), tp or track_close_params()
        image, cn = _host_image(image)
        depth = np.asarray(depth)
        assert depth.dtype == np.uint16 and depth.ndim == 2 and depth.shape == image.shape[:2]
        if depth.strides[1] != 2 or depth.strides[0] < depth.shape[1] * 2:
            depth = np.ascontiguousarray(depth)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(1024)
        types = (("xy", np.float32, (2,)), ("xy_undist", np.float32, (2,)), ("pts", np.float32, (3,)), ("angle", np.float32, ()),
                 ("response", np.float32, ()), ("octave", np.int32, ()), ("det_dist", np.float64, ()))
        n = len(np.asarray(rows["xy"]).reshape(-1, 2))
        t = {k: np.ascontiguousarray(rows[k], dt).reshape((n,) + tail) for k, dt, tail in types}

        def struct(d):
            return PsTrackedRows(d["xy"].ctypes.data, d["xy_undist"].ctypes.data, d["pts"].ctypes.data, None, d["angle"].ctypes.data,
                                 d["response"].ctypes.data, d["octave"].ctypes.data, d["det_dist"].ctypes.data)
        cap = max(n, 1) + max(1, min(int(params.detect.maximalTrackedFeatures), PS_MAX_KPTS))
        o = {k: np.zeros((cap,) + tail, dt) for k, dt, tail in types}
        desc, src = np.zeros((cap, 32), np.uint8), np.zeros(cap, np.int32)
        k, refill = C.c_int(0), C.c_int(0)
        self._chk(self._L.ps_track_close_pair(self._h, _p(image), _p(depth), image.shape[0], image.shape[1], cn, image.strides[0],
                                              depth.strides[0], C.byref(params), None if pat is None else _p(pat), C.byref(geometry),
                                              C.byref(tp), C.byref(struct(t)), n, _p(desc), C.byref(struct(o)), _p(src), cap, C.byref(k),
                                              C.byref(refill)))
        k = k.value
        return dict(desc=desc[:k].copy(), rows={name: a[:k].copy() for name, a in o.items()}, src_idx=src[:k].copy(), refill=refill.value)

    def ransac_match_lists(self, params, cfg, K, prev, cur, matches, pairs=None):
        """The estimator over P caller-supplied match lists (ps_ransac_match_lists) on numpy data, uploads and downloads included,
        synchronous: prev / cur lists of (n, 3) float32 point sets, matches a list of P DMATCH_DTYPE arrays, pairs (P, 2) (previous
        set, current set) or None for (p, p); pair p draws from cfg.seed + p.  Returns a dict: inlierMask (P, cap) uint8, pose
        (P, 16), stats (P,) STATS_DTYPE.  (The data goes through device_batch, which allocates with torch.)"""
        from . import device_batch as db
        dev = "cuda:%d" % self._L.ps_context_device(self._h)
        P = len(matches)
        if P == 0:      # (ps_ransac_match_lists: P == 0 is PS_OK and writes nothing)
            return dict(inlierMask=np.zeros((0, 1), np.uint8), pose=np.zeros((0, 16), np.float32), stats=np.zeros(0, STATS_DTYPE))
        sets_p, sets_c = db.PointSets.from_host(prev, dev), db.PointSets.from_host(cur, dev)
        cap = max([1] + [len(m) for m in matches])
        block = np.zeros((max(P, 1), cap), DMATCH_DTYPE)
        for p, m in enumerate(matches):
            block[p, :len(m)] = np.asarray(m, DMATCH_DTYPE)
        import torch
        d_matches = torch.from_numpy(block.view(np.int32).reshape(max(P, 1), cap, 4)).to(dev)
        d_num = torch.from_numpy(np.array([len(m) for m in matches] or [0], np.int32)).to(dev)
        d_pairs = None if pairs is None else torch.from_numpy(np.ascontiguousarray(pairs, np.int32).reshape(P, 2)).to(dev)
        out = db.ransac_match_lists(self, params, cfg, K, sets_p, sets_c, d_matches, d_num, d_pairs)
        res = out.download()
        return dict(inlierMask=res["inlierMask"], pose=res["pose"], stats=res["stats"])

    def points3Dto2D(self, xyz, K):
        xyz = np.ascontiguousarray(xyz, np.float32)
        K = np.ascontiguousarray(K, np.float32)
        uv = np.zeros((xyz.shape[0], 2), np.float32)
        self._chk(self._L.ps_points3Dto2D(self._h, _p(xyz), xyz.shape[0], _p(K), _p(uv)))
        return uv

    # ---- N2 ----
    def match_xyz(self, map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, radius=0.12, ratio=0.55):
        """Guided map matching core of Matcher::matchXYZ (matcher.cpp:694-746)."""
        return self._match_xyz(self._L.ps_match_xyz, np.uint8, 32, (), map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level,
                               radius, ratio)

    def match_xyz_l2(self, map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, radius=0.12, ratio=0.55):
        """match_xyz for float descriptors (ps_match_xyz_l2_f32): (n, dim) float32 rows, the value is the L2 norm of the float
        difference accumulated in double (tests/map_l2_ref.py)."""
        map_desc = np.ascontiguousarray(map_desc, np.float32)
        cur_desc = np.ascontiguousarray(cur_desc, np.float32)
        assert map_desc.ndim == 2 and cur_desc.ndim == 2 and map_desc.shape[1] == cur_desc.shape[1]
        dim = map_desc.shape[1]
        return self._match_xyz(self._L.ps_match_xyz_l2_f32, np.float32, dim * 4, (dim,), map_pos, map_desc, map_level, cur_pos,
                               cur_desc, cur_level, radius, ratio)

    def _match_xyz(self, entry, dtype, row_bytes, dim_arg, map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, radius, ratio):
        """match_xyz / match_xyz_l2: `entry` on rows of `dtype`, `row_bytes` apart (dim_arg: what the entry takes after ncur);
        repeated with the reported count while the output rows are too few."""
        map_pos = np.ascontiguousarray(map_pos, np.float32)
        cur_pos = np.ascontiguousarray(cur_pos, np.float32)
        map_desc = np.ascontiguousarray(map_desc, dtype)
        cur_desc = np.ascontiguousarray(cur_desc, dtype)
        map_level = np.ascontiguousarray(map_level, np.int32)
        cur_level = np.ascontiguousarray(cur_level, np.int32)
        nmap, ncur = map_pos.shape[0], cur_pos.shape[0]
        cap = max(1, 4 * nmap)
        while True:
            out = np.zeros(cap, DMATCH_DTYPE)
            n = C.c_int(0)
            rc = entry(self._h, _p(map_pos), _p(map_desc), row_bytes, _p(map_level), nmap, _p(cur_pos), _p(cur_desc), row_bytes,
                       _p(cur_level), ncur, *dim_arg, float(radius), float(ratio), _p(out), cap, C.byref(n))
            if rc == PS_OK:
                return out[: n.value].copy()
            if n.value > cap:
                cap = n.value
                continue
            self._chk(rc)

    def predicted_level(self, octave, det_dist, cur_dist):
        return self._L.ps_predicted_level(int(octave), float(det_dist), float(cur_dist))

    # ---- map views from a resident feature map ----
    def map_views_device(self, store: PsMapStore, request: PsMapViewRequest, out: PsMapViewOut):
        """ps_map_views_device on filled structs of device pointers (asynchronous): device_batch.build_map_views."""
        self._chk(self._L.ps_map_views_device(self._h, C.byref(store), C.byref(request), C.byref(out)))

    def frame_levels_device(self, frames: "DeviceFrames", octave_ptr, det_dist_ptr, cur_level_ptr):
        """ps_frame_levels_device: predicted levels of the keypoints of a device-resident frame set (asynchronous)."""
        fs = frames.struct()
        self._chk(self._L.ps_frame_levels_device(self._h, C.byref(fs), _v(octave_ptr), _v(det_dist_ptr), _v(cur_level_ptr)))

    # ---- loop-closure candidates from a resident feature map ----
    def pose_sets_device(self, store: PsMapStore, request: PsPoseSetRequest, out: PsPoseSetOut):
        """ps_pose_sets_device on filled structs of device pointers (asynchronous): device_batch.build_pose_sets."""
        self._chk(self._L.ps_pose_sets_device(self._h, C.byref(store), C.byref(request), C.byref(out)))

    def map_views_l2_device(self, store: PsMapStoreF32, request: PsMapViewRequest, out: PsMapViewOutF32):
        """ps_map_views_l2_device on filled structs of device pointers (asynchronous): device_batch.build_map_views_l2."""
        self._chk(self._L.ps_map_views_l2_device(self._h, C.byref(store), C.byref(request), C.byref(out)))

    def pose_sets_l2_device(self, store: PsMapStoreF32, request: PsPoseSetRequest, out: PsPoseSetOutF32):
        """ps_pose_sets_l2_device on filled structs of device pointers (asynchronous): device_batch.build_pose_sets_l2."""
        self._chk(self._L.ps_pose_sets_l2_device(self._h, C.byref(store), C.byref(request), C.byref(out)))

    def loop_pairs_l2_device(self, params, cfg, K, batch: PsLoopBatchF32, out: PsLoopResults):
        """ps_loop_pairs_l2_device on filled structs of device pointers (asynchronous): device_batch.run_loop_pairs_l2."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        self._chk(self._L.ps_loop_pairs_l2_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(batch), C.byref(out)))

    def loop_pairs_device(self, params, cfg, K, batch: PsLoopBatch, out: PsLoopResults):
        """ps_loop_pairs_device on filled structs of device pointers (asynchronous): device_batch.run_loop_pairs."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        self._chk(self._L.ps_loop_pairs_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(batch), C.byref(out)))

    def verify_loop_closures(self, store, obs_point3d, candidates, params, cfg, K, min_features=35, ratio_threshold=0.4,
                             max_kpts=None):
        """The loop of FeaturesMap::loopClosure (featuresMap.cpp:751-806) over a whole queue of candidates as two calls on the
        resident store (a device_batch.MapStoreDevice; obs_point3d (O, 3) float64 beside it): candidates (L, 2) POSE ids
        ([0] = frameIds[0], the query side); the poses are made unique, ps_pose_sets_device builds one set per pose and
        ps_loop_pairs_device verifies every candidate, candidate l drawing from cfg.seed + l; params.errorVersion is used as
        given (the caller sets errorVersionMap).  max_kpts (default 1024) is the sets' first capacity: if a set overflows it
        the two calls are repeated once with the largest reported count (PS_MAX_KPTS at most), the ladder's rule.
        Returns dict(poses (S,) the unique pose ids, pairs (L, 2) set indices, set_count (S,), ratio (L,) -- matchingRatio as
        the reference logs it: 0.0 gated, -1.0 no matches --, closed (L,) bool, num_paired (L,), paired_rows / paired_feat:
        lists of (n, 2) arrays (rows of the two sets / feature indices), pose (L, 4, 4), stats, num_matches)."""
        from . import device_batch as db
        return self._verify_loop_closures(db.build_pose_sets, db.LoopBatchDevice, db.run_loop_pairs, store, obs_point3d, candidates,
                                          params, cfg, K, min_features, ratio_threshold, max_kpts)

    def verify_loop_closures_l2(self, store, obs_point3d, candidates, params, cfg, K, min_features=35, ratio_threshold=0.4,
                                max_kpts=None):
        """verify_loop_closures for a store of float descriptor rows (a device_batch.MapStoreF32Device): ps_pose_sets_l2_device
        and ps_loop_pairs_l2_device; the same contract, the same result dict, the same single retry at the reported capacity."""
        from . import device_batch as db
        return self._verify_loop_closures(db.build_pose_sets_l2, db.LoopBatchF32Device, db.run_loop_pairs_l2, store, obs_point3d,
                                          candidates, params, cfg, K, min_features, ratio_threshold, max_kpts)

    def _verify_loop_closures(self, build_sets, batch_type, run_pairs, store, obs_point3d, candidates, params, cfg, K, min_features,
                              ratio_threshold, max_kpts):
        from . import device_batch
        cand = np.ascontiguousarray(candidates, np.int32).reshape(-1, 2)
        poses, inv = np.unique(cand.reshape(-1), return_inverse=True)
        poses, pairs = poses.astype(np.int32), inv.reshape(-1, 2).astype(np.int32)
        # (uploaded once, whatever the number of attempts)
        obs_point3d = device_batch.to_device_tensor(obs_point3d, device_batch.torch.float64, store.device, (-1, 3))

        def run(cap):
            sets = build_sets(self, store, obs_point3d, poses, cap)
            batch = batch_type(sets, pairs, min_features, ratio_threshold)
            run_pairs(self, params, cfg, K, batch)
            r = batch.download()
            count = sets.set_count.cpu().numpy()[:len(poses)]
            over = count[(count < 0) & (count != PS_SET_INVALID)]     # a set overflowed its rows: -(count)
            return (r, count), int(-over.min()) if len(over) else 0

        (r, count), cap = retry_with_reported_capacity(run, int(max_kpts) if max_kpts is not None else 1024, PS_MAX_KPTS)
        n = [max(int(x), 0) for x in r["numPaired"]]
        return dict(poses=poses, pairs=pairs, set_count=count, ratio=r["ratio"].copy(), closed=r["closed"].astype(bool),
                    num_paired=r["numPaired"].copy(), paired_rows=[r["pairedRows"][l, :n[l]].copy() for l in range(len(n))],
                    paired_feat=[r["pairedFeat"][l, :n[l]].copy() for l in range(len(n))],
                    pose=r["pose"].reshape(-1, 4, 4).transpose(0, 2, 1).copy(), stats=r["stats"].copy(),
                    num_matches=r["numMatches"].copy(), max_kpts=cap)

    # ---- A2 / A12: device-resident batch ----
    def vo_pairs_device(self, params, cfg, K, frames: "DeviceFrames", pairs_dev_ptr, P, out: "DeviceResults"):
        K = np.ascontiguousarray(K, np.float32)
        fs, res = frames.struct(), out.struct()
        self._chk(self._L.ps_vo_pairs_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(fs),
                                             C.c_void_p(pairs_dev_ptr), int(P), C.byref(res)))

    def match_l2_device(self, frames: "DeviceFramesF32", pairs_dev_ptr, P, matches_ptr, num_matches_ptr):
        """ps_match_l2_device: the float-descriptor cross-check matching of every pair; asynchronous, device pointers."""
        fs = frames.struct()
        self._chk(self._L.ps_match_l2_device(self._h, C.byref(fs), C.c_void_p(pairs_dev_ptr), int(P), C.c_void_p(matches_ptr),
                                             C.c_void_p(num_matches_ptr)))

    def vo_pairs_l2_device(self, params, cfg, K, frames: "DeviceFramesF32", pairs_dev_ptr, P, out: "DeviceResults"):
        """ps_vo_pairs_l2_device: ps_vo_pairs_device with the float-descriptor matcher in front."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        fs, res = frames.struct(), out.struct()
        self._chk(self._L.ps_vo_pairs_l2_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(fs),
                                                C.c_void_p(pairs_dev_ptr), int(P), C.byref(res)))

    # ---- N2, device-resident batch ----
    def match_xyz_device(self, batch: "DeviceMapBatch", matches_ptr, num_matches_ptr):
        """ps_match_xyz_device: the guided matching of every pair of the batch; asynchronous, device pointers."""
        mb = batch.struct()
        self._chk(self._L.ps_match_xyz_device(self._h, C.byref(mb), C.c_void_p(matches_ptr), C.c_void_p(num_matches_ptr)))

    def map_pairs_device(self, params, cfg, K, batch: "DeviceMapBatch", out: "DeviceResults"):
        """ps_map_pairs_device: guided matching + the estimator for every pair; asynchronous, device pointers."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        mb, res = batch.struct(), out.struct()
        self._chk(self._L.ps_map_pairs_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(mb), C.byref(res)))

    def match_xyz_l2_device(self, batch: "DeviceMapBatchF32", matches_ptr, num_matches_ptr):
        """ps_match_xyz_l2_device: match_xyz_device for float descriptors; asynchronous, device pointers."""
        mb = batch.struct()
        self._chk(self._L.ps_match_xyz_l2_device(self._h, C.byref(mb), C.c_void_p(matches_ptr), C.c_void_p(num_matches_ptr)))

    def map_pairs_l2_device(self, params, cfg, K, batch: "DeviceMapBatchF32", out: "DeviceResults"):
        """ps_map_pairs_l2_device: map_pairs_device for float descriptors; asynchronous, device pointers."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        mb, res = batch.struct(), out.struct()
        self._chk(self._L.ps_map_pairs_l2_device(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(mb), C.byref(res)))

    def match_xyz_ladder_l2(self, map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, params, cfg, K, radius=0.12,
                            ratio=0.55, max_tries=10, min_ratio=0.1, max_matches=None, device=None):
        """match_xyz_ladder for float descriptors ((n, dim) float32 rows): the tries of matcher.cpp:617-622 as ONE
        ps_map_pairs_l2_device call; the same selection, the same result dict, the same capacity rule."""
        from . import device_batch as db
        map_desc = np.ascontiguousarray(map_desc, np.float32)
        cur_desc = np.ascontiguousarray(cur_desc, np.float32)
        assert map_desc.ndim == 2 and cur_desc.ndim == 2 and map_desc.shape[1] == cur_desc.shape[1]
        return self._match_xyz_ladder(db.FrameSetF32Device, db.MapBatchF32Device, db.run_map_pairs_l2, np.float32, map_desc.shape[1],
                                      map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, params, cfg, K, radius, ratio,
                                      max_tries, min_ratio, max_matches, device)

    def match_xyz_ladder(self, map_pos, map_desc, map_level, cur_pos, cur_desc, cur_level, params, cfg, K, radius=0.12,
                         ratio=0.55, max_tries=10, min_ratio=0.1, max_matches=None, device=None):
        """The retry loop of PUTSLAM.cpp:788-798 around Matcher::matchXYZ as ONE ps_map_pairs_device call of `max_tries` pairs
        that all name the same map view and frame: try k = 1 .. max_tries has radius + 0.02 (k - 1) and
        max(0.1, ratio - 0.05 (k - 1)) (matcher.cpp:617-622) and draws from cfg.seed + k - 1.  Returns the first try whose
        pointInlierRatio (-1.0 for "no matches") is not below min_ratio, else the last: dict(matches, mask, pose (4 x 4), stats,
        inlier_ratio, try_used (1-based), num_matches).  max_matches (default 4 x map features) is the rows' first capacity: if
        any try overflows it the call is repeated once with the largest reported count, so no try is ever passed over.
        The call does max_tries times the work of a first try that succeeds -- it is meant for hosts that care about the
        worst frame, whose ten sequential tries are ten round trips; a host that cares about the average frame calls
        match_xyz + ransac_rigid3d and retries.  Measured (profiles/r08a/map_pairs.txt): 0.55 ms at 500 x 500 and 0.85 ms at
        2000 x 2000 against 0.23 / 0.68 / 2.3 ms and 0.30 / 0.89 / 3.2 ms for one / three / ten sequential tries -- the ladder
        wins from the third try on."""
        from . import device_batch as db
        return self._match_xyz_ladder(db.FrameSetDevice, db.MapBatchDevice, db.run_map_pairs, np.uint8, 32, map_pos, map_desc,
                                      map_level, cur_pos, cur_desc, cur_level, params, cfg, K, radius, ratio, max_tries, min_ratio,
                                      max_matches, device)

    def _match_xyz_ladder(self, frame_set_type, batch_type, run_pairs, dtype, width, map_pos, map_desc, map_level, cur_pos, cur_desc,
                          cur_level, params, cfg, K, radius, ratio, max_tries, min_ratio, max_matches, device):
        map_pos = np.ascontiguousarray(map_pos, np.float32)
        cur_pos = np.ascontiguousarray(cur_pos, np.float32)
        nmap, ncur = map_pos.shape[0], cur_pos.shape[0]
        dev = device if device is not None else "cuda:%d" % self._L.ps_context_device(self._h)

        def side(desc, pos, level, n):       # one view / frame as a frame set of its own (capacity >= 1)
            cap = max(n, 1)
            d, q, lv = np.zeros((1, cap, width), dtype), np.zeros((1, cap, 3), np.float32), np.zeros((1, cap), np.int32)
            if n:
                d[0], q[0], lv[0] = np.asarray(desc, dtype).reshape(n, width), pos, np.asarray(level, np.int32).reshape(n)
            return frame_set_type(d, q, [n], dev), lv

        views, mlv = side(map_desc, map_pos, map_level, nmap)
        frames, clv = side(cur_desc, cur_pos, cur_level, ncur)
        tries = [ladder_try(float(radius), float(ratio), k) for k in range(1, int(max_tries) + 1)]

        def run(cap):
            batch = batch_type(views, mlv, frames, clv, np.zeros((len(tries), 2), np.int32), cap,
                               radius=[t[0] for t in tries], ratio=[t[1] for t in tries])
            run_pairs(self, params, cfg, K, batch)
            r = batch.download()
            # (a try that overflowed its rows reports -(count): the repeat has room for the largest, as the loop would see it)
            return r, int(-r["numMatches"].min()) if len(tries) else 0

        r, _ = retry_with_reported_capacity(run, int(max_matches) if max_matches is not None else max(1, 4 * nmap))
        ratios = [float(x) for x in r["stats"]["pointInlierRatio"]]
        k = ladder_pick(ratios, min_ratio)
        n = max(int(r["numMatches"][k]), 0)
        ir = ratios[k]
        return dict(matches=r["matches"][k, :n].copy(), mask=r["inlierMask"][k, :n].copy(), pose=r["pose"][k].reshape(4, 4).T.copy(),
                    stats=r["stats"][k].copy(), inlier_ratio=-1.0 if ir != ir else ir, try_used=k + 1,
                    num_matches=int(r["numMatches"][k]))


class _ChainContext(Context):
    """A chain context of a BatchQueue: owned by the queue (never destroyed from here)."""

    def __init__(self, L, handle):
        self._L = L
        self._h = C.c_void_p(handle)

    def close(self):
        self._h = None


class BatchQueue:
    """PsBatchQueue: ps_vo_pairs_device through launch chains that are never joined (chains = 0: the library's default, four;
    whole batches in turn: consecutive batches run side by side and need output blocks of their own, `chains` of them in turn)."""

    def __init__(self, ctx: Context, chains=0):
        self._ctx = ctx
        h = C.c_void_p()
        ctx._chk(ctx._L.ps_batch_queue_create(ctx._h, int(chains), C.byref(h)))
        self._h = h
        self.chains = ctx._L.ps_batch_queue_chains(h)
        self.contexts = [_ChainContext(ctx._L, ctx._L.ps_batch_queue_context(h, i)) for i in range(self.chains)]

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):
                self._ctx._L.ps_batch_queue_destroy(self._h)
            self._h = None
            for c in self.contexts:
                c.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, params, cfg, K, frames: "DeviceFrames", pairs_dev_ptr, P, out: "DeviceResults"):
        """Asynchronous; returns the batch's ticket."""
        K = np.ascontiguousarray(K, np.float32)
        fs, res = frames.struct(), out.struct()
        t = C.c_int64(-1)
        self._ctx._chk(self._ctx._L.ps_batch_queue_submit(self._h, C.byref(params), C.byref(cfg), _p(K), C.byref(fs),
                                                          C.c_void_p(pairs_dev_ptr), int(P), C.byref(res), C.byref(t)))
        return int(t.value)

    def wait(self, ticket):
        self._ctx._chk(self._ctx._L.ps_batch_queue_wait(self._h, int(ticket)))

    def query(self, ticket):
        r = self._ctx._L.ps_batch_queue_query(self._h, int(ticket))
        if r < 0:
            self._ctx._chk(r)
        return bool(r)

    def wait_on_stream(self, ticket, stream_ptr):
        self._ctx._chk(self._ctx._L.ps_batch_queue_wait_on_stream(self._h, int(ticket), C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ctx._chk(self._ctx._L.ps_batch_queue_synchronize(self._h))

    def last_split(self):
        b = np.zeros(self.chains + 1, np.int32)
        self._ctx._L.ps_batch_queue_last_split(self._h, b.ctypes.data)
        return [int(x) for x in b]


class VoStream:
    """Streaming Matcher::match (matcher.cpp:452-516): previous frame resident in HBM (ps_vo_stream_*)."""

    def __init__(self, ctx: Context, max_kpts):
        self._ctx = ctx
        self._cap = int(max_kpts)
        h = C.c_void_p()
        ctx._chk(ctx._L.ps_vo_stream_create(ctx._h, self._cap, C.byref(h)))
        self._h = h
        # push()'s output block, allocated once with its pointers (four arrays and five pointer objects per call were a
        # quarter of a pushed frame's 0.097 ms; the C call itself takes 0.07 - 0.08, demos/cpp/demo_latency)
        self._matches = np.zeros(max(self._cap, 1), DMATCH_DTYPE)
        self._mask = np.zeros(max(self._cap, 1), np.uint8)
        self._pose = np.zeros(16, np.float32)
        self._stats = np.zeros(1, STATS_DTYPE)
        self._nm = C.c_int(0)
        self._out_ptrs = (_p(self._matches), C.byref(self._nm), _p(self._mask), _p(self._pose), _p(self._stats))

    def close(self):
        if getattr(self, "_h", None):
            # (a stream outliving its context -- a test that failed before closing it, collected after the context fixture -- is
            # leaked, not destroyed through a dangling context)
            if getattr(self._ctx, "_h", None):
                self._ctx._L.ps_vo_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, params, cfg, K, desc, pts):
        """Returns None for the first frame, else dict(matches, mask, pose, stats)."""
        desc = np.ascontiguousarray(desc, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        K = np.ascontiguousarray(K, np.float32)
        pm, pn, pk, pp, ps = self._out_ptrs
        rc = self._ctx._L.ps_vo_stream_push(self._h, C.byref(params), C.byref(cfg), C.c_void_p(K.ctypes.data), C.c_void_p(desc.ctypes.data),
                                            32, C.c_void_p(pts.ctypes.data), desc.shape[0], pm, pn, pk, pp, ps)
        if rc:
            self._ctx._chk(rc)
        nm = self._nm.value
        if nm < 0:
            return None
        return dict(matches=self._matches[:nm].copy(), mask=self._mask[:nm].copy(),
                    pose=self._pose.reshape(4, 4).T.copy(), stats=self._stats[0].copy())

    # ---- pipelined form (ps_vo_stream_configure_async ...): results come back with a lag, in pair order ----
    def configure_async(self, params, cfg, K, chunk_frames=0, lanes=0, results=0, packed=False):
        """results: 0 = everything (PS_RESULTS_FULL), 1 = inlier matches + pose + stats, 2 = pose + stats.
        packed: PS_FRAMES_PACKED -- every frame one block [cap x 32 B][cap x 12 B] of `packed_stride` bytes, on the host and in
        the ring: one upload per chunk (push_many_packed)."""
        K = None if K is None else np.ascontiguousarray(K, np.float32)
        self._ctx._chk(self._ctx._L.ps_vo_stream_set_result_mode(self._h, int(results)))
        self._ctx._chk(self._ctx._L.ps_vo_stream_set_frame_layout(self._h, 1 if packed else 0))
        self._ctx._chk(self._ctx._L.ps_vo_stream_configure_async(self._h, C.byref(params), C.byref(cfg), _p(K),
                                                                 int(chunk_frames), int(lanes)))

    def _rc(self, rc):
        """PS_ERR_BUSY is flow control, not a failure: returns False for it, True for PS_OK, raises otherwise."""
        if rc == PS_ERR_BUSY:
            return False
        self._ctx._chk(rc)
        return True

    def push_async(self, desc, pts):
        """One frame (matcher.cpp:452-516's call shape); False = no room (every lane busy and the upload-ahead queue full), pop first."""
        desc = np.ascontiguousarray(desc, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        return self._rc(self._ctx._L.ps_vo_stream_push_async(self._h, _p(desc), 32, _p(pts), desc.shape[0]))

    def push_many(self, desc, pts, nkpts):
        """desc (F, cap, 32) u8, pts (F, cap, 3) f32, nkpts (F,) i32 -- numpy arrays (pinned ones are read in place: keep them
        untouched until their results have been popped) or raw (address, address, array) for pre-sliced pinned blocks."""
        nk = np.ascontiguousarray(nkpts, np.int32)
        if isinstance(desc, int):
            dp, pp = C.c_void_p(desc), C.c_void_p(pts)
        else:
            assert desc.flags.c_contiguous and pts.flags.c_contiguous and desc.dtype == np.uint8 and pts.dtype == np.float32
            assert desc.shape[1:] == (self._cap, 32) and pts.shape[1:] == (self._cap, 3)
            dp, pp = _p(desc), _p(pts)
        return self._rc(self._ctx._L.ps_vo_stream_push_many(self._h, dp, pp, _p(nk), nk.shape[0]))

    @property
    def packed_stride(self):
        """Bytes per frame of the packed layout (cap x 44 rounded up to a multiple of 16)."""
        return int(self._ctx._L.ps_vo_stream_packed_stride(self._h))

    def push_many_packed(self, frames, nkpts):
        """frames: (F, packed_stride) u8, every row [cap x 32 B descriptors][cap x 12 B points][padding] -- a numpy array
        (pinned: read in place) or a raw address; nkpts (F,) i32."""
        nk = np.ascontiguousarray(nkpts, np.int32)
        if isinstance(frames, int):
            fp = C.c_void_p(frames)
        else:
            assert frames.flags.c_contiguous and frames.dtype == np.uint8 and frames.shape[1:] == (self.packed_stride,)
            fp = _p(frames)
        return self._rc(self._ctx._L.ps_vo_stream_push_many_packed(self._h, fp, self.packed_stride, _p(nk), nk.shape[0]))

    def flush(self):
        return self._rc(self._ctx._L.ps_vo_stream_flush(self._h))

    def reset(self):
        return self._rc(self._ctx._L.ps_vo_stream_reset(self._h))

    def pending(self):
        return self._ctx._L.ps_vo_stream_pending(self._h)

    def graph_launches(self):
        """Pushes / small chunks replayed from a captured hipGraph so far."""
        return int(self._ctx._L.ps_vo_stream_graph_launches(self._h))

    def pop_many(self, wait=True, copy=True):
        """Results of the oldest chunk in flight: None if nothing is ready, else dict(first_pair, epoch, matches (n, cap),
        numMatches, inlierMask, pose (n, 16), stats).  copy=False: views of the pinned block, valid until the next pop."""
        v = PsHostPairResults()
        self._ctx._chk(self._ctx._L.ps_vo_stream_pop_many(self._h, 1 if wait else 0, C.byref(v)))
        if v.count == 0:
            return None
        n, cap = v.count, v.maxKpts

        def arr(ptr, nbytes, dtype, shape):
            a = np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype).reshape(shape)
            return a.copy() if copy else a

        return dict(first_pair=int(v.firstPair), epoch=int(v.epoch), count=n, result_mode=int(v.resultMode),
                    matches=arr(v.matches, n * cap * 16, DMATCH_DTYPE, (n, cap)) if v.matches else None,
                    numMatches=arr(v.numMatches, n * 4, np.int32, (n,)),
                    inlierMask=arr(v.inlierMask, n * cap, np.uint8, (n, cap)) if v.inlierMask else None,
                    pose=arr(v.pose, n * 64, np.float32, (n, 16)),
                    stats=arr(v.stats, n * STATS_DTYPE.itemsize, STATS_DTYPE, (n,)))

    def pop(self, wait=True):
        """One pair, copied out: None if nothing is ready / in flight, else the dict `push` returns."""
        matches = np.zeros(max(self._cap, 1), DMATCH_DTYPE)
        mask = np.zeros(max(self._cap, 1), np.uint8)
        pose = np.zeros(16, np.float32)
        stats = np.zeros(1, STATS_DTYPE)
        nm = C.c_int(0)
        self._ctx._chk(self._ctx._L.ps_vo_stream_pop(self._h, 1 if wait else 0, _p(matches), C.byref(nm), _p(mask), _p(pose),
                                                     _p(stats)))
        if nm.value < 0:
            return None
        return dict(matches=matches[: nm.value].copy(), mask=mask[: nm.value].copy(),
                    pose=pose.reshape(4, 4).T.copy(), stats=stats[0].copy())


class PinnedBuffer:
    """Page-locked host memory from ps_host_alloc, as a numpy array (frames handed to VoStream.push_many in place)."""

    def __init__(self, shape, dtype):
        self._L = _lib.load()
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.ptr = self._L.ps_host_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise MemoryError("ps_host_alloc failed")
        self.array = np.frombuffer((C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr), dtype=self.dtype,
                                   count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._L.ps_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceFrames:
    """Raw device pointers of a frame set (PsFrameSet)."""

    def __init__(self, desc_ptr, pts_ptr, nkpts_ptr, num_frames, max_kpts, desc_stride=0, pts_stride=0):
        self.desc_ptr, self.pts_ptr, self.nkpts_ptr = desc_ptr, pts_ptr, nkpts_ptr
        self.num_frames, self.max_kpts = int(num_frames), int(max_kpts)
        self.desc_stride, self.pts_stride = int(desc_stride), int(pts_stride)      # bytes between frames; 0 = dense

    def struct(self):
        return PsFrameSet(self.desc_ptr, self.pts_ptr, self.nkpts_ptr, self.num_frames, self.max_kpts, self.desc_stride,
                          self.pts_stride)


class DeviceFramesF32:
    """Raw device pointers of a frame set with float descriptors (PsFrameSetF32); strides in bytes, 0 = dense."""

    def __init__(self, desc_ptr, pts_ptr, nkpts_ptr, num_frames, max_kpts, dim, row_stride=0, desc_stride=0, pts_stride=0):
        self.desc_ptr, self.pts_ptr, self.nkpts_ptr = desc_ptr, pts_ptr, nkpts_ptr
        self.num_frames, self.max_kpts, self.dim = int(num_frames), int(max_kpts), int(dim)
        self.row_stride, self.desc_stride, self.pts_stride = int(row_stride), int(desc_stride), int(pts_stride)

    def struct(self):
        return PsFrameSetF32(self.desc_ptr, self.pts_ptr, self.nkpts_ptr, self.num_frames, self.max_kpts, self.dim,
                             self.row_stride, self.desc_stride, self.pts_stride)


class DeviceResults:
    """Raw device pointers of per-pair outputs (PsPairResults)."""

    def __init__(self, matches_ptr, num_matches_ptr, mask_ptr, pose_ptr, stats_ptr):
        self.matches_ptr, self.num_matches_ptr, self.mask_ptr = matches_ptr, num_matches_ptr, mask_ptr
        self.pose_ptr, self.stats_ptr = pose_ptr, stats_ptr

    def struct(self):
        return PsPairResults(self.matches_ptr, self.num_matches_ptr, self.mask_ptr, self.pose_ptr, self.stats_ptr)


class DeviceMapBatch:
    """Raw device pointers of a map-matching batch (PsMapBatch): maps / frames are DeviceFrames."""

    def __init__(self, maps: DeviceFrames, map_level_ptr, frames: DeviceFrames, cur_level_ptr, pairs_ptr, P, max_matches,
                 radius_bound=0.0, accept_ratio=0.0, radius_bound_per_pair_ptr=None, accept_ratio_per_pair_ptr=None):
        self.maps, self.frames = maps, frames
        self.map_level_ptr, self.cur_level_ptr, self.pairs_ptr = map_level_ptr, cur_level_ptr, pairs_ptr
        self.P, self.max_matches = int(P), int(max_matches)
        self.radius_bound, self.accept_ratio = float(radius_bound), float(accept_ratio)
        self.radius_bound_per_pair_ptr, self.accept_ratio_per_pair_ptr = radius_bound_per_pair_ptr, accept_ratio_per_pair_ptr

    def struct(self):
        return PsMapBatch(self.maps.struct(), self.map_level_ptr, self.frames.struct(), self.cur_level_ptr, self.pairs_ptr,
                          self.P, self.max_matches, self.radius_bound, self.accept_ratio, self.radius_bound_per_pair_ptr,
                          self.accept_ratio_per_pair_ptr)


class DeviceMapBatchF32(DeviceMapBatch):
    """Raw device pointers of a float-descriptor map-matching batch (PsMapBatchF32): maps / frames are DeviceFramesF32."""

    def struct(self):
        return PsMapBatchF32(self.maps.struct(), self.map_level_ptr, self.frames.struct(), self.cur_level_ptr, self.pairs_ptr,
                             self.P, self.max_matches, self.radius_bound, self.accept_ratio, self.radius_bound_per_pair_ptr,
                             self.accept_ratio_per_pair_ptr)


def kernel_names():
    L = _lib.load()
    raw = L.ps_kernel_names()
    names, cur, i = [], b"", 0
    while True:
        ch = raw[i]
        i += 1
        if ch == b"\x00":
            if not cur:
                break
            names.append(cur.decode())
            cur = b""
        else:
            cur += ch
    return names


def algorithmic_bytes(nkpts, matches_in, matches_valid, H):
    return int(_lib.load().ps_algorithmic_bytes(int(nkpts), int(matches_in), int(matches_valid), int(H)))


def gradient_tie_table(k=1):
    """ps_debug_gradient_tie_table: the 5 x 4 table of the colour gradient's ties at magnitude k, by this host's libm (no device)."""
    t = np.zeros((5, 4), np.int32)
    rc = _lib.load().ps_debug_gradient_tie_table(int(k), _p(t))
    if rc != PS_OK:
        raise PsError(rc, "ps_debug_gradient_tie_table")
    return t
