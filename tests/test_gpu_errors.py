"""Error behaviour of the C ABI (include/putslam_hip.h: negative PsStatus + ps_last_error, outputs reset to the
reference's failure values: identity pose, no inliers) and that a failed call leaves the context usable."""
import ctypes as C

import numpy as np
import pytest

from putslam_amd import _lib, synth
from putslam_amd._abi import (DMATCH_DTYPE, EST_RANSAC, PsRansacStats, TUM_FR1_K, default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

OK, BAD_ARG, NO_DEVICE, HIP, ALLOC, UNSUPPORTED = 0, -1, -2, -3, -4, -5


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture()
def raw():
    L = _lib.load()
    h = C.c_void_p()
    assert L.ps_context_create(0, C.byref(h)) == OK
    yield L, h
    L.ps_context_destroy(h)


def test_context_create_rejects_bad_device():
    L = _lib.load()
    h = C.c_void_p()
    assert L.ps_context_create(-1, C.byref(h)) == BAD_ARG and not h.value
    assert L.ps_context_create(4096, C.byref(h)) == BAD_ARG and not h.value
    assert L.ps_context_create(0, None) == BAD_ARG
    assert L.ps_last_error(None) == b"null context"
    L.ps_context_destroy(None)          # harmless


def test_match_argument_errors_then_success(raw):
    L, h = raw
    r = np.random.default_rng(1)
    q = r.integers(0, 256, (100, 32), dtype=np.uint8)
    t = r.integers(0, 256, (90, 32), dtype=np.uint8)
    out = np.zeros(100, DMATCH_DTYPE)
    n = C.c_int(7)
    assert L.ps_match_hamming256(h, None, 100, 32, _p(t), 90, 32, _p(out), C.byref(n)) == BAD_ARG and n.value == 0
    assert b"bad argument" in L.ps_last_error(h)
    assert L.ps_match_hamming256(h, _p(q), 100, 32, _p(t), 90, 32, None, C.byref(n)) == BAD_ARG
    assert L.ps_match_hamming256(h, _p(q), -1, 32, _p(t), 90, 32, _p(out), C.byref(n)) == BAD_ARG
    assert L.ps_match_hamming256(h, _p(q), 100, 16, _p(t), 90, 32, _p(out), C.byref(n)) == UNSUPPORTED  # short rows
    assert b"32 bytes" in L.ps_last_error(h)
    assert L.ps_match_hamming256(h, _p(q), 20000, 32, _p(t), 90, 32, _p(out), C.byref(n)) == UNSUPPORTED
    # empty sides are not errors: BFMatcher returns no matches
    assert L.ps_match_hamming256(h, _p(q), 0, 32, _p(t), 90, 32, _p(out), C.byref(n)) == OK and n.value == 0
    assert L.ps_match_hamming256(h, _p(q), 100, 32, _p(t), 0, 32, _p(out), C.byref(n)) == OK and n.value == 0
    # the context still works, and a successful call clears the message
    assert L.ps_match_hamming256(h, _p(q), 100, 32, _p(t), 90, 32, _p(out), C.byref(n)) == OK and n.value > 0
    assert L.ps_last_error(h) == b""


def test_ransac_argument_errors_reset_outputs(raw, oracle):
    L, h = raw
    a, b = synth.make_pair(300, config=2, index=3)
    m = oracle.match_hamming256(a["desc"], b["desc"])
    prm = default_ransac_params(1)
    cfg, _ = make_config(EST_RANSAC, 487, seed=9)
    K = np.ascontiguousarray(TUM_FR1_K, np.float32)
    prev, cur = np.ascontiguousarray(a["pts"], np.float32), np.ascontiguousarray(b["pts"], np.float32)
    pose = np.full(16, 7.0, np.float32)
    inl = np.zeros(len(m), DMATCH_DTYPE)
    ninl = C.c_int(99)
    mask = np.full(len(m), 5, np.uint8)
    st = PsRansacStats()

    def call(prm_=prm, cfg_=cfg, matches=m, nprev=len(prev), ncur=len(cur), pose_=pose):
        return L.ps_ransac_rigid3d(h, C.byref(prm_) if prm_ is not None else None,
                                   C.byref(cfg_) if cfg_ is not None else None, _p(K), _p(prev), nprev, _p(cur), ncur,
                                   _p(matches), len(matches), _p(pose_) if pose_ is not None else None, _p(inl),
                                   C.byref(ninl), _p(mask), C.byref(st))

    def is_reset():
        return np.array_equal(pose.reshape(4, 4), np.eye(4, dtype=np.float32)) and ninl.value == 0

    assert call(prm_=None) == BAD_ARG and is_reset()
    pose[:] = 7.0
    bad = default_ransac_params(1)
    bad.usedPairs = 4
    assert call(prm_=bad) == UNSUPPORTED and is_reset() and b"usedPairs" in L.ps_last_error(h)
    for H in (0, -3, (1 << 20) + 1):
        c2, _ = make_config(EST_RANSAC, 487, seed=9)
        c2.numHypotheses = H
        pose[:] = 7.0
        assert call(cfg_=c2) == BAD_ARG and is_reset()
    c3, _ = make_config(EST_RANSAC, 487, seed=9)
    c3.estimator = 17
    assert call(cfg_=c3) == BAD_ARG and b"estimator" in L.ps_last_error(h)
    m2 = m.copy()
    m2["trainIdx"][5] = len(cur)                       # one index past the end
    pose[:] = 7.0
    assert call(matches=m2) == BAD_ARG and is_reset() and b"out of range" in L.ps_last_error(h)
    m2 = m.copy()
    m2["queryIdx"][0] = -1
    assert call(matches=m2) == BAD_ARG
    assert call(pose_=None) == BAD_ARG
    # and the same context then produces the oracle's answer
    assert call() == OK
    c = oracle.ransac_rigid3d(prm, cfg, TUM_FR1_K, a["pts"], b["pts"], m)
    assert np.array_equal(pose.reshape(4, 4).T.view(np.uint32), np.asarray(c["pose"], np.float32).view(np.uint32))  # ABI: column-major
    assert ninl.value == len(c["inliers"])


def test_null_context_is_rejected_everywhere():
    L = _lib.load()
    n = C.c_int(0)
    buf = np.zeros(64, np.uint8)
    assert L.ps_context_synchronize(None) == BAD_ARG
    assert L.ps_match_hamming256(None, _p(buf), 1, 32, _p(buf), 1, 32, _p(buf), C.byref(n)) == BAD_ARG
    assert L.ps_context_enable_timing(None, 1) == BAD_ARG
    assert L.ps_context_set_stream(None, None) == BAD_ARG


def test_minutes_long_batch_is_refused_before_anything_is_allocated():
    """complete scoring (option "prune" = 0) of a batch under USAC's cap -- 20 000 pairs x 850 000 hypotheses x
    16 384 matches > 2e14 evaluations -- is refused with PS_ERR_UNSUPPORTED.  The refusal used to stand BEHIND the request for the
    per-hypothesis counts block (4 bytes x pairs x hypotheses = 68 GB here, 400 GB for larger batches: an allocation failure or a
    huge allocation instead of the message); now it comes first and the context's arena stays as small as it was."""
    import torch
    from putslam_amd import api
    from putslam_amd._abi import EST_USAC
    c = api.Context(0)
    c.set_option("prune", 0)
    before = c.get_option("arena_mib")
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda")          # never touched: the call is refused before any launch
    p = dummy.data_ptr()
    prm = default_ransac_params(0)
    cfg, _ = make_config(EST_USAC, 850000, seed=1)
    with pytest.raises(api.PsError) as e:
        c.vo_pairs_device(prm, cfg, TUM_FR1_K, api.DeviceFrames(p, p, p, 20001, 16384), p, 20000, api.DeviceResults(p, p, p, p, p))
    assert e.value.code == UNSUPPORTED and "run for minutes" in str(e.value)
    assert c.get_option("arena_mib") <= before + 16                       # (the stop table of the cap: 850 000 doubles)
    c.set_option("prune", 1)
    c.close()


# ---------------------------------------------------------------- PsFrameSet strides and the stream hand-over, call by call
# Every device entry point that takes a PsFrameSet applies ONE stride rule, and every asynchronous entry point that uses the
# context's scratch marks its queued work for a later ps_context_set_stream.  The smallest shapes: 2 frames / views of 64
# keypoints, one pair, a 64-feature map store.  Each _prep_*(k, dpad, ppad) builds the seeded inputs k of one entry point with
# dpad / ppad bytes between consecutive frames' descriptor / point blocks and returns (call, outs): call(ctx, **how) issues the
# call with the frame set's view altered by `how` (_Set.view), outs are the output tensors, filled with the sentinel beforehand.
CAP, SENT = 64, 0x5A
STRIDE_CASES = [dict(dstride=CAP * 32 + 8), dict(dstride=CAP * 32 - 16), dict(desc_off=8), dict(pstride=CAP * 12 + 2),
                dict(pstride=CAP * 12 - 4)]


class _Set:
    """A device frame set of CAP keypoints a frame; desc = None: an output set, all sentinel."""

    def __init__(self, desc, pts, nkpts, dpad=0, ppad=0):
        import torch
        F = len(nkpts)
        d = np.full((F, CAP * 32 + dpad), SENT, np.uint8)
        p = np.full((F, CAP * 12 + ppad), SENT, np.uint8)
        if desc is not None:
            d[:, :CAP * 32] = np.ascontiguousarray(desc, np.uint8).reshape(F, -1)
            p[:, :CAP * 12] = np.ascontiguousarray(pts, np.float32).reshape(F, -1).view(np.uint8)
        self.desc, self.pts = torch.from_numpy(d).cuda(), torch.from_numpy(p).cuda()
        self.nkpts = torch.from_numpy(np.ascontiguousarray(nkpts, np.int32)).cuda()
        self.F, self.dpad, self.ppad = F, dpad, ppad

    def view(self, dstride=None, pstride=None, desc_off=0, no_desc=False):
        from putslam_amd import api
        ds = (CAP * 32 + self.dpad if self.dpad else 0) if dstride is None else dstride
        ps = (CAP * 12 + self.ppad if self.ppad else 0) if pstride is None else pstride
        return api.DeviceFrames(None if no_desc else self.desc.data_ptr() + desc_off, self.pts.data_ptr(), self.nkpts.data_ptr(),
                                self.F, CAP, ds, ps)


def _outs(**shapes):
    import torch
    return {k: torch.full(s, SENT, dtype=torch.uint8, device="cuda") for k, s in shapes.items()}


def _bytes(outs):
    """The outputs as host bytes; a frame set among them without the padding between its frames."""
    return {k: t.cpu().numpy()[:, :CAP * (32 if k == "setDesc" else 12 if k == "setPts" else 1 << 20)].tobytes()
            for k, t in outs.items()}


def _results(outs):
    from putslam_amd import api
    return api.DeviceResults(*(outs[k].data_ptr() for k in ("matches", "numMatches", "mask", "pose", "stats")))


def _pair_outs(rows):
    from putslam_amd._abi import STATS_DTYPE
    return _outs(matches=(1, rows * 16), numMatches=(1, 4), mask=(1, rows), pose=(1, 64), stats=(1, STATS_DTYPE.itemsize))


def _prep_vo(k, dpad=0, ppad=0):
    import torch
    seq = synth.make_sequence(2, CAP, config=3, index=4100 + k)
    fs = _Set(seq["desc"], seq["pts"], seq["nkpts"], dpad, ppad)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    outs = _pair_outs(CAP)
    prm = default_ransac_params(0)
    cfg, keep = make_config(EST_RANSAC, 487, seed=7 + k)

    def call(c, **how):
        c.vo_pairs_device(prm, cfg, TUM_FR1_K, fs.view(**how), pairs.data_ptr(), 1, _results(outs))
    call.keep = (keep, pairs)
    return call, outs


def _prep_map(k, dpad=0, ppad=0, ransac=False, which="maps"):
    """One (map view, frame) pair: the view's features are the frame's keypoints, moved by a centimetre, 3 % of the descriptor
    bits flipped.  `which` set of the batch a call's `how` alters."""
    import torch
    from putslam_amd import api
    seq = synth.make_sequence(2, CAP, config=3, index=4200 + k)
    rng = np.random.default_rng(4200 + k)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)
    vdesc = seq["desc"] ^ np.packbits(rng.random((2, CAP, 256)) < 0.03, axis=2)
    sets = dict(maps=_Set(vdesc, vpos, seq["nkpts"], dpad, ppad), frames=_Set(seq["desc"], seq["pts"], seq["nkpts"], dpad, ppad))
    level = torch.from_numpy(rng.integers(0, 3, (2, CAP)).astype(np.int32)).cuda()
    pairs = torch.tensor([[1, 1]], dtype=torch.int32, device="cuda")
    outs = _pair_outs(4 * CAP)
    prm = default_ransac_params(0)
    cfg, keep = make_config(EST_RANSAC, 487, seed=17 + k)

    def call(c, **how):
        v = {n: s.view(**(how if n == which else {})) for n, s in sets.items()}
        b = api.DeviceMapBatch(v["maps"], level.data_ptr(), v["frames"], level.data_ptr(), pairs.data_ptr(), 1, 4 * CAP,
                               api.map_sphere_bound(0.12), 0.55)
        if ransac:
            c.map_pairs_device(prm, cfg, TUM_FR1_K, b, _results(outs))
        else:
            c.match_xyz_device(b, outs["matches"].data_ptr(), outs["numMatches"].data_ptr())
    call.keep = (keep, pairs, level)
    return call, outs


def _prep_views(k, dpad=0, ppad=0):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import map_view_ref as vref
    from putslam_amd._abi import PsMapViewOut, PsMapViewRequest, PsFrameSet
    from putslam_amd.device_batch import MapStoreDevice
    rng = np.random.default_rng(4300 + k)
    store = vref.make_store(rng, 64, 30)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 2)
    sd = MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                        store["obs_det_dist"], store["num_poses"])
    cam = torch.from_numpy(np.ascontiguousarray(cam_inv.transpose(0, 2, 1)).reshape(-1, 16)).cuda()
    angd = torch.from_numpy(np.ascontiguousarray(ang)).cuda()
    views = _Set(None, None, np.full(2, 0x5A5A5A5A, np.int32), dpad, ppad)
    outs = _outs(mapLevel=(2, CAP * 4), viewCount=(2, 4), featIdx=(2, CAP * 4), obsIdx=(2, CAP * 4), posCam=(2, CAP * 24),
                 uv=(2, CAP * 16), angle=(2, CAP * 8))
    outs.update(setDesc=views.desc, setPts=views.pts, setN=views.nkpts.view(torch.uint8).reshape(2, 4))
    rq = PsMapViewRequest()
    rq.camInv, rq.poseAngle = cam.data_ptr(), angd.data_ptr()
    rq.maxAngle, rq.fx, rq.fy, rq.cx, rq.cy, rq.imageW, rq.imageH = (10.0,) + vref.K_TUM + vref.IMAGE
    rq.V = 2

    def call(c, **how):
        f = views.view(**how)
        o = PsMapViewOut(PsFrameSet(f.desc_ptr, f.pts_ptr, f.nkpts_ptr, f.num_frames, f.max_kpts, f.desc_stride, f.pts_stride),
                         *(outs[n].data_ptr() for n in ("mapLevel", "viewCount", "featIdx", "obsIdx", "posCam", "uv", "angle")))
        c.map_views_device(sd.view(), rq, o)
    call.keep = (sd, cam, angd, views)
    return call, outs


def _prep_levels(k, dpad=0, ppad=0):
    import torch
    seq = synth.make_sequence(2, CAP, config=3, index=4400 + k)
    rng = np.random.default_rng(4400 + k)
    fs = _Set(seq["desc"], seq["pts"], seq["nkpts"], dpad, ppad)
    octave = torch.from_numpy(rng.integers(0, 8, (2, CAP)).astype(np.int32)).cuda()
    det = torch.from_numpy(np.linalg.norm(seq["pts"].astype(np.float64), axis=2) * rng.uniform(0.8, 1.25, (2, CAP))).cuda()
    outs = _outs(level=(2, CAP * 4))

    def call(c, **how):
        c.frame_levels_device(fs.view(**how), octave.data_ptr(), det.data_ptr(), outs["level"].data_ptr())
    call.keep = (fs, octave, det)
    return call, outs


def _prep_exclude(k):
    """One frame: 64 candidates, each on an existing feature but for a seeded half of them, which input k moves away."""
    import torch
    from putslam_amd import api
    rng = np.random.default_rng(4500 + k)
    e3 = (rng.uniform(-1.0, 1.0, (1, CAP, 3)) + [0, 0, 3.0]).astype(np.float32)
    e2 = rng.uniform(0.0, 600.0, (1, CAP, 2)).astype(np.float32)
    c3, c2 = e3.copy(), e2.copy()
    away = rng.permutation(CAP)[:CAP // 2]
    c3[0, away] += rng.uniform(0.5, 1.0, (CAP // 2, 3)).astype(np.float32)
    c2[0, away] += 50.0
    t = [torch.from_numpy(a).cuda() for a in (c3, c2, e3, e2)]
    n = torch.full((1,), CAP, dtype=torch.int32, device="cuda")
    outs = _outs(kept=(1, CAP * 4), nkept=(1, 4))
    rule = api.rule_new_map_features(0.03, 2.0, 100000)

    def call(c):
        c.exclude_device(rule, t[0].data_ptr(), t[1].data_ptr(), n.data_ptr(), CAP, t[2].data_ptr(), t[3].data_ptr(), n.data_ptr(), CAP,
                         1, outs["kept"].data_ptr(), outs["nkept"].data_ptr())
    call.keep = (t, n)
    return call, outs


def _count(outs, name):
    return int(outs[name].cpu().numpy().view(np.int32).max())


ENTRY_POINTS = {
    "ps_vo_pairs_device": (_prep_vo, "numMatches"),
    "ps_match_xyz_device/maps": (lambda k, d=0, p=0: _prep_map(k, d, p, False, "maps"), "numMatches"),
    "ps_match_xyz_device/frames": (lambda k, d=0, p=0: _prep_map(k, d, p, False, "frames"), "numMatches"),
    "ps_map_pairs_device/maps": (lambda k, d=0, p=0: _prep_map(k, d, p, True, "maps"), "numMatches"),
    "ps_map_pairs_device/frames": (lambda k, d=0, p=0: _prep_map(k, d, p, True, "frames"), "numMatches"),
    "ps_map_views_device": (_prep_views, "viewCount"),
    "ps_frame_levels_device": (_prep_levels, None),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_frame_set_stride_rule_is_the_same_at_every_entry_point(name):
    """descFrameStride not a multiple of 16 / below dense, desc off its 16-byte alignment, ptsFrameStride not a multiple of 4 /
    below dense: PS_ERR_BAD_ARG and nothing written.  ps_frame_levels_device reads no descriptors: only the points' cases apply,
    and a set whose desc is null is accepted.  The padded layout (dense + 16 / dense + 4) gives the dense layout's bytes."""
    import torch
    from putslam_amd import api
    prep, count = ENTRY_POINTS[name]
    levels = name == "ps_frame_levels_device"
    c = api.Context(0)
    call, outs = prep(0)
    torch.cuda.synchronize()
    untouched = _bytes(outs)
    for how in STRIDE_CASES[3:] if levels else STRIDE_CASES:
        with pytest.raises(api.PsError) as e:
            call(c, **how)
        assert e.value.code == BAD_ARG and ("descFrameStride" if ("dstride" in how or "desc_off" in how) else "ptsFrameStride") in str(e.value), how
        c.synchronize()
        torch.cuda.synchronize()
        assert _bytes(outs) == untouched, how
    call(c)
    c.synchronize()
    dense = _bytes(outs)
    assert dense != untouched and (count is None or _count(outs, count) > 0)
    if levels:
        call2, outs2 = prep(0)
        torch.cuda.synchronize()
        call2(c, no_desc=True)
        c.synchronize()
        assert _bytes(outs2) == dense
    call3, outs3 = prep(0, 16, 4)
    torch.cuda.synchronize()
    call3(c)
    c.synchronize()
    assert _bytes(outs3) == dense
    for k in ("setDesc", "setPts"):                    # an output set: the bytes between its frames are nobody's
        if k in outs3:
            assert bool((outs3[k][:, CAP * (32 if k == "setDesc" else 12):] == SENT).all())
    c.close()


@pytest.mark.parametrize("name", ["ps_match_xyz_device/maps", "ps_map_pairs_device/maps", "ps_exclude_device", "ps_map_views_device",
                                  "ps_frame_levels_device"])
def test_queued_work_is_handed_over_to_the_next_stream(name):
    """A call on stream A, ps_context_set_stream to stream B with no synchronisation in between, the same call with a second
    input: both results are those of two separate synchronised calls, byte for byte (the context's scratch is shared; for
    ps_vo_pairs_device this is test_gpu_batch.py::test_one_context_called_from_two_streams_is_ordered)."""
    import torch
    from putslam_amd import api
    prep = _prep_exclude if name == "ps_exclude_device" else ENTRY_POINTS[name][0]
    c = api.Context(0)
    want = []
    for k in (0, 1):
        call, outs = prep(k)
        torch.cuda.synchronize()
        call(c)
        c.synchronize()
        want.append(_bytes(outs))
    assert want[0] != want[1]
    runs = [prep(0), prep(1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (call, _), st in zip(runs, streams):
        c.set_stream(st.cuda_stream)
        call(c)
    torch.cuda.synchronize()
    assert [_bytes(outs) for _, outs in runs] == want
    c.set_stream(0)
    c.close()
