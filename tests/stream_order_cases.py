"""One stream-order case per asynchronous entry point of the library (include/putslam_hip.h: every ps_*_device whose first
parameter is the context), keyed by its C name; tests/test_gpu_stream_handover.py runs them, tests/test_stream_order_table_host.py
holds the table to the header.  Nothing here touches the GPU at import.

TABLE[name] = Entry(prep, drains).  prep(k, ctx) builds the seeded input k (0 or 1: different results) at the smallest shape that
gives a non-trivial output and returns a Case (the context is needed because the pyramid sets, the detector and the pose sets a
loop batch reads are made by it):

  inputs     the device tensors the call reads, holding their STALE content: a valid, empty input (zero images, counts 0, slot
             0, pairs (0, 0), zero descriptors) -- never a sentinel, so that a lost race shows as wrong bytes and never as a fault;
  finals     the same tensors with the real values (a test copies finals -> inputs on the stream under test);
  call(ctx, direct=False)   through the device_batch wrapper; direct=True: on the stream the context has (use_torch_stream=False);
  outputs()  the tensors to compare, pre-filled before the call; norm(clones) clears the rows beyond a count, which nobody writes;
  counts()   a tensor that is > 0 everywhere when the call did something.

Object state a call reads (pyramid slots, detector maps, pose sets) is filled in prep by a fully synchronised call on valid
images.  A build has no output tensor: its case queues the build and then the reader (track / describe) and compares the reader's
outputs; build(ctx, direct) and read(ctx, direct) are the two halves.  A reader's case has rebuild(ctx, direct): the same slots
built again from other images.

drains: the wrapper synchronises the host (torch's current stream) before it queues.

The second half of the module is the front-end chain detect -> thin -> gather -> describe -> track -> select: its scene, the
restatements chained on the CPU (chain_reference) and the device chain (chain_device)."""
import contextlib
import functools
import gc
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import (EST_FIXED, EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, detect_params,  # noqa: E402
                              make_config)

Entry = namedtuple("Entry", "prep drains")

CAP, NK = 64, [40, 64]
DEV = "cuda:0"

EXEMPT = {"ps_pack_records_device": "takes its stream as an argument: the caller orders it, the context's stream is not used"}


class Case:
    def __init__(self, inputs, finals, call, outputs, counts, norm=None, **more):
        self.inputs, self.finals, self.call, self.outputs, self.counts = inputs, finals, call, outputs, counts
        self.norm = norm or (lambda got: list(got))
        self.__dict__.update(more)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stale(finals):
    import torch
    return [torch.zeros_like(f) for f in finals]


def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device=DEV)


def _synchronize():
    import torch
    torch.cuda.synchronize()


@contextlib.contextmanager
def quiet_collector():
    """The timed part of a stream-order test: collect what earlier tests left behind, then hold the collector off.  A context or a
    handle that a reference cycle kept alive past its test (the record of a pytest.raises holds the frame that holds it) is destroyed
    by whichever collection finds it, and a destroy waits for the device: inside the timed call that reads as a call that
    synchronised the host (9.7 ms to queue under a ballast of 9.9 ms, seen once in a whole-suite run; 0.02 .. 0.12 ms otherwise)."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def mask_rows(t, n):
    """t (P, cap, ...) with the rows beyond n[p], which are not written, cleared."""
    import torch
    cols = torch.arange(t.shape[1], device=t.device).reshape((1, -1) + (1,) * (t.dim() - 2))
    return torch.where(cols < n.reshape((-1,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t))


def _results(b):
    return [b.matches, b.num_matches, b.mask, b.pose, b.stats]


def _set_tensors(s):
    return [s.desc, s.pts, s.nkpts]


# ---------------------------------------------------------------- frame pairs, binary and float rows
def _prep_vo(k, ctx):
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    seq = synth.make_sequence(2, CAP, config=3, index=5100 + k)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, keep = make_config(EST_FIXED, 64, seed=11 + k)
    fs = FrameSetDevice(seq["desc"], seq["pts"], NK)
    late = FrameSetDevice(np.zeros_like(seq["desc"]), np.zeros_like(seq["pts"]), [0, 0])
    out = PairBatchDevice([[0, 1]], CAP)
    return Case(_set_tensors(late), _set_tensors(fs),
                lambda c, direct=False: run_pairs(c, prm, cfg, TUM_FR1_K, late, out, use_torch_stream=not direct),
                lambda: _results(out), lambda: out.num_matches, keep=keep)


def _float_frames(k):
    from putslam_amd.device_batch import FrameSetF32Device
    seq = synth.make_float_sequence(2, CAP, "surf", index=5500 + k)
    fs = FrameSetF32Device(seq["fdesc"], seq["pts"], NK)
    late = FrameSetF32Device(np.zeros_like(seq["fdesc"]), np.zeros_like(seq["pts"]), [0, 0])
    return fs, late


def _prep_match_l2(k, ctx):
    from putslam_amd.device_batch import PairBatchDevice, run_match_l2
    fs, late = _float_frames(k)
    out = PairBatchDevice([[0, 1]], CAP)
    return Case(_set_tensors(late), _set_tensors(fs), lambda c, direct=False: run_match_l2(c, late, out, use_torch_stream=not direct),
                lambda: [out.matches, out.num_matches], lambda: out.num_matches)


def _prep_vo_l2(k, ctx):
    from putslam_amd.device_batch import PairBatchDevice, run_vo_pairs_l2
    fs, late = _float_frames(k)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, keep = make_config(EST_FIXED, 64, seed=21 + k)
    out = PairBatchDevice([[0, 1]], CAP)
    return Case(_set_tensors(late), _set_tensors(fs),
                lambda c, direct=False: run_vo_pairs_l2(c, prm, cfg, TUM_FR1_K, late, out, use_torch_stream=not direct),
                lambda: _results(out), lambda: out.num_matches, keep=keep)


# ---------------------------------------------------------------- the filters
def _kept_case(stale, final, fn):
    """A filter that returns (kept (F, cap), nkept (F,)) in blocks of its own."""
    res = []

    def call(c, direct=False):
        del res[:]
        res.extend(fn(c, *stale))
    return Case(stale, final, call, lambda: list(res), lambda: res[1], lambda got: [mask_rows(got[0], got[1]), got[1]])


def _prep_dbscan(k, ctx):
    from putslam_amd.device_batch import dbscan_thin_device
    rng = np.random.default_rng(5200 + k)
    centres = rng.uniform(40.0, 600.0, (2, 8, 2))
    xy = (centres[np.arange(2)[:, None], rng.integers(0, 8, (2, CAP))] + rng.normal(0.0, 3.0, (2, CAP, 2))).astype(np.float32)
    xy[:, ::5] = rng.uniform(0.0, 640.0, (2, len(range(0, CAP, 5)), 2))          # (and some keypoints on their own)
    octave = rng.integers(0, 4, (2, CAP)).astype(np.int32)
    final = [_up(xy), _up(np.array(NK, np.int32)), _up(octave)]
    return _kept_case(_stale(final), final, dbscan_thin_device)


def _prep_exclude(k, ctx):
    from putslam_amd import api
    from putslam_amd.device_batch import exclude_device
    rng = np.random.default_rng(5300 + k)
    e3 = (rng.uniform(-1.0, 1.0, (2, CAP, 3)) + [0, 0, 3.0]).astype(np.float32)
    e2 = rng.uniform(0.0, 600.0, (2, CAP, 2)).astype(np.float32)
    c3, c2 = e3.copy(), e2.copy()                       # every candidate on an existing feature, but for every other one
    c3[:, ::2] += rng.uniform(0.5, 1.0, (2, CAP // 2, 3)).astype(np.float32)
    c2[:, ::2] += np.float32(50.0)
    counts = np.array(NK, np.int32)
    rule = api.rule_new_map_features(0.03, 2.0, 200)
    final = [_up(a) for a in (c3, c2, counts, e3, e2, counts)]
    return _kept_case(_stale(final), final, lambda c, *t: exclude_device(c, rule, *t))


# ---------------------------------------------------------------- guided map matching, binary and float rows
def _map_case(k, ransac, l2):
    """One (map view, frame) pair: the view's features are the frame's keypoints, a centimetre off, their rows a little noisy."""
    from putslam_amd import device_batch as D
    rng = np.random.default_rng(5400 + k)
    level = np.zeros((1, CAP), np.int32)
    if l2:
        seq = synth.make_float_sequence(1, CAP, "surf", index=5450 + k)
        desc = seq["fdesc"]
        vdesc = (desc + rng.normal(0.0, 0.01, desc.shape)).astype(np.float32)
        Set, Batch = D.FrameSetF32Device, D.MapBatchF32Device
        run = (D.run_map_pairs_l2, D.run_match_xyz_l2)
    else:
        seq = synth.make_sequence(1, CAP, config=3, index=5400 + k)
        desc = seq["desc"]
        vdesc = desc ^ np.packbits(rng.random((1, CAP, 256)) < 0.03, axis=2)
        Set, Batch = D.FrameSetDevice, D.MapBatchDevice
        run = (D.run_map_pairs, D.run_match_xyz)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)
    views, frames = Set(vdesc, vpos, [CAP]), Set(desc, seq["pts"], [CAP])
    late = [Set(np.zeros_like(desc), np.zeros_like(vpos), [0]) for _ in range(2)]
    out = Batch(late[0], level, late[1], level, [[0, 0]], 4 * CAP)
    inputs, finals = [t for s in late for t in _set_tensors(s)], [t for s in (views, frames) for t in _set_tensors(s)]
    if ransac:
        prm = default_ransac_params(EUCLIDEAN_ERROR)
        cfg, keep = make_config(EST_RANSAC, 487, seed=17 + k)
        return Case(inputs, finals, lambda c, direct=False: run[0](c, prm, cfg, TUM_FR1_K, out, use_torch_stream=not direct),
                    lambda: _results(out), lambda: out.num_matches, keep=keep)
    return Case(inputs, finals, lambda c, direct=False: run[1](c, out, use_torch_stream=not direct),
                lambda: [out.matches, out.num_matches], lambda: out.num_matches)


# ---------------------------------------------------------------- the resident store: views, levels, pose sets, loop closure
def _view_outputs(out):
    return [out.desc, out.pts, out.nkpts, out.view_count, out.map_level, out.feat_idx, out.obs_idx, out.pos_cam, out.uv, out.angle]


def _prep_views(k, ctx, l2=False):
    """Two views of a 64-feature store through a candidate list of every feature; stale: both lists empty."""
    import map_store_f32_ref as fref
    import map_view_ref as vref
    from putslam_amd import device_batch as D
    rng = np.random.default_rng(5600 + k)
    store = vref.make_store(rng, CAP, 30)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 2)
    if l2:
        fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), 64))
        sd, build = fref.store_device(fs), D.build_map_views_l2
        out = D.MapViewsF32Device(2, CAP, 64, sd.device)
    else:
        sd = D.MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                              store["obs_det_dist"], store["num_poses"])
        build, out = D.build_map_views, D.MapViewsDevice(2, CAP, sd.device)
    cam = _up(np.ascontiguousarray(cam_inv.transpose(0, 2, 1)).reshape(-1, 16))
    angd, cand = _up(ang), _up(np.tile(np.arange(CAP, dtype=np.int32), (2, 1)))
    final = [_up(np.array([CAP, CAP - 9], np.int32))]
    stale = _stale(final)

    def call(c, direct=False):
        build(c, sd, cam, angd, 10.0, vref.K_TUM, vref.IMAGE, CAP, cand=cand, cand_counts=stale[0], out=out,
              use_torch_stream=not direct)
    return Case(stale, final, call, lambda: _view_outputs(out), lambda: out.view_count)


def _prep_levels(k, ctx):
    from putslam_amd.device_batch import FrameSetDevice, frame_levels_device
    seq = synth.make_sequence(2, CAP, config=3, index=5700 + k)
    rng = np.random.default_rng(5700 + k)
    fs = FrameSetDevice(seq["desc"], seq["pts"], NK)
    late = FrameSetDevice(np.zeros_like(seq["desc"]), np.zeros_like(seq["pts"]), [0, 0])
    final = [fs.pts, fs.nkpts, _up(rng.integers(1, 8, (2, CAP)).astype(np.int32)),
             _up(np.linalg.norm(seq["pts"].astype(np.float64), axis=2) * rng.uniform(0.8, 1.25, (2, CAP)))]
    stale = [late.pts, late.nkpts] + _stale(final[2:])
    res = []

    def call(c, direct=False):
        del res[:]
        res.append(frame_levels_device(c, late, stale[2], stale[3], use_torch_stream=not direct))
    return Case(stale, final, call, lambda: list(res), lambda: (res[0] != 0).sum().reshape(1))


def _loop_scene(k, l2):
    """(device store, obs_point3d, its float rows' store or None): a 64-feature map over poses 0 .. 3 and a true loop of 48
    features between the poses 4 and 5 (loop_closure_ref.plant_loop / map_store_f32_ref.plant_loop)."""
    import loop_closure_ref as lref
    import map_store_f32_ref as fref
    rng = np.random.default_rng(5800 + k)
    store, p3d = lref.make_scene(rng, CAP, 4, max_obs=3, extra_poses=2)
    feats, side = lref.unpack(store, p3d), {}
    if l2:
        fref.plant_loop(rng, feats, side, 4, 5, range(48), 64)
    else:
        lref.plant_loop(rng, feats, 4, 5, range(48))
    store, p3d = lref.pack(store, feats)
    if not l2:
        return lref.store_device(store), p3d
    rows = fref.unit_rows(rng, len(store["obs_pose"]), 64)
    start = store["obs_start"]
    for f in range(len(store["pos"])):
        for o in range(int(start[f]), int(start[f + 1])):
            r = side.get((f, int(store["obs_pose"][o])))
            if r is not None:
                rows[o] = r
    return fref.store_device(fref.float_store(store, rows)), p3d


def _set_outputs(out):
    return [out.desc, out.pts, out.nkpts, out.set_count, out.feat_idx, out.obs_idx]


def _prep_sets(k, ctx, l2=False):
    """The sets of the two poses of the loop; stale: pose 0 twice."""
    from putslam_amd import device_batch as D
    sd, p3d = _loop_scene(k, l2)
    p3d = _up(p3d)
    final = [_up(np.array([4, 5], np.int32))]
    stale = _stale(final)
    out = D.PoseSetsF32Device(2, CAP, 64, sd.device) if l2 else D.PoseSetsDevice(2, CAP, sd.device)
    build = D.build_pose_sets_l2 if l2 else D.build_pose_sets
    return Case(stale, final, lambda c, direct=False: build(c, sd, p3d, stale[0], CAP, out=out, use_torch_stream=not direct),
                lambda: _set_outputs(out), lambda: out.set_count)


def _prep_loop(k, ctx, l2=False):
    """One candidate, the two sets of the loop; stale: the pair (0, 0), the first set against itself.  The sets are built here,
    under synchronisation."""
    from putslam_amd import device_batch as D
    sd, p3d = _loop_scene(k, l2)
    poses = np.array([4, 5], np.int32)
    sets = (D.build_pose_sets_l2 if l2 else D.build_pose_sets)(ctx, sd, p3d, poses, CAP)
    _synchronize()
    b = (D.LoopBatchF32Device if l2 else D.LoopBatchDevice)(sets, [[0, 0]])
    prm = default_ransac_params(EUCLIDEAN_ERROR, lc=True)
    cfg, keep = make_config(EST_RANSAC, 487, seed=41 + k)
    run = D.run_loop_pairs_l2 if l2 else D.run_loop_pairs
    return Case([b.pairs], [_up(np.array([[0, 1]], np.int32))],
                lambda c, direct=False: run(c, prm, cfg, TUM_FR1_K, b, use_torch_stream=not direct),
                lambda: _results(b) + [b.ratio, b.closed, b.num_paired, b.paired_rows, b.paired_feat], lambda: b.num_matches, keep=keep)


# ---------------------------------------------------------------- the front end: KLT, FAST, ORB
KLT_SHAPE, ORB_SHAPE = (48, 64), (80, 96)


def _klt_images(seed):
    import klt_ref as K
    return _up(np.stack([K.smooth_texture(*KLT_SHAPE, 1, seed=seed)[:, :, 0],
                         K.smooth_texture(*KLT_SHAPE, 1, seed=seed, shift=(-1.3, 0.7))[:, :, 0]]))


def _prep_klt(k, ctx, build):
    """Forty points of a 48 x 64 pair tracked from slot 0 to slot 1.  build: the case of ps_klt_pyramids_build_device (inputs:
    the images; the slots hold other images before); else that of ps_klt_track_device (inputs: pairs, points, counts)."""
    import klt_ref as K
    import torch
    from putslam_amd import device_batch as D
    images, other = _klt_images(11 + k), _klt_images(31 + k)
    pyr = D.KltPyramids(ctx, *KLT_SHAPE, 1, 2)
    pyr.build(other if build else images)
    _synchronize()
    real = [_up(np.array([[0, 1]], np.int32)), _up(K.random_points(*KLT_SHAPE, CAP, 3 + k)[None]), _up(np.array([40], np.int32))]
    out = [_zeros((1, CAP, 2), torch.float32), _zeros((1, CAP), torch.uint8), _zeros((1, CAP), torch.float32)]
    final = [images] if build else real
    stale = _stale(final)
    img_in = stale[0] if build else images
    pairs, prev, counts = real if build else stale

    def do_build(c, direct=False):
        pyr.build(img_in, use_torch_stream=not direct)

    def read(c, direct=False):
        D.track_klt_pairs(c, pyr, pairs, prev, counts, None, *out, use_torch_stream=not direct)

    def call(c, direct=False):
        if build:
            do_build(c, direct)
        read(c, direct)
    _synchronize()
    return Case(stale, final, call, lambda: list(out), lambda: out[1].sum().reshape(1), pyr=pyr, build=do_build, read=read,
                rebuild=lambda c, direct=False: pyr.build(other, use_torch_stream=not direct))


def _prep_select(k, ctx):
    from putslam_amd.device_batch import select_tracked
    rng = np.random.default_rng(5900 + k)
    final = [_up(rng.uniform(0, 64, (1, CAP, 2)).astype(np.float32)), _up((rng.uniform(size=(1, CAP)) < 0.85).astype(np.uint8)),
             _up(rng.uniform(0, 4, (1, CAP)).astype(np.float32)), _up(np.array([50], np.int32))]
    stale = _stale(final)
    res = []

    def call(c, direct=False):
        del res[:]
        res.extend(select_tracked(c, *stale, 3.0, 4.0, use_torch_stream=not direct))
    return Case(stale, final, call, lambda: list(res), lambda: res[1],
                lambda got: [mask_rows(got[0], got[1]), got[1], mask_rows(got[2], got[1]), mask_rows(got[3], got[1])])


def _prep_detect(k, ctx, share=None):
    """Two 48 x 64 frames (rectangles with noise; noise) through a 2 x 2 grid.  share: an earlier case whose detector is used."""
    import fast_ref as F
    import torch
    from putslam_amd import device_batch as D
    rows, cols = KLT_SHAPE
    final = [_up(np.stack([F.blocks(rows, cols, 3 + k, 30, noise=6), F.noise256(rows, cols, 7 + k)]))]
    stale = _stale(final)
    prm = detect_params(20, True, 2, 2, CAP)
    out = [_zeros((2, CAP, 2), torch.float32), _zeros((2, CAP), torch.float32), _zeros((2,), torch.int32)]
    if share is None:
        det = D.FastDetector(ctx, rows, cols, 1, 2)
        D.detect_features_batch(ctx, det, _up(np.stack([F.noise4(rows, cols, 5), F.noise4(rows, cols, 6)])), prm, CAP)
    else:
        det = share.det
    _synchronize()
    return Case(stale, final, lambda c, direct=False: D.detect_features_batch(c, det, stale[0], prm, CAP, *out, use_torch_stream=not direct),
                lambda: list(out), lambda: out[2], det=det)


def _orb_images(seed):
    import orb_ref as R
    return _up(np.stack([R.texture(*ORB_SHAPE, seed), R.texture(*ORB_SHAPE, seed + 10)]))


def _prep_orb(k, ctx, build):
    """40 and 64 key points of two 80 x 96 frames, every octave.  build: the case of ps_orb_pyramids_build_device; else that of
    ps_describe_features_device (inputs: slots, key points, counts)."""
    import orb_ref as R
    import torch
    from putslam_amd import device_batch as D
    images, other = _orb_images(3 + k), _orb_images(23 + k)
    pyr = D.OrbPyramids(ctx, *ORB_SHAPE, 1, 2)
    pyr.build(other if build else images)
    _synchronize()
    kp = [R.random_keypoints(CAP, *ORB_SHAPE, 8, seed=60 + 2 * k + f) for f in range(2)]
    real = [_up(np.array([0, 1], np.int32))] + [_up(np.stack([p[i] for p in kp])) for i in range(3)] + [_up(np.array(NK, np.int32))]
    out = [_zeros((2, CAP, 32), torch.uint8), _zeros((2, CAP), torch.int32), _zeros((2,), torch.int32)]
    final = [images] if build else real
    stale = _stale(final)
    img_in = stale[0] if build else images
    args = real if build else stale

    def do_build(c, direct=False):
        pyr.build(img_in, use_torch_stream=not direct)

    def read(c, direct=False):
        D.describe_features_batch(c, pyr, *args, *out, use_torch_stream=not direct)

    def call(c, direct=False):
        if build:
            do_build(c, direct)
        read(c, direct)
    _synchronize()
    return Case(stale, final, call, lambda: list(out), lambda: out[2], pyr=pyr, build=do_build, read=read,
                rebuild=lambda c, direct=False: pyr.build(other, use_torch_stream=not direct))


TABLE = {
    "ps_vo_pairs_device": Entry(_prep_vo, False),
    "ps_dbscan_thin_device": Entry(_prep_dbscan, False),
    "ps_exclude_device": Entry(_prep_exclude, False),
    "ps_match_xyz_device": Entry(lambda k, ctx: _map_case(k, False, False), False),
    "ps_map_pairs_device": Entry(lambda k, ctx: _map_case(k, True, False), False),
    "ps_map_views_device": Entry(_prep_views, True),
    "ps_frame_levels_device": Entry(_prep_levels, True),
    "ps_pose_sets_device": Entry(_prep_sets, True),
    "ps_loop_pairs_device": Entry(_prep_loop, False),
    "ps_match_l2_device": Entry(_prep_match_l2, False),
    "ps_vo_pairs_l2_device": Entry(_prep_vo_l2, False),
    "ps_match_xyz_l2_device": Entry(lambda k, ctx: _map_case(k, False, True), False),
    "ps_map_pairs_l2_device": Entry(lambda k, ctx: _map_case(k, True, True), False),
    "ps_map_views_l2_device": Entry(lambda k, ctx: _prep_views(k, ctx, True), True),
    "ps_pose_sets_l2_device": Entry(lambda k, ctx: _prep_sets(k, ctx, True), True),
    "ps_loop_pairs_l2_device": Entry(lambda k, ctx: _prep_loop(k, ctx, True), False),
    "ps_klt_pyramids_build_device": Entry(lambda k, ctx: _prep_klt(k, ctx, True), False),
    "ps_klt_track_device": Entry(lambda k, ctx: _prep_klt(k, ctx, False), False),
    "ps_klt_select_device": Entry(_prep_select, False),
    "ps_detect_features_device": Entry(_prep_detect, False),
    "ps_orb_pyramids_build_device": Entry(lambda k, ctx: _prep_orb(k, ctx, True), False),
    "ps_describe_features_device": Entry(lambda k, ctx: _prep_orb(k, ctx, False), False),
}


# ---------------------------------------------------------------- the front-end chain
CHAIN = dict(rows=96, cols=128, cap=128, detect=(20, True, 2, 2, 128), dbscan=(4.0, 2), klt=(7, 3, 30, 0.01), select=(4.0, 8.0))
# what the restatements alone give on the scene (tests/test_stream_order_table_host.py): every step removes rows, none all
CHAIN_COUNTS = dict(detected=[128, 128], thinned=[89, 89], described=[22, 23], tracked=87, selected=57)


def chain_images():
    """Two 96 x 128 frames cut from one texture 2 px apart: (x, y) of the first is (x + 2, y) of the second."""
    import orb_ref as R
    base = R.texture(CHAIN["rows"], CHAIN["cols"] + 2, 11)
    return [np.ascontiguousarray(base[:, 2:]), np.ascontiguousarray(base[:, :-2])]


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The restatements chained on the CPU: per frame detected xy, the rows DBScan keeps, their descriptors and kept indices; for
    the pair (0, 1) the track of frame 0's kept rows and its selection."""
    import dbscan_ref_py as B
    import fast_ref as F
    import klt_ref as K
    import orb_ref as R
    imgs = chain_images()
    frames = []
    for img in imgs:
        xy, resp = F.detect_closed(img, *CHAIN["detect"])
        keep = B.dbscan_keep(xy, None, *CHAIN["dbscan"])
        kxy = xy[keep]
        desc, kept = R.describe(R.pyramid(img), kxy, np.full(len(kxy), -1, np.float32), np.zeros(len(kxy), np.int32))
        frames.append(dict(xy=xy, response=resp, keep=keep, kxy=kxy, desc=desc, kept=kept))
    nxt, status, err = K.track(imgs[0], imgs[1], frames[0]["kxy"], *CHAIN["klt"])
    sel, matches = K.select_pairwise(nxt, status, err, *CHAIN["select"])
    return dict(frames=frames, next=nxt, status=status, err=err, selected=sel, matches=matches)


class ChainDevice:
    """The detector and the two pyramid sets of the chain, made once (their creation synchronises)."""

    def __init__(self, ctx):
        from putslam_amd import device_batch as D
        r, c = CHAIN["rows"], CHAIN["cols"]
        self.ctx = ctx
        self.det, self.orb, self.klt = D.FastDetector(ctx, r, c, 1, 2), D.OrbPyramids(ctx, r, c, 1, 2), D.KltPyramids(ctx, r, c, 1, 2, 7, 3)
        valid = _up(np.stack(chain_images()[::-1]))      # every slot and map filled from valid images, under synchronisation
        D.detect_features_batch(ctx, self.det, valid, detect_params(*CHAIN["detect"]), CHAIN["cap"])
        self.orb.build(valid)
        self.klt.build(valid)
        self.pairs = _up(np.array([[0, 1]], np.int32))   # (uploaded here: a copy from pageable host memory waits for the stream)
        _synchronize()

    def run(self, images, step=lambda: None):
        """The chain on torch's current stream, step() after every link; returns the clones, by name."""
        import torch
        from putslam_amd import device_batch as D
        ctx, cap = self.ctx, CHAIN["cap"]
        dev = images.device
        xy, resp, counts = D.detect_features_batch(ctx, self.det, images, detect_params(*CHAIN["detect"]), cap)
        step()
        kept, nkept = D.dbscan_thin_device(ctx, xy, counts, None, *CHAIN["dbscan"])
        step()
        live = torch.arange(cap, device=dev)[None, :] < nkept[:, None]          # (the rows beyond a count are not written)
        idx = torch.where(live, kept, torch.zeros_like(kept)).long().clamp(0, cap - 1)
        kxy = torch.where(live[:, :, None], torch.gather(xy, 1, idx[:, :, None].expand(-1, -1, 2)), torch.zeros_like(xy)).contiguous()
        step()
        self.orb.build(images)
        angle, octave = torch.full((2, cap), -1.0, dtype=torch.float32, device=dev), torch.zeros((2, cap), dtype=torch.int32, device=dev)
        desc, dkept, dnum = D.describe_features_batch(ctx, self.orb, torch.arange(2, dtype=torch.int32, device=dev), kxy, angle, octave,
                                                      nkept)
        step()
        self.klt.build(images)
        nxt, status, err = D.track_klt_pairs(ctx, self.klt, self.pairs, kxy[0:1], nkept[0:1], None)
        step()
        matches, num, spts, sidx = D.select_tracked(ctx, nxt, status, err, nkept[0:1], *CHAIN["select"])
        step()
        out = dict(xy=xy, response=resp, counts=counts, kept=torch.where(live, kept, torch.zeros_like(kept)), nkept=nkept, kxy=kxy,
                   desc=desc, dkept=dkept, dnum=dnum, next=nxt, status=status, err=err, num=num, matches=mask_rows(matches, num),
                   spts=mask_rows(spts, num), sidx=mask_rows(sidx, num))
        return {k: t.clone() for k, t in out.items()}

    def close(self):
        for o in (self.det, self.orb, self.klt):
            o.close()
