"""Map views built on the device from a resident feature map (ps_map_views_device, ps_frame_levels_device) against the CPU
restatement of tests/map_view_ref.py, byte for byte: the desc / pts / nkpts / mapLevel rows up to the count, the side arrays and
viewCount; then the chain views -> levels -> ps_map_pairs_device against map_view_ref followed by map_pairs_ref."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_pairs_ref as mref  # noqa: E402
import map_view_ref as vref  # noqa: E402

from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, PS_LEVEL_OCTAVE_MAX, PS_VIEW_INVALID, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

K, IMG = vref.K_TUM, vref.IMAGE


def _store_dev(store):
    from putslam_amd.device_batch import MapStoreDevice
    return MapStoreDevice(store["pos"], store["obs_start"], store["obs_pose"], store["obs_desc"], store["obs_octave"],
                          store["obs_det_dist"], store["num_poses"])


def _build(ctx, sd, cam_inv, ang, max_angle, max_kpts, cand=None, cc=None, vis=False, packed=None, K_=K, image=IMG, out=None):
    from putslam_amd.device_batch import build_map_views
    return build_map_views(ctx, sd, cam_inv, ang, max_angle, K_, image, max_kpts, cand=cand, cand_counts=cc, require_visible=vis,
                           packed_stride=packed, out=out)


# ---------------------------------------------------------------- random stores
@pytest.mark.parametrize("F,N,V,capacity,max_kpts,vis,packed,nan,max_angle", [
    (20000, 400, 64, None, 16384, True, False, 0, 0.5),      # every feature of the store, 64 views
    (20000, 50, 7, 6000, 6000, False, True, 3, 0.3),         # ragged lists, views as packed blocks, NaN table entries
    (3000, 120, 1, 3000, 3000, False, False, 10, 0.25),      # one view
    (3000, 2500, 5, 1200, 1200, True, True, 100, 0.4),       # more poses than the LDS stage holds: the table is read from HBM
    (257, 50, 33, 257, 300, True, False, 1, 10.0),
    (600, 64, 4, None, 600, False, False, 2, 0.35),
])
def test_random_stores_equal_the_reference(ctx, F, N, V, capacity, max_kpts, vis, packed, nan, max_angle):
    rng = np.random.default_rng(F * 131 + N * 7 + V)
    store = vref.make_store(rng, F, N)
    cam_inv, ang, _, _ = vref.make_request(rng, store, V, nan_entries=nan)
    cand, cc = (None, None) if capacity is None else vref.ragged_candidates(rng, F, V, capacity)
    want = vref.build_views(store, cam_inv, ang, max_angle, K, IMG, max_kpts, cand, cc, vis, fast=True)
    counts = [w["viewCount"] for w in want]
    assert max(counts) > 0 and (V == 1 or len(set(counts)) > 1), counts
    stride = (max_kpts * 44 + 15) // 16 * 16 + 256 if packed else None
    got = _build(ctx, _store_dev(store), cam_inv, ang, max_angle, max_kpts, cand, cc, vis, stride).download()
    vref.compare(got, want, what=(F, N, V))
    if F <= 3000 and V <= 5:      # the sequential restatement itself, where the Python loop is affordable
        vref.compare(got, vref.build_views(store, cam_inv, ang, max_angle, K, IMG, max_kpts, cand, cc, vis), what="sequential")


def test_rows_beyond_the_count_are_not_written(ctx):
    from putslam_amd.device_batch import MapViewsDevice
    rng = np.random.default_rng(3)
    store = vref.make_store(rng, 900, 60)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3)
    want = vref.build_views(store, cam_inv, ang, 0.3, K, IMG, 900, require_visible=True)
    sd = _store_dev(store)
    out = MapViewsDevice(3, 900, sd.device)
    for t in (out.desc, out.map_level, out.feat_idx, out.obs_idx):
        t.fill_(0x5A)
    for t in (out.pts, out.pos_cam, out.uv, out.angle):
        t.fill_(-123.0)
    got = _build(ctx, sd, cam_inv, ang, 0.3, 900, vis=True, out=out).download()
    vref.compare(got, want)
    for v, w in enumerate(want):
        n = w["nkpts"]
        assert 0 < n < 900
        assert (got["desc"][v, n:] == 0x5A).all() and (got["pts"][v, n:] == -123.0).all() and (got["mapLevel"][v, n:] == 0x5A).all()
        assert (got["featIdx"][v, n:] == 0x5A).all() and (got["posCam"][v, n:] == -123.0).all() and (got["angle"][v, n:] == -123.0).all()


# ---------------------------------------------------------------- directed edges
def _edge_store(t):
    """A hand-made store under the identity camera (camera frame = global frame) and K_EDGE.  Returns (store, angle table,
    maxAngle, notes) with notes[name] = feature index."""
    MAXA = 0.3
    up = float(np.nextafter(MAXA, 1.0))
    ang = np.array([MAXA, up, 0.2, 0.2, np.nan, 0.1, 0.25, np.nan, 0.05, 0.05], np.float64)
    feats, notes = [], {}

    def add(name, pos, obs):
        notes[name] = len(feats)
        feats.append((pos, obs))

    centre = (0.0, 0.0, 2.0)
    add("angle_on_max", centre, [(0, 0, 2.0)])                   # angle == maxAngle: kept
    add("angle_above_max", centre, [(1, 0, 2.0)])                # the next double up: dropped
    add("tie_first", centre, [(2, 1, 2.0), (3, 2, 2.0)])         # equal angles: the first pose
    add("nan_only", centre, [(4, 0, 2.0), (7, 0, 2.0)])          # NaN entries are never chosen: dropped
    add("nan_then_valid", centre, [(4, 0, 2.0), (6, 3, 2.5), (7, 0, 2.0)])
    add("no_observations", centre, [])
    add("later_smaller", centre, [(2, 0, 2.0), (5, 4, 3.0), (6, 0, 2.0)])
    add("equal_least_later", centre, [(6, 0, 2.0), (8, 5, 2.0), (9, 6, 2.0)])    # 0.05 twice: pose 8
    def beyond(p, c, bound):                                     # the first coordinate past p whose projection leaves [0, bound]
        q = p
        while 0.0 <= ((512.0 * q) / 1.0) + c <= bound:
            q = float(np.nextafter(q, q * 2))
        return q

    for name, x in (("u_zero", -0.625), ("u_below_zero", beyond(-0.625, 320.0, 640.0)), ("u_width", 0.625),
                    ("u_above_width", beyond(0.625, 320.0, 640.0))):
        add(name, (x, 0.0, 1.0), [(5, 2, 1.0)])
    for name, y in (("v_zero", -0.46875), ("v_below_zero", beyond(-0.46875, 240.0, 480.0)), ("v_height", 0.46875),
                    ("v_above_height", beyond(0.46875, 240.0, 480.0))):
        add(name, (0.0, y, 1.0), [(5, 2, 1.0)])
    for name, z in (("z_near", 0.8), ("z_below_near", float(np.nextafter(0.8, 0.0))), ("z_far", 6.0),
                    ("z_above_far", float(np.nextafter(6.0, 7.0)))):
        add(name, (0.0, 0.0, z), [(5, 1, z)])
    add("nan_position", (np.nan, 0.0, 2.0), [(5, 2, 2.0)])
    add("behind", (0.1, 0.1, -2.0), [(5, 2, 2.0)])
    add("zero_depth", (0.1, 0.1, 0.0), [(5, 2, 2.0)])
    add("zero_det_dist", centre, [(5, 2, 0.0)])
    add("negative_det_dist", centre, [(5, 2, -1.0)])
    add("huge_det_dist", centre, [(5, 7, 1e308)])
    add("nan_det_dist", centre, [(5, 2, np.nan)])
    add("octave_table_ends", centre, [(5, -16, 30.0)])
    add("octave_table_top", centre, [(5, PS_LEVEL_OCTAVE_MAX, 1e-3)])
    for i, (o, d, k, kind) in enumerate(vref.level_edge_inputs(t)):
        add("level_%d_%s_%d" % (k, kind, i), centre, [(5, o, d)])
    pos = np.array([f[0] for f in feats], np.float64)
    start = np.zeros(len(feats) + 1, np.int32)
    start[1:] = np.cumsum([len(f[1]) for f in feats])
    obs = [o for f in feats for o in f[1]]
    rng = np.random.default_rng(1)
    store = dict(pos=pos, obs_start=start, obs_pose=np.array([o[0] for o in obs], np.int32),
                 obs_desc=rng.integers(0, 256, (len(obs), 32), dtype=np.uint8), obs_octave=np.array([o[1] for o in obs], np.int32),
                 obs_det_dist=np.array([o[2] for o in obs], np.float64), num_poses=len(ang))
    return store, ang[None, :], MAXA, notes


def test_directed_edges(ctx):
    from putslam_amd import api
    t = api.level_thresholds()
    store, ang, MAXA, notes = _edge_store(t)
    cam_inv = np.eye(4)[None]
    sd = _store_dev(store)
    F = len(store["pos"])
    for vis in (False, True):
        want = vref.build_views(store, cam_inv, ang, MAXA, vref.K_EDGE, IMG, F, require_visible=vis)
        got = _build(ctx, sd, cam_inv, ang, MAXA, F, vis=vis, K_=vref.K_EDGE).download()
        vref.compare(got, want, what=("edges", vis))
        n = int(got["viewCount"][0])
        row = {int(f): i for i, f in enumerate(got["featIdx"][0, :n])}
        start = store["obs_start"]
        at = lambda name: row.get(notes[name])   # noqa: E731
        # (what the comparison above rests on, said once more without the restatement)
        assert at("angle_on_max") is not None and at("angle_above_max") is None
        assert at("nan_only") is None and at("no_observations") is None
        assert got["obsIdx"][0, at("tie_first")] == start[notes["tie_first"]]
        assert got["obsIdx"][0, at("nan_then_valid")] == start[notes["nan_then_valid"]] + 1
        assert got["obsIdx"][0, at("later_smaller")] == start[notes["later_smaller"]] + 1
        assert got["obsIdx"][0, at("equal_least_later")] == start[notes["equal_least_later"]] + 1
        assert got["angle"][0, at("angle_on_max")] == MAXA
        for inside, outside in (("u_zero", "u_below_zero"), ("u_width", "u_above_width"), ("v_zero", "v_below_zero"),
                                ("v_height", "v_above_height"), ("z_near", "z_below_near"), ("z_far", "z_above_far")):
            assert tuple(got["uv"][0, at(inside)]) != (-1.0, -1.0), inside
            if vis:
                assert at(outside) is None, outside
            else:
                assert tuple(got["uv"][0, at(outside)]) == (-1.0, -1.0), outside
        assert tuple(got["uv"][0, at("u_zero")]) == (0.0, 240.0) and tuple(got["uv"][0, at("u_width")]) == (640.0, 240.0)
        assert tuple(got["uv"][0, at("v_zero")]) == (320.0, 0.0) and tuple(got["uv"][0, at("v_height")]) == (320.0, 480.0)
        assert np.isnan(got["uv"][0, at("nan_position")]).all() and np.isnan(got["pts"][0, at("nan_position"), 0])
        assert got["mapLevel"][0, at("nan_position")] == 0      # (NaN falls through the visibility test: emitted under both flags)
        assert (at("behind") is None) == vis and (at("zero_depth") is None) == vis
        for name in ("zero_det_dist", "negative_det_dist", "nan_det_dist"):
            assert got["mapLevel"][0, at(name)] == 0, name
        assert got["mapLevel"][0, at("huge_det_dist")] == 0     # (x overflows to +inf: the reference's int cast gives 0)
        seen = set()
        for name, f in notes.items():
            if name.startswith("level_"):
                k, kind = int(name.split("_")[1]), name.split("_")[2]
                assert got["mapLevel"][0, row[f]] == (k + 1 if kind == "on" else k), name
                seen.add((k, kind))
        assert len(seen) == 14


def test_overflow_reports_the_capacity_and_a_second_call_fits(ctx):
    rng = np.random.default_rng(8)
    store = vref.make_store(rng, 2000, 80)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 4)
    cand, cc = vref.ragged_candidates(rng, 2000, 4, 1500, counts=[1500, 40, 1400, 0])
    sd = _store_dev(store)
    want = vref.build_views(store, cam_inv, ang, 0.6, K, IMG, 300, cand, cc, fast=True)
    assert want[0]["viewCount"] < -300 and want[2]["viewCount"] < -300 and 0 < want[1]["viewCount"] <= 40 and want[3]["viewCount"] == 0
    got = _build(ctx, sd, cam_inv, ang, 0.6, 300, cand, cc).download()
    vref.compare(got, want, what="overflow")
    need = int(-min(got["viewCount"]))
    want2 = vref.build_views(store, cam_inv, ang, 0.6, K, IMG, need, cand, cc, fast=True)
    assert min(w["viewCount"] for w in want2) >= 0 and max(w["viewCount"] for w in want2) == need
    vref.compare(_build(ctx, sd, cam_inv, ang, 0.6, need, cand, cc).download(), want2, what="second call")


def test_invalid_views_leave_their_neighbours_intact(ctx):
    rng = np.random.default_rng(21)
    store = vref.make_store(rng, 1200, 40, obs_per_feature=3)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 6)
    ang[:] = np.minimum(ang, 0.2)                 # (every observation passes: the chosen one is each feature's least)
    cand, cc = vref.ragged_candidates(rng, 1000, 6, 700, counts=[700, 300, 650, 10, 0, 700])     # features 0 .. 999 only
    first = lambda f: int(store["obs_start"][f])   # noqa: E731

    def run(store_, cand_, cc_, bad_views):
        want = vref.build_views(store_, cam_inv, ang, 0.5, K, IMG, 700, cand_, cc_, fast=True)
        for v in range(6):
            assert (want[v]["viewCount"] == PS_VIEW_INVALID) == (v in bad_views), (v, want[v]["viewCount"])
        vref.compare(_build(ctx, _store_dev(store_), cam_inv, ang, 0.5, 700, cand_, cc_).download(), want, what=bad_views)

    run(store, cand, cc, ())
    # features 1100 / 1101 are in nobody's list; views 1 and 5 get one of them
    c2 = cand.copy()
    c2[1, 299], c2[5, 0] = 1100, 1101
    for val in (40, -1):                          # a pose id outside the table on ONE observation, chosen or not
        s2 = dict(store)
        s2["obs_pose"] = store["obs_pose"].copy()
        s2["obs_pose"][first(1100)] = val
        s2["obs_pose"][first(1101) + 2] = val
        run(s2, c2, cc, (1, 5))
    for val in (48, -17):                         # an octave outside the level table on the chosen observation
        s2 = dict(store)
        s2["obs_octave"] = store["obs_octave"].copy()
        s2["obs_octave"][first(1100):first(1100) + 3] = val
        s2["obs_octave"][first(1101):first(1101) + 3] = val
        run(s2, c2, cc, (1, 5))
    # ... and on an observation that is not the chosen one: nothing reads it
    rows = vref.build_views(store, cam_inv, ang, 0.5, K, IMG, 700, c2, cc, fast=True)[1]["rows"]
    chosen = int(rows["obsIdx"][list(rows["featIdx"]).index(1100)])
    s2 = dict(store)
    s2["obs_octave"] = store["obs_octave"].copy()
    s2["obs_octave"][first(1100) + (1 if chosen == first(1100) else 0)] = 99
    run(s2, c2, cc, ())
    # candidate indices outside the store, counts outside the capacity
    c3 = cand.copy()
    c3[0, 5], c3[2, 649] = -1, 1200
    run(store, c3, cc, (0, 2))
    cc3 = cc.copy()
    cc3[3], cc3[5] = -1, 701
    run(store, cand, cc3, (3, 5))
    # an observation range that is not inside the store (obs_start[1101] ends feature 1100 and begins feature 1101)
    s4 = dict(store)
    s4["obs_start"] = store["obs_start"].copy()
    s4["obs_start"][1101] = store["obs_start"][-1] + 5
    run(s4, c2, cc, (1, 5))


def test_empty_lists_no_views_and_argument_errors(ctx):
    import torch
    from putslam_amd import api
    from putslam_amd._abi import PsMapViewRequest
    from putslam_amd.device_batch import MapViewsDevice
    rng = np.random.default_rng(4)
    store = vref.make_store(rng, 500, 30)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3)
    sd = _store_dev(store)
    cand, cc = vref.ragged_candidates(rng, 500, 3, 64, counts=[0, 0, 0])
    got = _build(ctx, sd, cam_inv, ang, 0.5, 64, cand, cc).download()
    assert got["viewCount"].tolist() == [0, 0, 0] and got["nkpts"].tolist() == [0, 0, 0]
    # a store without features, and a candidate capacity of zero
    empty = vref.make_store(rng, 0, 30)
    got = _build(ctx, _store_dev(empty), cam_inv, ang, 0.5, 64).download()
    assert got["viewCount"].tolist() == [0, 0, 0]
    got = _build(ctx, sd, cam_inv, ang, 0.5, 64, np.zeros((3, 0), np.int32), np.zeros(3, np.int32)).download()
    assert got["viewCount"].tolist() == [0, 0, 0]
    # argument errors leave the outputs alone; V == 0 is fine and does nothing
    out = MapViewsDevice(3, 64, sd.device)
    out.view_count.fill_(-77)
    out.nkpts.fill_(-77)
    out.map_level.fill_(0x5A)
    d = dict(cam=torch.from_numpy(np.ascontiguousarray(cam_inv.transpose(0, 2, 1)).reshape(-1, 16)).to(sd.device),
             ang=torch.from_numpy(ang).to(sd.device))
    torch.cuda.synchronize()

    def request():
        rq = PsMapViewRequest()
        rq.camInv, rq.poseAngle = d["cam"].data_ptr(), d["ang"].data_ptr()
        rq.maxAngle, rq.fx, rq.fy, rq.cx, rq.cy, rq.imageW, rq.imageH = (0.5,) + K + IMG
        rq.V = 3
        return rq

    def expect(code, mutate):
        st, rq, os_ = sd.view(), request(), out.out_struct()
        mutate(st, rq, os_)
        with pytest.raises(api.PsError) as e:
            ctx.map_views_device(st, rq, os_)
        assert e.value.code == code and len(str(e.value)) > 25, (e.value, code)

    BAD, UNSUP = -1, -5
    expect(BAD, lambda st, rq, o: setattr(rq, "V", -1))
    expect(BAD, lambda st, rq, o: setattr(st, "numFeatures", -1))
    expect(BAD, lambda st, rq, o: setattr(st, "numObs", -1))
    expect(BAD, lambda st, rq, o: setattr(st, "numPoses", -2))
    expect(BAD, lambda st, rq, o: setattr(st, "pos", None))
    expect(BAD, lambda st, rq, o: setattr(st, "obsStart", None))
    expect(BAD, lambda st, rq, o: setattr(st, "obsDesc", None))
    expect(BAD, lambda st, rq, o: setattr(st, "obsDesc", st.obsDesc + 8))
    expect(BAD, lambda st, rq, o: setattr(rq, "camInv", None))
    expect(BAD, lambda st, rq, o: setattr(rq, "poseAngle", None))
    expect(BAD, lambda st, rq, o: setattr(rq, "cand", d["cam"].data_ptr()))            # a list without counts
    expect(BAD, lambda st, rq, o: setattr(o, "mapLevel", None))
    expect(BAD, lambda st, rq, o: setattr(o, "viewCount", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "desc", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "nkpts", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "numFrames", 2))
    expect(BAD, lambda st, rq, o: setattr(o.views, "maxKpts", 0))
    expect(UNSUP, lambda st, rq, o: setattr(o.views, "maxKpts", 16385))
    expect(BAD, lambda st, rq, o: setattr(o.views, "descFrameStride", 64 * 32 + 8))
    expect(BAD, lambda st, rq, o: setattr(o.views, "ptsFrameStride", 64 * 12 - 4))
    rq = request()
    rq.V = 0
    ctx.map_views_device(sd.view(), rq, out.out_struct())
    with pytest.raises(api.PsError):
        ctx.frame_levels_device(api.DeviceFrames(0, 0, 0, 1, 64), 0, 0, 0)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((out.view_count == -77).all()) and bool((out.nkpts == -77).all()) and bool((out.map_level == 0x5A).all())


def test_whole_store_of_a_million_features(ctx):
    """cand = NULL over 2^20 features with PS_VIEW_REQUIRE_VISIBLE: 4096 chunks a view, the rows in feature order."""
    rng = np.random.default_rng(1 << 20)
    F = 1 << 20
    store = vref.make_store(rng, F, 300, max_obs=6)
    store["pos"][:, 0] *= 10.0                     # a map 50 m x 40 m: a fraction of a per cent is in view
    store["pos"][:, 1] *= 10.0
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3)
    want = vref.build_views(store, cam_inv, ang, 0.45, K, IMG, 16384, require_visible=True, fast=True)
    assert all(1000 < w["viewCount"] <= 16384 for w in want), [w["viewCount"] for w in want]
    got = _build(ctx, _store_dev(store), cam_inv, ang, 0.45, 16384, vis=True).download()
    vref.compare(got, want, what="2^20")
    for v in range(3):
        assert (np.diff(got["featIdx"][v, :got["nkpts"][v]]) > 0).all()


# ---------------------------------------------------------------- the frame side
def test_frame_levels_equal_predicted_level(ctx):
    from putslam_amd import api
    from putslam_amd.device_batch import FrameSetDevice, PackedFrameSetDevice, frame_levels_device
    rng = np.random.default_rng(12)
    nk = [700, 0, 1, 333, 512]
    cap = 700
    pts = (rng.uniform(-1.5, 1.5, (5, cap, 3)) + [0, 0, 2.5]).astype(np.float32)
    desc = np.zeros((5, cap, 32), np.uint8)
    octave = rng.integers(0, 8, (5, cap)).astype(np.int32)
    det = np.linalg.norm(pts.astype(np.float64), axis=2) * rng.uniform(0.3, 3.5, (5, cap))
    # frame 3: the threshold straddles at (0, 0, 2), special distances, octaves at and beyond the table's ends
    edges = vref.level_edge_inputs(api.level_thresholds())
    for i, (o, d, k, kind) in enumerate(edges):
        pts[3, i], octave[3, i], det[3, i] = (0, 0, 2), o, d
    e = len(edges)
    special = [(0, np.nan), (0, np.inf), (0, -1.0), (0, 0.0), (3, 1e308), (-16, 40.0), (47, 1e-3), (-17, 1.0), (48, 1.0), (1 << 30, 1.0),
               (-(1 << 31), 1.0)]
    for i, (o, d) in enumerate(special):
        octave[3, e + i], det[3, e + i] = o, d
    pts[3, e + len(special)] = (0, 0, 0)           # curDist 0: x = +inf
    pts[3, e + len(special) + 1] = (np.nan, 1, 1)
    want = vref.frame_levels(pts, nk, octave, det)
    assert (want[3, e + 7:e + 11] == -1).all() and set(np.unique(want[0])) == set(range(8))
    for k, kind in {(x[2], x[3]) for x in edges}:
        i = next(i for i, x in enumerate(edges) if x[2] == k and x[3] == kind)
        assert want[3, i] == (k + 1 if kind == "on" else k)
    for fs in (FrameSetDevice(desc, pts, nk), PackedFrameSetDevice(desc, pts, nk, stride=cap * 44 + 64)):
        got = frame_levels_device(ctx, fs, octave, det)
        import torch
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for f, n in enumerate(nk):
            assert got[f, :n].tobytes() == want[f, :n].tobytes(), f
            assert (got[f, n:] == 0).all()          # (rows beyond the count are not written: the tensor starts as zeros)


# ---------------------------------------------------------------- the chain: views -> levels -> ps_map_pairs_device
@pytest.fixture(scope="module")
def chain(oracle):
    rng = np.random.default_rng(20261017)
    cap = 700
    store = vref.make_store(rng, 4000, 90)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 6, nan_entries=2)
    cand, cc = vref.ragged_candidates(rng, 4000, 6, 2400, counts=[1800, 1500, 0, 300, 2400, 1])
    views = vref.build_views(store, cam_inv, ang, 0.4, K, IMG, cap, cand, cc, True, fast=True)
    counts = [w["viewCount"] for w in views]
    assert 400 < counts[0] <= cap and 300 < counts[1] <= cap and counts[2] == 0 and 50 < counts[3] and counts[4] < -cap, counts
    fr = vref.frames_from_views(rng, views, [0, 1, 3, 4, 0, 2, 1, 4], [700, 650, 80, 700, 1, 64, 333, 512], cap)
    level = vref.frame_levels(fr["pos"], fr["nkpts"], fr["octave"], fr["det"])
    level[level == -9] = 0
    frames = dict(pos=fr["pos"], desc=fr["desc"], level=level, nkpts=fr["nkpts"], cap=cap)
    scene = vref.views_as_scene(views, cap)
    allp = [(v, f) for v in range(6) for f in range(8)]
    near = [(0, 0), (1, 1), (3, 2), (4, 3), (0, 4), (1, 6), (4, 7)]
    pairs = np.array((near * 4 + allp)[:64], np.int32)
    return dict(store=store, cam_inv=cam_inv, ang=ang, cand=cand, cc=cc, fr=fr, frames=frames, scene=scene, pairs=pairs, cap=cap,
                ref=mref.Ref(oracle, scene, frames), views=views)


def _chain_batch(ctx, chain, pairs, max_matches, radius=0.12, ratio=0.55, built=None):
    """Views and levels built on the device, handed to a MapBatchDevice as device tensors."""
    from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice, frame_levels_device
    if built is None:
        built = _build(ctx, _store_dev(chain["store"]), chain["cam_inv"], chain["ang"], 0.4, chain["cap"], chain["cand"],
                       chain["cc"], vis=True)
    fr = chain["fr"]
    fs = FrameSetDevice(fr["desc"], fr["pos"], fr["nkpts"])
    cur = frame_levels_device(ctx, fs, fr["octave"], fr["det"])
    return MapBatchDevice(built, built.map_level, fs, cur, pairs, max_matches, radius=radius, ratio=ratio), built


def test_chain_equals_the_reference_chain(ctx, chain):
    from putslam_amd.device_batch import run_map_pairs
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    pairs, ref, cap = chain["pairs"], chain["ref"], chain["cap"]
    want = ref.batch(prm, EST_RANSAC, 487, 99, TUM_FR1_K, pairs, 0.12, 0.55, 4 * cap)
    assert sum(w["numMatches"] > 50 for w in want) > 12 and any(w["stats"]["accepted"] for w in want)
    cfg, _ = make_config(EST_RANSAC, 487, seed=99)
    built = None
    for n in (1, 2, 7, 33, 64):
        b, built = _chain_batch(ctx, chain, pairs[:n], 4 * cap, built=built if n != 33 else None)
        run_map_pairs(ctx, prm, cfg, TUM_FR1_K, b)
        mref.compare(b.download(), want[:n], what=("chain", n))
    vref.compare(built.download(), chain["views"], what="chain views")
    # the retry ladder of ten on ONE built view: ten pairs with per-pair radius / ratio
    lad = [mref.ladder_try(0.12, 0.55, k) for k in range(1, 11)]
    lp = np.array([(1, 1)] * 10, np.int32)
    rad, rat = [x[0] for x in lad], [x[1] for x in lad]
    want = ref.batch(prm, EST_RANSAC, 487, 5, TUM_FR1_K, lp, rad, rat, 8 * cap)
    assert want[9]["numMatches"] > want[0]["numMatches"] > 50
    b, _ = _chain_batch(ctx, chain, lp, 8 * cap, radius=rad, ratio=rat, built=built)
    cfg5, _ = make_config(EST_RANSAC, 487, seed=5)
    run_map_pairs(ctx, prm, cfg5, TUM_FR1_K, b)
    mref.compare(b.download(), want, what="ladder")


def test_views_beside_a_vo_batch_on_a_second_context(ctx, chain, oracle):
    """20 repetitions of views -> map batch on one context while a second context runs VO batches: byte-identical every time."""
    import torch
    from putslam_amd import api
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_map_pairs, run_pairs
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    pairs = chain["pairs"][:28]
    want = chain["ref"].batch(prm, EST_RANSAC, 487, 31, TUM_FR1_K, pairs, 0.12, 0.55, 2800)
    seq = synth.make_sequence(9, 600, config=3, index=77)
    cfg_vo, _ = make_config(EST_RANSAC, 487, seed=1234)
    c_vo = oracle.vo_pairs(prm, cfg_vo, TUM_FR1_K, seq["desc"], seq["pts"], seq["nkpts"], seq["pairs"], threads=4)
    other = api.Context(0)
    s_map, s_vo = torch.cuda.Stream(), torch.cuda.Stream()
    fs = FrameSetDevice(seq["desc"], seq["pts"], seq["nkpts"])
    pb_other = PairBatchDevice(seq["pairs"], fs.max_kpts)
    cfg, _ = make_config(EST_RANSAC, 487, seed=31)
    sd = _store_dev(chain["store"])
    first = None
    for rep in range(20):
        with torch.cuda.stream(s_vo):
            run_pairs(other, prm, cfg_vo, TUM_FR1_K, fs, pb_other)
            run_pairs(other, prm, cfg_vo, TUM_FR1_K, fs, pb_other)
        with torch.cuda.stream(s_map):
            built = _build(ctx, sd, chain["cam_inv"], chain["ang"], 0.4, chain["cap"], chain["cand"], chain["cc"], vis=True)
            b, _ = _chain_batch(ctx, chain, pairs, 2800, built=built)
            run_map_pairs(ctx, prm, cfg, TUM_FR1_K, b)
        g, gv = b.download(), built.download()
        if first is None:
            mref.compare(g, want, what="beside VO")
            vref.compare(gv, chain["views"], what="beside VO")
            first = {k: v.tobytes() for k, v in g.items() if k in ("numMatches", "pose", "stats")}
            first_v = {k: gv[k].tobytes() for k in ("viewCount", "nkpts")}
            first_r = [[gv[k][v, :gv["nkpts"][v]].tobytes() for k in vref.ROW_KEYS] for v in range(6)]
        else:
            for k, v in first.items():
                assert g[k].tobytes() == v, (rep, k)
            for k, v in first_v.items():
                assert gv[k].tobytes() == v, (rep, k)
            for v in range(6):
                assert [gv[k][v, :gv["nkpts"][v]].tobytes() for k in vref.ROW_KEYS] == first_r[v], (rep, v)
    go = pb_other.download()
    assert go["pose"].tobytes() == c_vo["pose"].tobytes()
    other.close()


# ---------------------------------------------------------------- the time bar
def test_one_call_takes_a_tenth_of_the_host_loop(tmp_path):
    """At 64 and at 499 views of 2000 candidates with ten observations each, ONE ps_map_views_device call (call -> synchronised)
    takes at most a tenth, per view, of (a) a single-threaded C++ host loop over the same store layout
    (profiles/scripts/map_views_host_loop.cpp, -O2) plus the upload of the views it built -- both measured here, in one process,
    alternating regions, medians of five (profiles/scripts/map_views_times.py prints the full table from the same helpers).
    The bar is the project's own for a batched call.  Both sides build the same bytes (checked)."""
    from putslam_amd import api
    c = api.Context(0)
    lib = vref.build_host_loop(tmp_path)
    for V in (64, 499):
        tm = vref.ViewTiming(c, lib, vref.timing_scene(2000, V, seed=V))
        a, a0, b = tm.medians()
        kept = tm.check()
        print("2000 candidates, %d views (%d kept on average): host loop + upload %.1f us/view (loop alone %.1f), one call %.2f us/view, "
              "ratio %.1f" % (V, kept, a / V * 1e6, a0 / V * 1e6, b / V * 1e6, a / b))
        assert b * 10 <= a, (V, a, b)
    c.close()
