"""Map views with FLOAT descriptor rows built on the device from a resident store (ps_map_views_l2_device) against the restatement
of tests/map_store_f32_ref.py, byte for byte -- rows as 32-bit words, and every word of the output allocation that is no row
found as it was --, then the chain views -> ps_map_pairs_l2_device against a host-filled PsMapBatchF32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_store_f32_ref as fref  # noqa: E402
import map_view_ref as vref  # noqa: E402

from putslam_amd._abi import (EST_RANSAC, EUCLIDEAN_ERROR, PS_MAX_L2_DIM, PS_VIEW_INVALID, TUM_FR1_K,  # noqa: E402
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

K, IMG = vref.K_TUM, vref.IMAGE


def _build(ctx, sd, cam_inv, ang, max_angle, max_kpts, cand=None, cc=None, vis=False, row_floats=None, offset=0, obs_idx=True,
           fill=True):
    """(MapViewsF32Device written by the call, after its arrays were filled with sentinels)"""
    from putslam_amd.device_batch import MapViewsF32Device, build_map_views_l2
    out = MapViewsF32Device(len(cam_inv), max_kpts, sd.dim, sd.device, row_floats, offset, obs_idx)
    if fill:
        fref.fill_sentinels(out)
    return build_map_views_l2(ctx, sd, cam_inv, ang, max_angle, K, IMG, max_kpts, cand=cand, cand_counts=cc, require_visible=vis,
                              out=out)


@pytest.fixture(scope="module")
def small():
    """One store index and request for every width: 900 features, 40 poses, 3 views, ragged lists."""
    rng = np.random.default_rng(77)
    store = vref.make_store(rng, 900, 40)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3, nan_entries=2)
    cand, cc = vref.ragged_candidates(rng, 900, 3, 700, counts=[700, 333, 64])
    return dict(store=store, cam_inv=cam_inv, ang=ang, cand=cand, cc=cc, seq={})


# ---------------------------------------------------------------- widths and layouts
@pytest.mark.parametrize("dim", [1, 3, 4, 63, 64, 65, 128, PS_MAX_L2_DIM])
def test_widths_layouts_and_special_values(ctx, small, dim):
    """Dense rows, rows dim x 4 + 4 bytes apart, rows a multiple of 16 bytes apart, and a store base / an output base 4 bytes
    off 16-byte alignment (the word-wide gather); the rows hold NaN payloads, -0.0, +-inf and subnormals."""
    s = small
    rng = np.random.default_rng(dim)
    fs = fref.float_store(s["store"], fref.special_rows(rng, len(s["store"]["obs_pose"]), dim))
    want = fref.build_views(fs, s["cam_inv"], s["ang"], 0.4, K, IMG, 700, s["cand"], s["cc"], fast=True)
    assert min(w["nkpts"] for w in want) > 10 and len({w["nkpts"] for w in want}) == 3
    if dim in (3, 64):        # the sequential walk itself
        seq = fref.build_views(fs, s["cam_inv"], s["ang"], 0.4, K, IMG, 700, s["cand"], s["cc"])
        assert all(fref.same_words(a["rows"]["desc"], b["rows"]["desc"]) and vref.rows_equal(a["rows"], b["rows"])
                   for a, b in zip(seq, want))
    pad16 = (dim + 3) // 4 * 4 + 4
    layouts = [dict(), dict(store_rf=dim + 1, out_rf=dim + 1), dict(store_rf=pad16, out_rf=pad16, obs_idx=False),
               dict(store_off=1), dict(out_off=1, obs_idx=False), dict(store_off=1, out_off=1, store_rf=pad16, out_rf=pad16)]
    for lay in layouts:
        sd = fref.store_device(fs, row_floats=lay.get("store_rf"), offset_floats=lay.get("store_off", 0))
        assert (sd.obs_desc.data_ptr() % 16 == 0) == (lay.get("store_off", 0) == 0)
        out = _build(ctx, sd, s["cam_inv"], s["ang"], 0.4, 700, s["cand"], s["cc"], row_floats=lay.get("out_rf"),
                     offset=lay.get("out_off", 0), obs_idx=lay.get("obs_idx", True))
        fref.compare_views(out.download(), want, what=(dim, lay))
        fref.check_untouched(out, want, what=(dim, lay))


# ---------------------------------------------------------------- counts at the seams
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("dim,row_floats", [(64, None), (5, None), (128, 132)])
def test_view_counts_at_wave_and_work_group_seams(ctx, dim, row_floats):
    rng = np.random.default_rng(513 + dim)
    store = vref.make_store(rng, 2600, 30, max_obs=5)
    fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), dim))
    cam_inv, ang, _, _ = vref.make_request(rng, store, len(COUNTS))
    kept = fref.kept_features(fs, cam_inv, ang, 0.6, K, IMG)
    cand, cc = fref.candidates_with_counts(rng, fs, kept, COUNTS, 800)
    want = fref.build_views(fs, cam_inv, ang, 0.6, K, IMG, 520, cand, cc, fast=True)
    assert [w["viewCount"] for w in want] == COUNTS
    sd = fref.store_device(fs)
    for obs_idx in (True, False):
        out = _build(ctx, sd, cam_inv, ang, 0.6, 520, cand, cc, row_floats=row_floats, obs_idx=obs_idx)
        fref.compare_views(out.download(), want, what=(dim, obs_idx))
        fref.check_untouched(out, want, what=(dim, obs_idx))


# ---------------------------------------------------------------- whole store, visibility, overflow, invalid views
@pytest.mark.parametrize("vis", [False, True])
def test_every_feature_of_the_store_and_require_visible(ctx, vis):
    rng = np.random.default_rng(11 + vis)
    store = vref.make_store(rng, 1500, 2500 if vis else 60)      # 2500 poses: the angle table is read from HBM
    fs = fref.float_store(store, fref.special_rows(rng, len(store["obs_pose"]), 64))
    cam_inv, ang, _, _ = vref.make_request(rng, store, 4, nan_entries=5)
    want = fref.build_views(fs, cam_inv, ang, 0.5, K, IMG, 1500, require_visible=vis, fast=True)
    assert max(w["nkpts"] for w in want) > 50
    out = _build(ctx, fref.store_device(fs), cam_inv, ang, 0.5, 1500, vis=vis)
    fref.compare_views(out.download(), want, what=vis)
    fref.check_untouched(out, want, what=vis)


def test_an_overflowed_view_between_two_good_ones(ctx):
    rng = np.random.default_rng(8)
    store = vref.make_store(rng, 1600, 50)
    fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), 64))
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3)
    kept = fref.kept_features(fs, cam_inv, ang, 0.7, K, IMG)
    cand, cc = fref.candidates_with_counts(rng, fs, kept, [200, 300, 256], 600)
    want = fref.build_views(fs, cam_inv, ang, 0.7, K, IMG, 256, cand, cc, fast=True)
    assert [w["viewCount"] for w in want] == [200, -300, 256]
    sd = fref.store_device(fs)
    out = _build(ctx, sd, cam_inv, ang, 0.7, 256, cand, cc)
    fref.compare_views(out.download(), want, what="overflow")
    fref.check_untouched(out, want, what="overflow")              # no row of view 1 was written
    again = fref.build_views(fs, cam_inv, ang, 0.7, K, IMG, 300, cand, cc, fast=True)
    fref.compare_views(_build(ctx, sd, cam_inv, ang, 0.7, 300, cand, cc).download(), again, what="second call")


def test_every_cause_of_an_invalid_view(ctx):
    rng = np.random.default_rng(21)
    store = vref.make_store(rng, 1200, 40, obs_per_feature=3)
    rows = fref.special_rows(rng, len(store["obs_pose"]), 20)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 6)
    ang[:] = np.minimum(ang, 0.2)
    cand, cc = vref.ragged_candidates(rng, 1000, 6, 700, counts=[700, 300, 650, 10, 0, 700])
    first = lambda f: int(store["obs_start"][f])   # noqa: E731

    def run(store_, cand_, cc_, bad_views):
        fs = fref.float_store(store_, rows)
        want = fref.build_views(fs, cam_inv, ang, 0.5, K, IMG, 700, cand_, cc_, fast=True)
        for v in range(6):
            assert (want[v]["viewCount"] == PS_VIEW_INVALID) == (v in bad_views), (v, want[v]["viewCount"])
        out = _build(ctx, fref.store_device(fs), cam_inv, ang, 0.5, 700, cand_, cc_, obs_idx=len(bad_views) != 2)
        fref.compare_views(out.download(), want, what=bad_views)
        fref.check_untouched(out, want, what=bad_views)           # every row of an invalid view still holds the sentinel

    run(store, cand, cc, ())
    c2 = cand.copy()
    c2[1, 299], c2[5, 0] = 1100, 1101
    s2 = dict(store, obs_pose=store["obs_pose"].copy())           # a pose id outside the table
    s2["obs_pose"][first(1100)], s2["obs_pose"][first(1101) + 2] = 40, -1
    run(s2, c2, cc, (1, 5))
    s2 = dict(store, obs_octave=store["obs_octave"].copy())       # the chosen observation's octave outside the level table
    s2["obs_octave"][first(1100):first(1100) + 3] = 48
    s2["obs_octave"][first(1101):first(1101) + 3] = -17
    run(s2, c2, cc, (1, 5))
    c3 = cand.copy()                                              # candidate indices outside the store
    c3[0, 5], c3[2, 649] = -1, 1200
    run(store, c3, cc, (0, 2))
    cc3 = cc.copy()                                               # counts outside the capacity
    cc3[3], cc3[5] = -1, 701
    run(store, cand, cc3, (3, 5))
    s4 = dict(store, obs_start=store["obs_start"].copy())         # an observation range that is not inside the store
    s4["obs_start"][1101] = store["obs_start"][-1] + 5
    run(s4, c2, cc, (1, 5))


# ---------------------------------------------------------------- no views, empty stores, argument errors
def test_no_views_empty_stores_and_argument_errors(ctx):
    import torch
    from putslam_amd import api
    from putslam_amd._abi import PsMapViewRequest
    from putslam_amd.device_batch import MapViewsF32Device
    rng = np.random.default_rng(4)
    store = vref.make_store(rng, 500, 30)
    fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), 64))
    cam_inv, ang, _, _ = vref.make_request(rng, store, 3)
    sd = fref.store_device(fs)
    empty = vref.make_store(rng, 0, 30)
    efs = fref.float_store(empty, np.zeros((0, 64), np.float32))
    out = _build(ctx, fref.store_device(efs), cam_inv, ang, 0.5, 64)
    assert out.download()["viewCount"].tolist() == [0, 0, 0]
    fref.check_untouched(out, [dict(nkpts=0)] * 3, "empty store")
    out = _build(ctx, sd, cam_inv, ang, 0.5, 64, np.zeros((3, 0), np.int32), np.zeros(3, np.int32))
    assert out.download()["viewCount"].tolist() == [0, 0, 0]
    # argument errors leave the outputs alone; V == 0 is PS_OK and does nothing
    out = fref.fill_sentinels(MapViewsF32Device(3, 64, 64, sd.device))
    out.view_count.fill_(-77)
    out.nkpts.fill_(-77)
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
            ctx.map_views_l2_device(st, rq, os_)
        assert e.value.code == code and len(str(e.value)) > 25, (e.value, code)

    BAD, UNSUP = -1, -5

    def both_dims(value):
        def f(st, rq, o):
            st.dim = o.views.dim = value
        return f

    expect(BAD, lambda st, rq, o: setattr(st, "dim", 63))                              # views.dim != store.dim
    expect(BAD, lambda st, rq, o: setattr(o.views, "dim", 65))
    expect(BAD, both_dims(0))
    expect(BAD, both_dims(-4))
    expect(UNSUP, both_dims(PS_MAX_L2_DIM + 1))
    expect(BAD, lambda st, rq, o: setattr(st, "obsDescRowStride", 64 * 4 - 4))          # below a row
    expect(BAD, lambda st, rq, o: setattr(st, "obsDescRowStride", 64 * 4 + 2))          # no multiple of 4
    expect(BAD, lambda st, rq, o: setattr(st, "obsDesc", st.obsDesc + 2))               # not 4-byte aligned
    expect(BAD, lambda st, rq, o: setattr(o.views, "desc", o.views.desc + 2))
    expect(BAD, lambda st, rq, o: setattr(o.views, "descRowStride", 64 * 4 - 4))
    expect(BAD, lambda st, rq, o: setattr(o.views, "descFrameStride", 64 * 64 * 4 - 4))
    expect(BAD, lambda st, rq, o: setattr(o.views, "ptsFrameStride", 64 * 12 - 4))
    expect(BAD, lambda st, rq, o: setattr(rq, "V", -1))
    expect(BAD, lambda st, rq, o: setattr(st, "numObs", -1))
    expect(BAD, lambda st, rq, o: setattr(st, "pos", None))
    expect(BAD, lambda st, rq, o: setattr(st, "obsStart", None))
    expect(BAD, lambda st, rq, o: setattr(st, "obsDesc", None))
    expect(BAD, lambda st, rq, o: setattr(rq, "camInv", None))
    expect(BAD, lambda st, rq, o: setattr(rq, "cand", d["cam"].data_ptr()))             # a list without counts
    expect(BAD, lambda st, rq, o: setattr(o, "mapLevel", None))
    expect(BAD, lambda st, rq, o: setattr(o, "viewCount", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "pts", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "nkpts", None))
    expect(BAD, lambda st, rq, o: setattr(o.views, "numFrames", 2))
    expect(BAD, lambda st, rq, o: setattr(o.views, "maxKpts", 0))
    expect(UNSUP, lambda st, rq, o: setattr(o.views, "maxKpts", 16385))
    rq = request()
    rq.V = 0
    ctx.map_views_l2_device(sd.view(), rq, out.out_struct())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((out.view_count == -77).all()) and bool((out.nkpts == -77).all())
    fref.check_untouched(out, [dict(nkpts=0)] * 3, "errors")
    # the capacity of PS_MAX_L2_DIM and a stride that is large but legal are taken
    ok = _build(ctx, sd, cam_inv, ang, 0.5, 500, row_floats=64 + 1024)
    fref.compare_views(ok.download(), fref.build_views(fs, cam_inv, ang, 0.5, K, IMG, 500, fast=True), what="wide pitch")


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("dim", [64, 20])
def test_views_feed_map_pairs_l2_like_a_host_filled_batch(ctx, dim):
    """ps_map_views_l2_device -> ps_map_pairs_l2_device gives the bytes of a PsMapBatchF32 whose `maps` the host filled from the
    restatement's views."""
    from putslam_amd.device_batch import FrameSetF32Device, MapBatchF32Device, run_map_pairs_l2
    rng = np.random.default_rng(31 + dim)
    store = vref.make_store(rng, 1400, 50)
    fs = fref.float_store(store, fref.unit_rows(rng, len(store["obs_pose"]), dim))
    cam_inv, ang, _, _ = vref.make_request(rng, store, 4)
    cap = 700
    want = fref.build_views(fs, cam_inv, ang, 0.5, K, IMG, cap, require_visible=True, fast=True)
    assert min(w["nkpts"] for w in want) > 40
    scene = fref.views_as_scene(want, cap, dim)
    # frames near the views: a third of every view's rows, moved by a centimetre, their descriptors a little noisy
    nk = np.array([w["nkpts"] // 3 for w in want], np.int32)
    fdesc, fpts, flev = np.zeros((4, cap, dim), np.float32), np.zeros((4, cap, 3), np.float32), np.zeros((4, cap), np.int32)
    for f, w in enumerate(want):
        src = rng.choice(w["nkpts"], nk[f], replace=False)
        fdesc[f, :nk[f]] = w["rows"]["desc"][src] + rng.normal(0, 0.01, (nk[f], dim)).astype(np.float32)
        fpts[f, :nk[f]] = w["rows"]["pts"][src] + rng.normal(0, 0.01, (nk[f], 3)).astype(np.float32)
        flev[f, :nk[f]] = w["rows"]["mapLevel"][src] + rng.integers(-1, 2, nk[f])
    pairs = np.array([[0, 0], [1, 1], [2, 2], [3, 3], [0, 1], [3, 7]], np.int32)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=99)
    views = _build(ctx, fref.store_device(fs), cam_inv, ang, 0.5, cap, vis=True, fill=False)
    fref.compare_views(views.download(), want, what="chain")
    results = []
    for maps, level in ((views, views.map_level), (FrameSetF32Device(scene["desc"], scene["pos"], scene["nkpts"]), scene["level"])):
        frames = FrameSetF32Device(fdesc, fpts, nk)
        batch = MapBatchF32Device(maps, level, frames, flev, pairs, cap)
        run_map_pairs_l2(ctx, prm, cfg, TUM_FR1_K, batch)
        g = batch.download()
        n = np.maximum(g["numMatches"], 0)
        results.append(dict(numMatches=g["numMatches"].tobytes(), pose=g["pose"].tobytes(), stats=g["stats"].tobytes(),
                            rows=[g["matches"][p, :n[p]].tobytes() + g["inlierMask"][p, :n[p]].tobytes() for p in range(len(pairs))]))
        assert n[:4].min() > 10 and int(g["stats"]["accepted"][:4].sum()) >= 3
    assert results[0] == results[1]
