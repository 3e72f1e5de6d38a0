"""ORB key point detection on the GPU (ps_orb_detect.h): ps_orb_detect_frames, the host form ps_detect_features_orb, the per-level
planes and survivor lists of ps_debug_orb_detect_level and the Python wrappers equal the restatement (tests/orb_detect_ref.py) byte
for byte -- floats compared as uint32 words, counts, and sentinel-filled outputs checked beyond every count.  The premises of these
runs (both cuts bite at every live level, ties at the cuts) are asserted on the restatement in tests/test_orb_detect_ref_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orb_detect_ref as D  # noqa: E402
from image_frontend_util import as_hwc, u32, upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def prm(p):
    from putslam_amd._abi import orb_detect_params
    return orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"],
                             p["max_features"])


def sentinels(frames, cap):
    import torch
    f = lambda *shape: torch.from_numpy(np.full(shape, SENT_F, np.uint32).view(np.float32)).to("cuda:0")   # noqa: E731
    i = lambda *shape: torch.from_numpy(np.full(shape, SENT_I, np.int32)).to("cuda:0")   # noqa: E731
    return f(frames, cap, 2), f(frames, cap), f(frames, cap), i(frames, cap), i(frames)


def run_device(ctx, imgs, p, cap=None, padded=False, det=None):
    """detect_features_orb_batch over sentinel-filled blocks -> [xy, response, angle, octave, counts] as numpy, whole blocks."""
    import torch
    from putslam_amd import device_batch
    rows, cols, cn = as_hwc(imgs[0]).shape
    own = det is None
    det = device_batch.OrbDetector(ctx, rows, cols, cn, len(imgs), prm(p)) if own else det
    cap = max(1, p["max_features"]) if cap is None else cap
    blocks = sentinels(len(imgs), cap)
    device_batch.detect_features_orb_batch(ctx, det, upload_images(imgs, padded), prm(p), cap, *blocks)
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in blocks]
    if own:
        det.close()
    return out


def assert_frame(got, f, want, what=""):
    """Frame f of the device blocks holds the restatement's key points, and the sentinels beyond them."""
    xy, resp, ang, octv, cnt = got
    wxy, wr, wa, wo = want[:4]
    n = len(wr)
    assert int(cnt[f]) == n, (what, f, int(cnt[f]), n)
    assert u32(xy[f, :n]).tolist() == u32(wxy).reshape(-1, 2).tolist(), (what, f, xy[f, :n][:6].tolist(), wxy[:6].tolist())
    assert u32(resp[f, :n]).tolist() == u32(wr).tolist(), (what, f, resp[f, :n][:8].tolist(), wr[:8].tolist())
    assert u32(ang[f, :n]).tolist() == u32(wa).tolist(), (what, f, ang[f, :n][:8].tolist(), wa[:8].tolist())
    assert octv[f, :n].tolist() == wo.tolist(), (what, f)
    assert (u32(xy[f, n:]) == SENT_F).all() and (u32(resp[f, n:]) == SENT_F).all() and (u32(ang[f, n:]) == SENT_F).all(), (what, f)
    assert (octv[f, n:] == SENT_I).all(), (what, f)


def assert_levels(det, f, rois, what=""):
    """The raw level, the FAST score plane and the survivor lists after each cut, of every ROI and level of frame f."""
    for q, levels in enumerate(rois):
        for l, lv in enumerate(levels):
            got = det.level(f, q, l)
            assert np.array_equal(got["raw"], lv["raw"]), (what, "raw", q, l, np.argwhere(got["raw"] != lv["raw"])[:4].tolist())
            assert np.array_equal(got["score"], lv["score"]), (what, "score", q, l, np.argwhere(got["score"] != lv["score"])[:4].tolist())
            assert got["yx"].tolist() == ((lv["y"].astype(np.int64) << 16) | lv["x"]).tolist(), (what, "first cut", q, l)
            assert u32(got["response"]).tolist() == u32(lv["response"]).tolist(), (what, "harris", q, l)
            assert u32(got["angle"]).tolist() == u32(lv["angle"]).tolist(), (what, "angle", q, l)
            assert got["kept"].tolist() == lv["kept"].astype(np.uint8).tolist(), (what, "second cut", q, l)


CASE_IDS = ["%s-%dx%d-%d-%s" % (c[:4] + ("-".join(str(v) for v in c[4].values()),)) for c in D.ALL_CASES]


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("case", D.ALL_CASES, ids=CASE_IDS)
def test_cases_equal_restatement(ctx, case, padded):
    """Every scene, shape, channel count, parameter set and grid of the list, dense and in a block padded with 0xEE: the outputs and,
    through the debug call, the planes and both survivor lists of every level of every ROI."""
    from putslam_amd import device_batch
    name, rows, cols, cn, p = case
    img = D.image(name, rows, cols, cn)
    want = D.detect_closed(img, p, want_levels=True)
    det = device_batch.OrbDetector(ctx, rows, cols, cn, 1, prm(p))
    got = run_device(ctx, [img], p, padded=padded, det=det)
    assert_levels(det, 0, want[4], case[:4])
    assert_frame(got, 0, want, case[:4])
    det.close()


def test_colour_order_matters(ctx):
    """CV_RGB2GRAY weighs channel 0 with 4899: the same scene with its channels reversed gives other key points, on the device as in
    the restatement (the descriptor's BGR2GRAY would swap the two)."""
    name, rows, cols, cn, p = D.PREMISE_CASES[1]
    img = D.image(name, rows, cols, 3)
    rev = np.ascontiguousarray(img[..., ::-1])
    a, b = D.detect_closed(img, p), D.detect_closed(rev, p)
    assert a[0].tobytes() != b[0].tobytes()
    got = run_device(ctx, [img, rev], p)
    assert_frame(got, 0, a)
    assert_frame(got, 1, b)


def test_max_features_cuts_through_the_tied_block(ctx):
    """The tiled scene: eight exact Harris ties lead the list; maximalTrackedFeatures 0 .. 10 cuts at every position through them."""
    from putslam_amd import device_batch
    name, rows, cols, cn, p = D.TILED_CASE
    img = D.image(name, rows, cols, cn)
    det = device_batch.OrbDetector(ctx, rows, cols, cn, 1, prm(p))
    for mx in range(0, 11):
        q = dict(p, max_features=mx)
        want = D.detect_closed(img, q)
        assert len(want[1]) == mx
        assert_frame(run_device(ctx, [img], q, det=det), 0, want, mx)
    det.close()


def test_per_roi_cut_inside_ties(ctx):
    """Grid 2 x 2 on a 300 x 400 tiling of the patch: every ROI is the 150 x 200 tiled scene, so the per-ROI cut at 3 max / 4 and the
    join, which ties across ROIs, both fall inside blocks of equal responses."""
    img = D.tiled(300, 400)
    for mx in (2, 4, 7, 10, 40):
        p = D.params(12, 1.2, 3, 20, 2, 2, mx)
        want = D.detect_closed(img, p)
        assert len(want[1]) == mx
        assert_frame(run_device(ctx, [img], p), 0, want, mx)


def test_ragged_batch_equals_single_calls_and_the_host_form(ctx):
    """Five different frames in one call = five calls of one frame = ps_detect_features_orb on a region of a parent image."""
    rows, cols = 96, 128
    imgs = [D.image("texture", rows, cols), np.full((rows, cols), 7, np.uint8), D.image("noise256", rows, cols), D.image("noise4", rows, cols),
            D.image("tiled", rows, cols)]
    for p in (D.params(40, 1.2, 3, 20, 1, 1, 30), D.params(24, 1.2, 3, 20, 1, 2, 500)):
        batch = run_device(ctx, imgs, p, padded=True, cap=40)
        counts = batch[4].tolist()
        assert counts[1] == 0 and len(set(counts)) >= 3, counts
        for f, img in enumerate(imgs):
            want = D.detect_closed(img, p)
            assert_frame(batch, f, want, f)
            assert_frame(run_device(ctx, [img], p, cap=40), 0, want, f)
            parent = np.full((rows + 4, cols + 9), 0x33, np.uint8)
            parent[2:2 + rows, 5:5 + cols] = img
            got = ctx.detect_features_orb(parent[2:2 + rows, 5:5 + cols], prm(p))
            assert [u32(g).tolist() for g in got[:3]] == [u32(w).tolist() for w in want[:3]] and got[3].tolist() == want[3].tolist(), f


def test_host_form_reports_the_capacity_it_needs(ctx):
    img = D.image("texture", 96, 128)
    p = D.params(40, 1.2, 3)
    want = D.detect_closed(img, p)
    n = len(want[1])
    assert n > 4
    L = ctx._L
    xy, resp, ang = np.full((n, 2), SENT_F, np.uint32), np.full(n, SENT_F, np.uint32), np.full(n, SENT_F, np.uint32)
    octv = np.full(n, SENT_I, np.int32)
    nout = C.c_int(-7)
    pp = prm(p)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    args = (ctx._h, pv(img), 96, 128, 1, 0, C.byref(pp), pv(xy), pv(resp), pv(ang), pv(octv))
    assert L.ps_detect_features_orb(*args, n - 1, C.byref(nout)) == -1 and nout.value == n
    assert (xy == SENT_F).all() and (resp == SENT_F).all() and (ang == SENT_F).all() and (octv == SENT_I).all()
    assert b"cap" in L.ps_last_error(ctx._h)
    assert L.ps_detect_features_orb(*args, n, C.byref(nout)) == 0 and nout.value == n
    assert xy.tolist() == u32(want[0]).tolist() and resp.tolist() == u32(want[1]).tolist() and ang.tolist() == u32(want[2]).tolist()
    assert octv.tolist() == want[3].tolist()


def test_errors_leave_the_outputs_untouched(ctx):
    """Every error of the C ABI's list, with its code, a text through ps_last_error and the outputs as they were."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import PS_MAX_KPTS, PsImageSet
    L, h = ctx._L, ctx._h
    rows, cols = 96, 128
    base = D.params(12, 1.2, 3, 20, 1, 1, 40)
    det = device_batch.OrbDetector(ctx, rows, cols, 1, 2, prm(base))
    imgs = upload_images([D.image("texture", rows, cols)] * 2, False)
    cap = 40
    xy, resp, ang, octv, cnt = sentinels(2, cap)

    def image_set(frames=2, r=rows, c=cols, cn=1, row_stride=0, frame_stride=0, pixels=True):
        return PsImageSet(imgs.data_ptr() if pixels else None, row_stride, frame_stride, frames, r, c, cn)

    def call(s, p, capacity=cap, x=xy, r=resp, a=ang, o=octv, n=cnt, d=det.handle):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        return L.ps_orb_detect_frames(h, d, C.byref(s) if s is not None else None, C.byref(p) if p is not None else None, capacity, ptr(x),
                                      ptr(r), ptr(a), ptr(o), ptr(n))

    good = prm(base)

    def with_field(name, value):
        p = prm(base)
        setattr(p, name, value)
        return p

    bad_arg = [
        ("null detector", lambda: call(image_set(), good, d=None)),
        ("null images", lambda: call(None, good)),
        ("null params", lambda: call(image_set(), None)),
        ("null pixels", lambda: call(image_set(pixels=False), good)),
        ("null xy", lambda: call(image_set(), good, x=None)),
        ("null response", lambda: call(image_set(), good, r=None)),
        ("null angle", lambda: call(image_set(), good, a=None)),
        ("null octave", lambda: call(image_set(), good, o=None)),
        ("null counts", lambda: call(image_set(), good, n=None)),
        ("gridRows 0", lambda: call(image_set(), with_field("gridRows", 0))),
        ("gridCols -1", lambda: call(image_set(), with_field("gridCols", -1))),
        ("another grid", lambda: call(image_set(), with_field("gridCols", 2))),
        ("another level count", lambda: call(image_set(), with_field("nLevels", 4))),
        ("another scale factor", lambda: call(image_set(), with_field("scaleFactor", 1.5))),
        ("scale factor 1", lambda: call(image_set(), with_field("scaleFactor", 1.0))),
        ("nLevels 9", lambda: call(image_set(), with_field("nLevels", 9))),
        ("negative nFeatures", lambda: call(image_set(), with_field("nFeatures", -1))),
        ("negative maximum", lambda: call(image_set(), with_field("maximalTrackedFeatures", -1))),
        ("reserved", lambda: call(image_set(), with_field("reserved", 1))),
        ("other rows", lambda: call(image_set(r=rows - 1), good)),
        ("other cols", lambda: call(image_set(c=cols + 1), good)),
        ("other channels", lambda: call(image_set(cn=3), good)),
        ("row stride below a row", lambda: call(image_set(row_stride=cols - 1), good)),
        ("frame stride below a frame", lambda: call(image_set(frame_stride=rows * cols - 1), good)),
        ("more frames than the detector holds", lambda: call(image_set(frames=3), good)),
        ("negative frames", lambda: call(image_set(frames=-1), good)),
        ("capacity below the maximum", lambda: call(image_set(), good, capacity=cap - 1)),
        ("negative capacity", lambda: call(image_set(), with_field("maximalTrackedFeatures", 0), capacity=-1)),
    ]
    for what, run in bad_arg:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    unsupported = [
        ("maximum above PS_MAX_KPTS", lambda: call(image_set(), with_field("maximalTrackedFeatures", PS_MAX_KPTS + 1), capacity=PS_MAX_KPTS)),
        ("nFeatures above PS_MAX_KPTS", lambda: call(image_set(), with_field("nFeatures", PS_MAX_KPTS + 1))),
        ("capacity above PS_MAX_KPTS", lambda: call(image_set(), good, capacity=PS_MAX_KPTS + 1)),
    ]
    for what, run in unsupported:
        assert run() == -5, what
        assert len(L.ps_last_error(h)) > 0, what
    for shape, code in [((8193, 128, 1, 1), -5), ((96, 8193, 1, 1), -5), ((0, 128, 1, 1), -1), ((96, 0, 1, 1), -1), ((96, 128, 2, 1), -1),
                        ((96, 128, 1, 0), -1), ((96, 128, 1, 65536), -1)]:
        out = C.c_void_p(0x55)
        assert L.ps_orb_detector_create(h, *shape[:3], C.byref(good), shape[3], C.byref(out)) == code and not out.value, shape
    out = C.c_void_p(0x55)
    assert L.ps_orb_detector_create(h, 4, 128, 1, C.byref(with_field("gridRows", 5)), 1, C.byref(out)) == -1 and not out.value   # an empty ROI
    out = C.c_void_p(0x55)
    assert L.ps_orb_detector_create(h, 96, 128, 1, None, 1, C.byref(out)) == -1 and not out.value
    assert L.ps_orb_detector_create(h, 96, 128, 1, C.byref(good), 1, None) == -1
    # the host form: its own list
    img = D.image("texture", rows, cols)
    hx, hr, ha = np.full((cap, 2), SENT_F, np.uint32), np.full(cap, SENT_F, np.uint32), np.full(cap, SENT_F, np.uint32)
    ho, nout = np.full(cap, SENT_I, np.int32), C.c_int(-7)
    pv = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def host(image=img, r=rows, c=cols, cn=1, stride=0, p=good, x=hx, rr=hr, a=ha, o=ho, capacity=cap, n=nout):
        return L.ps_detect_features_orb(h, pv(image), r, c, cn, stride, C.byref(p) if p is not None else None, pv(x), pv(rr), pv(a), pv(o),
                                        capacity, C.byref(n) if n is not None else None)
    for what, run, code in [("null image", lambda: host(image=None), -1), ("null params", lambda: host(p=None), -1),
                            ("null xy", lambda: host(x=None), -1), ("null response", lambda: host(rr=None), -1),
                            ("null angle", lambda: host(a=None), -1), ("null octave", lambda: host(o=None), -1),
                            ("null nout", lambda: host(n=None), -1), ("stride", lambda: host(stride=cols - 1), -1),
                            ("channels", lambda: host(cn=2), -1), ("rows 0", lambda: host(r=0), -1),
                            ("negative cap", lambda: host(capacity=-1), -1), ("reserved", lambda: host(p=with_field("reserved", 2)), -1),
                            ("gridRows", lambda: host(p=with_field("gridRows", 0)), -1),
                            ("rows above 8192", lambda: host(r=8193), -5),
                            ("maximum above PS_MAX_KPTS", lambda: host(p=with_field("maximalTrackedFeatures", PS_MAX_KPTS + 1)), -5)]:
        assert run() == code, what
        assert len(L.ps_last_error(h)) > 0 and nout.value == -7, what
    assert (hx == SENT_F).all() and (hr == SENT_F).all() and (ha == SENT_F).all() and (ho == SENT_I).all()
    assert L.ps_debug_orb_detect_level(h, None, 0, 0, None, None, None, None, None, None, None, 0) == -1
    for slot, level in [(2, 0), (-1, 0), (0, 3), (0, -1)]:
        assert L.ps_debug_orb_detect_level(h, det.handle, slot, level, None, None, None, None, None, None, None, 0) == -1
    # nothing above wrote anything; zero frames is PS_OK and writes nothing either
    assert call(image_set(frames=0), good) == 0
    torch.cuda.synchronize()
    for t in (xy, resp, ang):
        assert (u32(t.cpu().numpy()) == SENT_F).all()
    assert (octv.cpu().numpy() == SENT_I).all() and (cnt.cpu().numpy() == SENT_I).all()
    # ... and the same arguments, all in order, work
    assert call(image_set(), good) == 0
    torch.cuda.synchronize()
    n = len(D.detect_closed(D.image("texture", rows, cols), base)[1])
    assert cnt.cpu().numpy().tolist() == [n, n]
    det.close()


def test_detected_arrays_drop_into_dbscan_and_description(ctx):
    """The shipped match() chain without a host step: the arrays ps_orb_detect_frames wrote go unchanged into ps_dbscan_thin_device
    (with octave) and ps_describe_features_device; kept indices and rows equal the restatements on the restatement's key points."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import orb_params
    import dbscan_ref_py as R
    import orb_ref as O
    rows, cols = 150, 200
    imgs = [D.image("texture", rows, cols, 3), D.image("noise4", rows, cols, 3), np.full((rows, cols, 3), 50, np.uint8)]
    p = D.params(60, 1.2, 8, 20, 1, 1, 60)
    det = device_batch.OrbDetector(ctx, rows, cols, 3, len(imgs), prm(p))
    dev = upload_images(imgs, False)
    xy, resp, ang, octv, cnt = device_batch.detect_features_orb_batch(ctx, det, dev, prm(p))
    kept, nkept = device_batch.dbscan_thin_device(ctx, xy, cnt, octv, 12.0, 2, 1)
    pyr = device_batch.OrbPyramids(ctx, rows, cols, 3, len(imgs), orb_params(1.2, 8))
    pyr.build(dev)
    slots = torch.arange(len(imgs), dtype=torch.int32, device=dev.device)
    desc, kidx, nk = device_batch.describe_features_batch(ctx, pyr, slots, xy, ang, octv, cnt)
    torch.cuda.synchronize()
    kept, nkept, desc, kidx, nk = (t.cpu().numpy() for t in (kept, nkept, desc, kidx, nk))
    thinned = described = 0
    for f, img in enumerate(imgs):
        wxy, _, wang, woct = D.detect_closed(img, p)
        want = R.dbscan_keep(wxy, woct, 12.0, 2, 1)
        assert int(nkept[f]) == len(want) and kept[f, :len(want)].tolist() == want.tolist(), f
        thinned += len(wxy) - len(want)
        wdesc, wkept = O.describe(O.pyramid(img, 1.2, 8), wxy, wang, woct)
        assert int(nk[f]) == len(wkept) and kidx[f, :len(wkept)].tolist() == wkept.tolist(), f
        assert np.array_equal(desc[f, :len(wkept)], wdesc), f
        described += len(wkept)
    assert thinned > 0 and described > 20      # both steps had something to do
    det.close()
    pyr.close()
