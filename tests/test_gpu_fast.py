"""FAST-9/16 key point detection on the GPU (ps_fast.h): the grey / score / corner maps, ps_detect_features_device, the host form
ps_detect_features and the Python wrappers equal the restatements (tests/fast_ref.py) byte for byte -- xy and response compared as
uint32 words, counts, and sentinel-filled outputs checked beyond every count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fast_ref as F  # noqa: E402
from image_frontend_util import as_hwc, u32, upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def prm(threshold=10, nms=True, grid_rows=1, grid_cols=1, max_features=500):
    from putslam_amd._abi import detect_params
    return detect_params(threshold, nms, grid_rows, grid_cols, max_features)


def sentinels(frames, cap):
    import torch
    xy = torch.from_numpy(np.full((frames, cap, 2), SENT_F, np.uint32).view(np.float32)).to("cuda:0")
    resp = torch.from_numpy(np.full((frames, cap), SENT_F, np.uint32).view(np.float32)).to("cuda:0")
    cnt = torch.from_numpy(np.full((frames,), SENT_I, np.int32)).to("cuda:0")
    return xy, resp, cnt


def run_device(ctx, imgs, p, cap=None, padded=False, det=None, want_maps=False):
    """detect_features_batch over sentinel-filled blocks -> (xy, response, counts) as numpy, whole blocks [, the maps per frame]."""
    import torch
    from putslam_amd import device_batch
    rows, cols, cn = as_hwc(imgs[0]).shape
    own = det is None
    det = device_batch.FastDetector(ctx, rows, cols, cn, len(imgs)) if own else det
    cap = max(1, p.maximalTrackedFeatures) if cap is None else cap
    xy, resp, cnt = sentinels(len(imgs), cap)
    device_batch.detect_features_batch(ctx, det, upload_images(imgs, padded), p, cap, xy, resp, cnt)
    torch.cuda.synchronize()
    out = [xy.cpu().numpy(), resp.cpu().numpy(), cnt.cpu().numpy()]
    if want_maps:
        out.append([det.maps(f) for f in range(len(imgs))])
    if own:
        det.close()
    return out


def assert_frame(got, f, want, what=""):
    """Frame f of the device blocks holds the restatement's key points, and the sentinels beyond them."""
    xy, resp, cnt = got[:3]
    wxy, wr = want
    n = len(wr)
    assert int(cnt[f]) == n, (what, f, int(cnt[f]), n)
    assert u32(xy[f, :n]).tolist() == u32(wxy).reshape(-1, 2).tolist(), (what, f, xy[f, :n][:6].tolist(), wxy[:6].tolist())
    assert u32(resp[f, :n]).tolist() == u32(wr).tolist(), (what, f, resp[f, :n][:8].tolist(), wr[:8].tolist())
    assert (u32(xy[f, n:]) == SENT_F).all() and (u32(resp[f, n:]) == SENT_F).all(), (what, f)


def ref(img, p, literal=False):
    fn = F.detect_literal if literal else F.detect_closed
    return fn(img, p.threshold, bool(p.nonmaxSuppression), p.gridRows, p.gridCols, p.maximalTrackedFeatures)


def scenes(rows, cols, cn):
    imgs = [mk(rows, cols) for mk in F.SCENES.values()]
    return imgs if cn == 1 else [F.colour(g, 17 + i) for i, g in enumerate(imgs)]


# threshold (two of them outside 0 .. 255), gridRows, gridCols: every grid of the list tests below, and one that divides nothing evenly
MAP_RUNS = [(0, 1, 1), (10, 2, 3), (40, 4, 4), (255, 6, 4), (-5, 1, 1), (300, 2, 3), (10, 5, 7)]


@pytest.mark.parametrize("rows,cols", [(48, 64), (37, 53), (96, 128)])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("padded", [False, True])
def test_maps_equal_restatement(ctx, rows, cols, cn, padded):
    """Grey, score and corner planes of three scenes through ps_debug_fast_maps: more than one tile a side, sizes that are no
    multiple of the tile, ROIs whose origins and remainder strips fall inside tiles."""
    from putslam_amd import device_batch
    imgs = scenes(rows, cols, cn)
    det = device_batch.FastDetector(ctx, rows, cols, cn, len(imgs))
    for t, gr, gc in MAP_RUNS:
        p = prm(t, True, gr, gc, 50)
        got = run_device(ctx, imgs, p, padded=padded, det=det, want_maps=True)
        for f, img in enumerate(imgs):
            wg, ws, wc = F.maps_closed(img, t, gr, gc)
            g, s, c = got[3][f]
            assert np.array_equal(g, wg), ("grey", t, gr, gc, f)
            assert np.array_equal(c, wc), ("corner", t, gr, gc, f, np.argwhere(c != wc)[:5].tolist())
            assert np.array_equal(s, ws), ("score", t, gr, gc, f, np.argwhere(s != ws)[:5].tolist())
            assert_frame(got, f, ref(img, p), (t, gr, gc))
    det.close()


@pytest.mark.parametrize("nms", [True, False])
@pytest.mark.parametrize("gr,gc", [(1, 1), (2, 3), (4, 4), (6, 4)])
def test_lists_equal_restatement(ctx, nms, gr, gc):
    """The emitted lists at 96 x 128: suppression on and off (off: every corner, response 0, raster order -- 1182 / 3494 / 1850
    corners in the three scenes, so the ordered placement runs over several chunks and the cut falls inside the one tie), the
    grids 1 x 1, 3 x 2, 4 x 4 and 4 x 6 (columns x rows), maximalTrackedFeatures 0, 1, 20 and 500."""
    from putslam_amd import device_batch
    imgs = scenes(96, 128, 1)
    det = device_batch.FastDetector(ctx, 96, 128, 1, len(imgs))
    for mx in (0, 1, 20, 500):
        p = prm(10, nms, gr, gc, mx)
        got = run_device(ctx, imgs, p, det=det)
        for f, img in enumerate(imgs):
            want = ref(img, p)
            if not nms:
                assert (want[1] == 0).all()
            assert_frame(got, f, want, (nms, gr, gc, mx))
    det.close()


def test_literal_restatement_on_the_device_lists(ctx):
    """The sequential restatement (a), grid loop and stable sorts included, against the device on one colour scene per grid."""
    img = F.colour(F.SCENES["blocks"](96, 128), 3)
    for gr, gc, mx, nms in [(1, 1, 500, True), (2, 3, 60, True), (4, 4, 500, False)]:
        p = prm(10, nms, gr, gc, mx)
        assert_frame(run_device(ctx, [img], p), 0, ref(img, p, literal=True), (gr, gc, mx, nms))


def tie_scene():
    """The four-level scene at 48 x 64, seed 5, t = 10: 111 key points, 24 of response 119, then 87 of response 59."""
    img = F.noise4(48, 64, 5)
    xy, r = F.detect_closed(img, 10, True, 1, 1, 500)
    lxy, lr = F.detect_literal(img, 10, True, 1, 1, 500)
    assert xy.tobytes() == lxy.tobytes() and r.tobytes() == lr.tobytes()
    assert len(r) == 111 and r.tolist() == [119.0] * 24 + [59.0] * 87
    return img, r


def test_cut_inside_a_tie_in_the_merge(ctx):
    """Grid 1 x 1: the ROI keeps 3 x max, the merge cuts at max.  Every max from 1 to 110 but 24 cuts between two equal responses;
    who survives is decided by raster order."""
    from putslam_amd import device_batch
    img, r = tie_scene()
    caps = [c for c in range(1, 111) if r[c - 1] == r[c]]
    assert caps == [c for c in range(1, 111) if c != 24]       # the premise: every one of these cuts inside a tie
    det = device_batch.FastDetector(ctx, 48, 64, 1, 1)
    for mx in caps + [24, 111, 112]:
        p = prm(10, True, 1, 1, mx)
        assert_frame(run_device(ctx, [img], p, det=det), 0, ref(img, p), mx)
    det.close()


def test_cut_inside_a_tie_per_roi(ctx):
    """Grid 2 x 2 on the four-level scene (21 / 25 / 23 / 21 key points an ROI, 5 / 5 / 6 / 1 of them of response 119, the rest of 59):
    for the maxima below the per-ROI cut at 3 x max / 4 falls between two equal responses in every ROI; the join then cuts the
    ROIs' lists, which tie across ROIs, to the maximum."""
    from putslam_amd import device_batch
    img, _ = tie_scene()
    gray = F.to_gray(img)
    per = []
    for x0, y0, w, h in F.roi_rects(48, 64, 2, 2):
        c, s = F.fast_closed(gray[y0:y0 + h, x0:x0 + w], 10)
        mask, resp = F.emitted_closed(c, s, True)
        per.append(np.sort(resp[mask].astype(np.int64))[::-1])
    maxima = [3, 4, 6, 12, 20, 27]
    for mx in maxima:   # the premise, on the restatement: the per-ROI cut separates equal responses in every ROI
        k = F.max_in_roi(mx, 2, 2)
        assert all(len(v) > k and v[k - 1] == v[k] for v in per), (mx, [len(v) for v in per])
    det = device_batch.FastDetector(ctx, 48, 64, 1, 1)
    for mx in maxima:
        p = prm(10, True, 2, 2, mx)
        want = ref(img, p)
        assert len(want[1]) == mx and ref(img, p, literal=True)[0].tobytes() == want[0].tobytes()
        assert_frame(run_device(ctx, [img], p, det=det), 0, want, mx)
    det.close()


def test_shape_edges(ctx):
    """A 7 x 7 image has one candidate; an image without a corner gives a count of 0 and writes nothing else; an ROI smaller than
    7 x 7 gives nothing (grid 6 x 4 on 53 x 37: ROIs of 13 x 6)."""
    one = np.zeros((7, 7), np.uint8)
    one[3, 3] = 255
    got = run_device(ctx, [one], prm(10, True, 1, 1, 5), want_maps=True)
    assert_frame(got, 0, (np.array([[3, 3]], np.float32), np.array([254], np.float32)))
    assert got[3][0][1][3, 3] == 254 and got[3][0][1].sum() == 254 and got[3][0][2].sum() == 1
    flat = np.full((40, 50), 90, np.uint8)
    got = run_device(ctx, [flat], prm(10, True, 1, 1, 5))
    assert_frame(got, 0, (np.zeros((0, 2), np.float32), np.zeros(0, np.float32)))
    img = F.SCENES["noise256"](37, 53)
    p = prm(10, True, 6, 4, 50)
    assert len(ref(img, p)[1]) == 0
    got = run_device(ctx, [img], p, cap=1, want_maps=True)
    assert_frame(got, 0, ref(img, p))
    assert got[3][0][1].sum() == 0 and got[3][0][2].sum() == 0
    small = F.noise256(6, 9, 1)
    assert_frame(run_device(ctx, [small], prm(10, True, 1, 1, 5)), 0, (np.zeros((0, 2), np.float32), np.zeros(0, np.float32)))


def test_ragged_batch_equals_single_calls_and_the_host_form(ctx):
    """Five different frames in one call (counts from 0 to the cap) = five calls of one frame = ps_detect_features, which also
    takes a region of a larger image by its row stride."""
    rows, cols = 48, 64
    imgs = [F.SCENES["blocks"](rows, cols), np.full((rows, cols), 7, np.uint8), F.SCENES["noise256"](rows, cols),
            F.SCENES["noise4"](rows, cols), F.blocks(rows, cols, 9, 3)]
    for p in (prm(10, True, 2, 2, 150), prm(10, False, 1, 1, 150)):
        batch = run_device(ctx, imgs, p, padded=True)
        counts = batch[2].tolist()
        assert counts[1] == 0 and max(counts) == 150 and len(set(counts)) >= 3, counts
        for f, img in enumerate(imgs):
            want = ref(img, p)
            assert_frame(batch, f, want, f)
            assert_frame(run_device(ctx, [img], p), 0, want, f)
            parent = np.full((rows + 4, cols + 9), 0x33, np.uint8)
            parent[2:2 + rows, 5:5 + cols] = img
            xy, resp = ctx.detect_features(parent[2:2 + rows, 5:5 + cols], p)
            assert u32(xy).tolist() == u32(want[0]).tolist() and u32(resp).tolist() == u32(want[1]).tolist(), f


def test_host_form_reports_the_capacity_it_needs(ctx):
    img = F.SCENES["noise256"](48, 64)
    p = prm(10, True, 1, 1, 500)
    want = ref(img, p)
    n = len(want[1])
    assert n == 268
    L = ctx._L
    xy, resp = np.full((n, 2), SENT_F, np.uint32), np.full(n, SENT_F, np.uint32)
    nout = C.c_int(-7)
    args = (ctx._h, img.ctypes.data_as(C.c_void_p), 48, 64, 1, 0, C.byref(p), xy.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p))
    assert L.ps_detect_features(*args, n - 1, C.byref(nout)) == -1 and nout.value == n
    assert (xy == SENT_F).all() and (resp == SENT_F).all() and b"cap" in L.ps_last_error(ctx._h)
    assert L.ps_detect_features(*args, n, C.byref(nout)) == 0 and nout.value == n
    assert xy.tolist() == u32(want[0]).tolist() and resp.tolist() == u32(want[1]).tolist()


def test_errors_leave_the_outputs_untouched(ctx):
    """Every error of the C ABI's list, with its code, a text through ps_last_error and the outputs as they were."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import PS_MAX_KPTS, PsImageSet
    L, h = ctx._L, ctx._h
    rows, cols = 48, 64
    det = device_batch.FastDetector(ctx, rows, cols, 1, 2)
    imgs = upload_images([F.SCENES["noise256"](rows, cols)] * 2, False)
    cap = 40
    xy, resp, cnt = sentinels(2, cap)

    def image_set(frames=2, r=rows, c=cols, cn=1, row_stride=0, frame_stride=0, pixels=True):
        return PsImageSet(imgs.data_ptr() if pixels else None, row_stride, frame_stride, frames, r, c, cn)

    def call(s, p, capacity=cap, x=xy, r=resp, n=cnt, d=det.handle):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        return L.ps_detect_features_device(h, d, C.byref(s) if s is not None else None, C.byref(p) if p is not None else None,
                                           capacity, ptr(x), ptr(r), ptr(n))

    good = prm(10, True, 1, 1, cap)

    def with_field(name, value):
        p = prm(10, True, 1, 1, cap)
        setattr(p, name, value)
        return p

    bad_arg = [
        ("null detector", lambda: call(image_set(), good, d=None)),
        ("null images", lambda: call(None, good)),
        ("null params", lambda: call(image_set(), None)),
        ("null pixels", lambda: call(image_set(pixels=False), good)),
        ("null xy", lambda: call(image_set(), good, x=None)),
        ("null response", lambda: call(image_set(), good, r=None)),
        ("null counts", lambda: call(image_set(), good, n=None)),
        ("gridRows 0", lambda: call(image_set(), with_field("gridRows", 0))),
        ("gridCols -1", lambda: call(image_set(), with_field("gridCols", -1))),
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
        ("negative capacity", lambda: call(image_set(), prm(10, True, 1, 1, 0), capacity=-1)),
    ]
    for what, run in bad_arg:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    # the capacity rule is min(maximalTrackedFeatures, candidate pixels): 58 x 42 candidates here, 1 x 1 in an ROI of 7 x 7
    assert call(image_set(), prm(10, True, 1, 1, 3000), capacity=58 * 42 - 1) == -1
    unsupported = [
        ("maximum above PS_MAX_KPTS", lambda: call(image_set(), prm(10, True, 1, 1, PS_MAX_KPTS + 1), capacity=PS_MAX_KPTS)),
        ("capacity above PS_MAX_KPTS", lambda: call(image_set(), good, capacity=PS_MAX_KPTS + 1)),
    ]
    for what, run in unsupported:
        assert run() == -5, what
        assert len(L.ps_last_error(h)) > 0, what
    out = C.c_void_p(0x55)
    assert L.ps_fast_detector_create(h, 8193, 64, 1, 1, C.byref(out)) == -5 and not out.value
    out = C.c_void_p(0x55)
    assert L.ps_fast_detector_create(h, 48, 8193, 1, 1, C.byref(out)) == -5 and not out.value
    for bad in [(0, 64, 1, 1), (48, 0, 1, 1), (48, 64, 2, 1), (48, 64, 1, 0), (48, 64, 1, 65536)]:
        out = C.c_void_p(0x55)
        assert L.ps_fast_detector_create(h, *bad, C.byref(out)) == -1 and not out.value, bad
    assert L.ps_fast_detector_create(h, 48, 64, 1, 1, None) == -1
    # the host form: its own list
    img = F.SCENES["noise256"](rows, cols)
    hx, hr, nout = np.full((cap, 2), SENT_F, np.uint32), np.full(cap, SENT_F, np.uint32), C.c_int(-7)
    pv = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731

    def host(image=img, r=rows, c=cols, cn=1, stride=0, p=good, x=hx, rr=hr, capacity=cap, n=nout):
        return L.ps_detect_features(h, pv(image), r, c, cn, stride, C.byref(p) if p is not None else None, pv(x), pv(rr), capacity,
                                    C.byref(n) if n is not None else None)
    for what, run, code in [("null image", lambda: host(image=None), -1), ("null params", lambda: host(p=None), -1),
                            ("null xy", lambda: host(x=None), -1), ("null response", lambda: host(rr=None), -1),
                            ("null nout", lambda: host(n=None), -1), ("stride", lambda: host(stride=cols - 1), -1),
                            ("channels", lambda: host(cn=2), -1), ("rows 0", lambda: host(r=0), -1),
                            ("negative cap", lambda: host(capacity=-1), -1), ("reserved", lambda: host(p=with_field("reserved", 2)), -1),
                            ("gridRows", lambda: host(p=with_field("gridRows", 0)), -1),
                            ("rows above 8192", lambda: host(r=8193), -5),
                            ("maximum above PS_MAX_KPTS", lambda: host(p=prm(10, True, 1, 1, PS_MAX_KPTS + 1)), -5)]:
        assert run() == code, what
        assert len(L.ps_last_error(h)) > 0 and nout.value == -7, what
    assert (hx == SENT_F).all() and (hr == SENT_F).all()
    assert L.ps_debug_fast_maps(h, None, 0, None, None, None) == -1
    assert L.ps_debug_fast_maps(h, det.handle, 2, None, None, None) == -1 and L.ps_debug_fast_maps(h, det.handle, -1, None, None, None) == -1
    # nothing above wrote anything; zero frames is PS_OK and writes nothing either
    assert call(image_set(frames=0), good) == 0
    torch.cuda.synchronize()
    assert (u32(xy.cpu().numpy()) == SENT_F).all() and (u32(resp.cpu().numpy()) == SENT_F).all() and (cnt.cpu().numpy() == SENT_I).all()
    # ... and the same arguments, all in order, work
    assert call(image_set(), good) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [cap, cap]
    det.close()


def test_detected_arrays_drop_into_dbscan(ctx):
    """The refill chain's first two steps without a host step: the arrays ps_detect_features_device wrote go unchanged into
    ps_dbscan_thin_device, whose kept indices equal the restatement of DBScan on the restatement's key points."""
    import torch
    from putslam_amd import device_batch
    import dbscan_ref_py as R
    imgs = [F.SCENES["blocks"](96, 128), F.SCENES["noise256"](96, 128), np.full((96, 128), 50, np.uint8)]
    det = device_batch.FastDetector(ctx, 96, 128, 1, len(imgs))
    p = prm(10, True, 2, 2, 300)
    xy, resp, cnt = device_batch.detect_features_batch(ctx, det, upload_images(imgs, False), p)
    kept, nkept = device_batch.dbscan_thin_device(ctx, xy, cnt, None, 6.0, 2, 1)
    torch.cuda.synchronize()
    kept, nkept = kept.cpu().numpy(), nkept.cpu().numpy()
    thinned = 0
    for f, img in enumerate(imgs):
        wxy, _ = ref(img, p)
        want = R.dbscan_keep(wxy, None, 6.0, 2, 1)
        assert int(nkept[f]) == len(want) and kept[f, :len(want)].tolist() == want.tolist(), f
        thinned += len(wxy) - len(want)
    assert thinned > 0      # the thinning had something to do
    det.close()
