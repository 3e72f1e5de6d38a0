"""The measurement uncertainty on the GPU (putslam_amd/csrc/ps_uncertainty.h): ps_feature_uncertainty, ps_measurement_edges and the
host forms against the sequential restatement (tests/uncertainty_ref.py), byte for byte -- NaNs included: every NaN is the one
pattern 0x7FF8000000000000 on both sides.  Outputs start as sentinels and are checked beyond every count.

The scene: three frames of 20 x 14 pixels in blocks whose rows and frames are padded.  Depth frame 0 has about 30 % holes, frame 1
about 85 % and frame 2 about 55 %, so that every neighbour count 0 .. 8 and every branch of the gradient's ladder occurs; colour
frames 0 and 1 are noise, frame 2 is black but for four bytes that put a gradient on each diagonal (and (0, 0) everywhere else).
The restatement counts what it met (uncertainty_ref.SEEN) and test_scene_reaches_every_branch asserts the list."""
import ctypes as C
import itertools
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import uncertainty_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, FRAMES = 14, 20, 3
K = np.array([21.0, 0, 9.5, 0, 19.5, 6.5, 0, 0, 1], np.float32)
SCALE = 5000.0
CAP = 300                          # two blocks of 256 rows
PAD = 0xEEEE
SENT_D = np.uint64(0x7FF5A5A5A5A5A5A5)
SENT_I = np.int32(-0x5A5A5A5B)
SENT_F = np.uint32(0x7FA55A5A)
MEMBERS = ("normal", "gradient", "info")
WIDTH = dict(normal=3, gradient=3, info=9, position=3, uv=2)
SENSORS = dict(scaled=dict(scaleUncertaintyNormal=3.0, scaleUncertaintyGradient=0.25), default={})
TIE_PIXELS = {(1, 1): (4, 4), (-1, 1): (10, 4), (-1, -1): (4, 9), (1, -1): (10, 9)}      # (sgn gradx, sgn grady): (u, v)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def geometry():
    from putslam_amd._abi import frame_geometry
    return frame_geometry(K, (0.0,) * 5, SCALE)


def sensor_struct(name):
    from putslam_amd._abi import sensor_model
    return sensor_model(**SENSORS[name])


# ------------------------------------------------------------------------------------------------------------------ scene
def scene():
    """(depths (3, ROWS, COLS) uint16, images (3, ROWS, COLS, 3) uint8)"""
    rng = np.random.RandomState(7)
    deps = []
    for holes in (0.30, 0.85, 0.55):
        d = rng.randint(2000, 12000, size=(ROWS, COLS))
        d[rng.rand(ROWS, COLS) < holes] = 0
        deps.append(d.astype(np.uint16))
    imgs = [rng.randint(0, 256, size=(ROWS, COLS, 3)).astype(np.uint8) for _ in range(2)] + [np.zeros((ROWS, COLS, 3), np.uint8)]
    # one byte per tie: the low byte of patch word (r, c) of the pixel -- w22 gives (+, +), w02 (-, +), w00 (-, -), w20 (+, -)
    for (sx, sy), (u, v) in TIE_PIXELS.items():
        r, c = {(1, 1): (2, 2), (-1, 1): (0, 2), (-1, -1): (0, 0), (1, -1): (2, 0)}[sx, sy]
        imgs[2][v - 1 + r].reshape(-1)[(u - 1) * 3 + 2 * c] = 1
    return np.stack(deps), np.stack(imgs)


def padded_depth(deps):
    """The depth frames in a block whose rows (5 pixels) and frames (a row and 3 pixels) are padded with PAD: the device view"""
    import torch
    row, frame = COLS + 5, (ROWS + 1) * (COLS + 5) + 3
    flat = np.full(len(deps) * frame, PAD, np.uint16)
    for f, d in enumerate(deps):
        flat[f * frame:f * frame + ROWS * row].reshape(ROWS, row)[:, :COLS] = d
    return torch.as_strided(dev(flat.view(np.int16)), (len(deps), ROWS, COLS), (frame, row, 1))


def padded_images(imgs):
    """The colour frames in a block whose rows (7 bytes) and frames (two rows and 5 bytes) are padded with 0xEE"""
    import torch
    row, frame = COLS * 3 + 7, (ROWS + 2) * (COLS * 3 + 7) + 5
    flat = np.full(len(imgs) * frame, 0xEE, np.uint8)
    for f, im in enumerate(imgs):
        flat[f * frame:f * frame + ROWS * row].reshape(ROWS, row)[:, :COLS * 3] = im.reshape(ROWS, COLS * 3)
    return torch.as_strided(dev(flat), (len(imgs), ROWS, COLS, 3), (frame, row, 3, 1))


NAMED = np.float32([[3.7, 5.2], [19.9, 13.9], [-0.5, 3.0], [-3.2, -1.0], [np.nan, 4.0], [4.0, np.nan], [3e9, 2.0], [-2147483648.0, 1.0],
                    [2147483520.0, 5.0], [np.inf, 3.0], [20.0, 5.0], [5.0, 14.0], [20.0, 13.0]])
IMAGE_FRAME = [0, 1, 2, 3, 1, -1, 0]
N_ROWS = ROWS * COLS + len(NAMED)
COUNTS = [N_ROWS, N_ROWS, N_ROWS, 20, CAP + 1, 7, -1]


def row_inputs():
    """xy (F, CAP, 2): every integer pixel, then the named positions, the same in every set; pts (F, CAP, 3) with Z from a depth
    image's range, some 0, one NaN"""
    rng = np.random.RandomState(8)
    F = len(COUNTS)
    v, u = np.mgrid[0:ROWS, 0:COLS]
    one = np.concatenate([np.stack([u.ravel(), v.ravel()], 1).astype(np.float32), NAMED, np.zeros((CAP - N_ROWS, 2), np.float32)])
    xy = np.broadcast_to(one, (F, CAP, 2)).copy()
    pts = (rng.randint(0, 12000, size=(F, CAP, 3)) / SCALE).astype(np.float32)
    pts[:, ::9, 2] = 0
    pts[:, 5, 2] = np.nan
    return xy, pts


_REF = {}


def reference(model, sensor):
    """The restatement of every valid set, all three members (computed once per model and sensor)"""
    if (model, sensor) not in _REF:
        deps, imgs = scene()
        xy, pts = row_inputs()
        s = U.sensor(**SENSORS[sensor])
        out = []
        for f, (g, n) in enumerate(zip(IMAGE_FRAME, COUNTS)):
            if not 0 <= n <= CAP:
                out.append(None)
                continue
            inside = 0 <= g < FRAMES
            out.append(U.rows(xy[f, :n], pts[f, :n], deps[g] if inside else None, imgs[g] if inside else None, K, SCALE, s, model))
        _REF[model, sensor] = out
    return _REF[model, sensor]


def test_scene_reaches_every_branch():
    U.SEEN.clear()
    _REF.pop((2, "scaled"), None)
    ref = reference(2, "scaled")
    for k in range(9):
        assert U.SEEN["kept", k] > 0, (k, U.SEEN)
    for b in ("border", "end-beg", "cen-beg", "end-cen", "fallback"):
        assert U.SEEN["branch", b] > 0, (b, U.SEEN)
    for t in [(0, 0)] + list(TIE_PIXELS):
        assert U.SEEN["tie", t[0], t[1]] > 0, (t, U.SEEN)
    assert U.SEEN["bad pixel"] == 3 * 5          # two NaNs, 3e9, -2^31 and inf in each of the three full sets
    # the set whose frame lies outside is NaN everywhere; the named pixels did what their names say
    assert all((ref[3][m].view(np.uint64) == U.NAN_BITS).all() for m in MEMBERS)
    base = ROWS * COLS
    for i in (4, 5, 6, 7, 9):
        assert all((ref[0][m][base + i].view(np.uint64) == U.NAN_BITS).all() for m in MEMBERS), i
    assert np.array_equal(ref[0]["normal"][base + 0], ref[0]["normal"][5 * COLS + 3])        # (3.7, 5.2) is pixel (3, 5)
    assert np.array_equal(ref[0]["normal"][base + 1], ref[0]["normal"][13 * COLS + 19])
    assert np.array_equal(ref[0]["normal"][base + 2], ref[0]["normal"][3 * COLS + 0])        # (-0.5, 3) truncates to (0, 3)


def sentinels(F=len(COUNTS)):
    return {m: dev(np.full((F, CAP, WIDTH[m]), SENT_D, np.uint64).view(np.float64)) for m in MEMBERS}


def same_rows(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    bad = np.flatnonzero((g != w).reshape(len(g), g[0].size if len(g) else 1).any(axis=1))
    assert len(bad) == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


# ------------------------------------------------------------------------------------------------------------ the row call
@pytest.mark.parametrize("model", [-1, 0, 1, 2])
def test_feature_uncertainty_equals_the_restatement_for_every_subset_of_outputs(ctx, model):
    """Models -1 .. 2, each with every subset of NULL outputs; images NULL where neither the gradient nor model 2 is wanted (every
    second such subset); a count of capacity + 1 and of -1 write nothing; a frame outside the sets gives NaN rows; rows beyond a
    count keep the sentinel; the padding's bytes never show."""
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import PsUncertaintyOut
    deps, imgs = scene()
    xy, pts = row_inputs()
    ddep, dimg = padded_depth(deps), padded_images(imgs)
    ds, iset = D.DepthSet(ddep, ROWS, COLS), D._image_set(dimg, ROWS, COLS, 3)
    dxy, dpts, dcnt, dfr = dev(xy), dev(pts), dev(np.array(COUNTS, np.int32)), dev(np.array(IMAGE_FRAME, np.int32))
    geo, sens = geometry(), sensor_struct("scaled")
    want = reference(model, "scaled")
    subsets = [c for k in (1, 2, 3) for c in itertools.combinations(MEMBERS, k)]
    for number, subset in enumerate(subsets):
        out = sentinels()
        torch.cuda.synchronize()
        need_images = "gradient" in subset or ("info" in subset and model == 2)
        images = iset if need_images or number % 2 == 0 else None
        o = PsUncertaintyOut(*[out[m].data_ptr() if m in subset else None for m in MEMBERS])
        ctx.feature_uncertainty_device(geo, sens, model, images, ds, dfr.data_ptr(), dxy.data_ptr(), dpts.data_ptr(), dcnt.data_ptr(),
                                       len(COUNTS), CAP, o)
        ctx.synchronize()
        for m in MEMBERS:
            got = out[m].cpu().numpy()
            if m not in subset:
                assert (got.view(np.uint64) == SENT_D).all(), (subset, m)
                continue
            for f, n in enumerate(COUNTS):
                n = n if 0 <= n <= CAP else 0
                if n:
                    same_rows(got[f, :n], want[f][m], (model, subset, m, f))
                assert (got[f, n:].view(np.uint64) == SENT_D).all(), (model, subset, m, f)


def test_default_sensor_gives_what_the_arithmetic_gives(ctx):
    """The reference's default scale factors are 0: models 1 and 2 divide by a zero determinant.  inf and NaN, byte for byte."""
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import PsUncertaintyOut
    deps, imgs = scene()
    xy, pts = row_inputs()
    ddep, dimg = padded_depth(deps), padded_images(imgs)      # (held: the sets below name their memory)
    ds, iset = D.DepthSet(ddep, ROWS, COLS), D._image_set(dimg, ROWS, COLS, 3)
    dxy, dpts, dcnt, dfr = dev(xy), dev(pts), dev(np.array(COUNTS, np.int32)), dev(np.array(IMAGE_FRAME, np.int32))
    for model in (1, 2):
        out = sentinels()
        torch.cuda.synchronize()
        ctx.feature_uncertainty_device(geometry(), sensor_struct("default"), model, iset, ds, dfr.data_ptr(), dxy.data_ptr(), dpts.data_ptr(),
                                       dcnt.data_ptr(), 1, CAP, PsUncertaintyOut(None, None, out["info"].data_ptr()))
        ctx.synchronize()
        want = U.rows(xy[0, :N_ROWS], pts[0, :N_ROWS], deps[0], imgs[0], K, SCALE, U.sensor(), model, want=("info",))["info"]
        same_rows(out["info"].cpu().numpy()[0, :N_ROWS], want, model)
        assert not np.isfinite(want).all()


def test_host_forms_equal_the_restatement_on_regions_of_larger_images(ctx):
    deps, imgs = scene()
    xy, pts = row_inputs()
    n = N_ROWS
    dparent = np.full((ROWS + 3, COLS + 6), PAD, np.uint16)
    dparent[1:1 + ROWS, 2:2 + COLS] = deps[2]
    iparent = np.full((ROWS + 4, COLS + 9, 3), 0xEE, np.uint8)
    iparent[2:2 + ROWS, 5:5 + COLS] = imgs[2]
    dview, iview = dparent[1:1 + ROWS, 2:2 + COLS], iparent[2:2 + ROWS, 5:5 + COLS]
    geo = geometry()
    want = reference(2, "scaled")[2]
    same_rows(ctx.compute_normals(xy[2, :n], dview, geo), want["normal"], "normals")
    same_rows(ctx.compute_rgb_gradients(xy[2, :n], iview, dview, geo), want["gradient"], "gradients")
    same_rows(ctx.information_matrices(xy[2, :n], pts[2, :n], dview, geo, sensor_struct("scaled"), 2, iview).reshape(n, 9), want["info"], "info 2")
    for model in (-1, 0, 1):
        got = ctx.information_matrices(xy[2, :n], pts[2, :n], dview, geo, sensor_struct("scaled"), model)
        same_rows(got.reshape(n, 9), reference(model, "scaled")[2]["info"], model)
    assert ctx.compute_normals(np.zeros((0, 2), np.float32), dview, geo).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------- the edges
MAP_CAP, MAX_MATCHES = 96, 128
EDGE_INLIERS = [0, 1, 63, 64, 70]
EDGE_PAIRS = [[0, 0], [1, 1], [0, 2], [1, 0], [0, 1], [1, 2], [0, 3]]        # the last names a frame outside the set of three
EDGE_FRAME = [2, 0, 1]                                                       # imageFrame of the batch's three frames


def edge_batch(seed=3):
    """A map batch of two views and three frames of MAP_CAP rows whose result block is written by hand: pairs with 0, 1, 63, 64
    and 70 inliers in lists of 0 .. 128 matches with holes in the mask, one overflowed pair (numMatches < 0) and one that names a
    frame outside the set.  Returns (batch, xy_undist (3, MAP_CAP, 2), host copies)."""
    from putslam_amd import device_batch as D
    from putslam_amd._abi import DMATCH_DTYPE
    rng = np.random.RandomState(seed)
    desc = rng.randint(0, 256, size=(3, MAP_CAP, 32)).astype(np.uint8)
    fpts = (rng.rand(3, MAP_CAP, 3) * 3 + 0.5).astype(np.float32)
    xyu = (rng.rand(3, MAP_CAP, 2) * [COLS + 2, ROWS + 2] - 1).astype(np.float32)
    xyu[:, 3] = [np.nan, 2.0]
    frames = D.FrameSetDevice(desc, fpts, [MAP_CAP] * 3)
    maps = D.FrameSetDevice(desc[:2], fpts[:2], [MAP_CAP] * 2)
    level = np.zeros((3, MAP_CAP), np.int32)
    batch = D.MapBatchDevice(maps, level[:2], frames, level, EDGE_PAIRS, MAX_MATCHES)
    P = len(EDGE_PAIRS)
    matches = np.zeros((P, MAX_MATCHES), DMATCH_DTYPE)
    matches["queryIdx"] = rng.randint(0, MAP_CAP, size=(P, MAX_MATCHES))
    matches["trainIdx"] = rng.randint(0, MAP_CAP, size=(P, MAX_MATCHES))
    matches["trainIdx"][4, 2] = 3                       # the row whose position is NaN, made an inlier below
    mask = np.zeros((P, MAX_MATCHES), np.uint8)
    num = np.array([17, 90, 100, 128, 128, -300, 60], np.int32)
    for p, k in enumerate(EDGE_INLIERS):
        mask[p, rng.permutation(num[p])[:k]] = 1
    if not mask[4, 2]:
        mask[4, np.flatnonzero(mask[4])[0]] = 0
        mask[4, 2] = 1
    mask[5, :40] = 1                                    # an overflowed pair's rows mean nothing
    mask[6, :30] = 1                                    # ... nor those of a pair outside the set
    mask[1, 95:] = 1                                    # beyond numMatches: not read
    import torch
    batch.matches.copy_(dev(matches.view(np.uint8).reshape(P, MAX_MATCHES, 16)))
    batch.num_matches.copy_(dev(num))
    batch.mask.copy_(dev(mask))
    torch.cuda.synchronize()
    return batch, dev(xyu), dict(matches=matches, num=num, mask=mask, pts=fpts, xyu=xyu)


def edge_sentinels(P):
    from putslam_amd import device_batch as D
    out = D.MeasurementEdges(P, MAX_MATCHES, "cuda:0")
    fill = {np.dtype(np.int32): SENT_I, np.dtype(np.float32): SENT_F, np.dtype(np.float64): SENT_D}
    for name in ("count", "map_row", "cur_row", "uv", "position", "normal", "gradient", "info"):
        t = getattr(out, name)
        a = t.cpu().numpy()
        word = {4: np.uint32 if a.dtype.kind == "f" else np.int32, 8: np.uint64}[a.dtype.itemsize]
        setattr(out, name, dev(np.full(a.shape, fill[a.dtype], word).view(a.dtype)))
    return out


def untouched(a):
    fill = {np.dtype(np.int32): SENT_I, np.dtype(np.float32): SENT_F, np.dtype(np.float64): SENT_D}[a.dtype]
    word = {np.dtype(np.int32): np.int32, np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}[a.dtype]
    return bool((np.ascontiguousarray(a).view(word) == fill).all())


@pytest.mark.parametrize("model", [0, 1, 2])
def test_measurement_edges_equal_numpy_and_the_restatement(ctx, model):
    """count, mapRow, curRow, uv and position are what numpy derives from the mask and the matches, in match-list order; normal,
    gradient and info are the restatement's on those rows; rows beyond a count keep the sentinel"""
    import torch
    from putslam_amd import device_batch as D
    deps, imgs = scene()
    batch, dxyu, host = edge_batch()
    P = len(EDGE_PAIRS)
    out = edge_sentinels(P)
    torch.cuda.synchronize()
    D.measurement_edges(ctx, batch, dxyu, geometry(), padded_depth(deps), padded_images(imgs), sensor_struct("scaled"), model,
                        np.array(EDGE_FRAME, np.int32), out=out)
    torch.cuda.synchronize()
    got = out.download()
    want = U.measurement_edges(host["matches"], host["num"], host["mask"], EDGE_PAIRS, 2, host["pts"], host["xyu"], EDGE_FRAME, list(deps),
                               list(imgs), K, SCALE, U.sensor(**SENSORS["scaled"]), model, MAX_MATCHES)
    assert got["count"].tolist() == EDGE_INLIERS + [0, 0] == [w["count"] for w in want]
    for p, w in enumerate(want):
        n = w["count"]
        if n:
            # numpy's derivation, spelled out once more: the indices of the set mask bytes below numMatches, ascending
            idx = np.flatnonzero(host["mask"][p, :host["num"][p]])
            assert np.array_equal(got["map_row"][p, :n], host["matches"]["queryIdx"][p, idx])
            assert np.array_equal(got["cur_row"][p, :n], host["matches"]["trainIdx"][p, idx]) and np.array_equal(got["cur_row"][p, :n], w["curRow"])
            fr = EDGE_PAIRS[p][1]
            assert got["uv"][p, :n].tobytes() == host["xyu"][fr, w["curRow"]].tobytes()
            same_rows(got["position"][p, :n], U.canon(host["pts"][fr, w["curRow"]].astype(np.float64)), ("position", p))
            for m in MEMBERS:
                same_rows(got[m][p, :n], w[m], (model, m, p))
        for name in ("map_row", "cur_row", "uv", "position") + MEMBERS:
            assert untouched(got[name][p, n:]), (name, p)
    # the NaN position's row is NaN in every member
    k = int(np.flatnonzero(np.flatnonzero(host["mask"][4, :128]) == 2)[0])
    assert all((got[m][4, k].view(np.uint64) == U.NAN_BITS).all() for m in MEMBERS)


TRAIN_OUTSIDE = (-1, MAP_CAP, -2 ** 31, 2 ** 31 - 1)


def test_a_train_index_outside_the_frame_is_not_followed(ctx):
    """include/putslam_hip.h: "a trainIdx outside 0 .. b->frames.maxKpts - 1 is not followed: that row is NaN".  Inliers of two
    lists carry -1, maxKpts, INT32_MIN and INT32_MAX: uv, position and every member of those rows are NaN, mapRow and curRow are the
    list's own values, the counts include the rows, and every other row is what it was."""
    import torch
    from putslam_amd import device_batch as D
    deps, imgs = scene()
    batch, dxyu, host = edge_batch()
    P = len(EDGE_PAIRS)
    matches = host["matches"].copy()
    planted = {}
    for p in (3, 4):
        inl = np.flatnonzero(host["mask"][p, :host["num"][p]])
        at = [k for k in (0, len(inl) // 3, len(inl) // 2, len(inl) - 1)]       # the first and the last inlier among them
        for k, t in zip(at, TRAIN_OUTSIDE if p == 3 else TRAIN_OUTSIDE[::-1]):
            matches["trainIdx"][p, inl[k]] = t
            planted[p, k] = t
    batch.matches.copy_(dev(matches.view(np.uint8).reshape(P, MAX_MATCHES, 16)))
    out = edge_sentinels(P)
    torch.cuda.synchronize()
    D.measurement_edges(ctx, batch, dxyu, geometry(), padded_depth(deps), padded_images(imgs), sensor_struct("scaled"), 2,
                        np.array(EDGE_FRAME, np.int32), out=out)
    torch.cuda.synchronize()
    got = out.download()
    want = U.measurement_edges(matches, host["num"], host["mask"], EDGE_PAIRS, 2, host["pts"], host["xyu"], EDGE_FRAME, list(deps), list(imgs), K,
                               SCALE, U.sensor(**SENSORS["scaled"]), 2, MAX_MATCHES)
    assert got["count"].tolist() == EDGE_INLIERS + [0, 0] == [w["count"] for w in want]
    for (p, k), t in planted.items():
        assert got["cur_row"][p, k] == t and got["map_row"][p, k] == want[p]["mapRow"][k]
        assert (got["uv"][p, k].view(np.uint32) == 0x7FC00000).all(), (p, k, got["uv"][p, k])
        for m in ("position",) + MEMBERS:
            assert (got[m][p, k].view(np.uint64) == U.NAN_BITS).all(), (m, p, k, got[m][p, k])
    for p, w in enumerate(want):
        n = w["count"]
        if n:
            assert np.array_equal(got["map_row"][p, :n], w["mapRow"]) and np.array_equal(got["cur_row"][p, :n], w["curRow"])
            assert got["uv"][p, :n].tobytes() == w["uv"].tobytes(), p
            for m in ("position",) + MEMBERS:
                same_rows(got[m][p, :n], w[m], (m, p))
        for name in ("map_row", "cur_row", "uv", "position") + MEMBERS:
            assert untouched(got[name][p, n:]), (name, p)
    # the rows beside the planted ones are not all NaN: the rule touched its rows alone
    assert np.isfinite(got["position"][3, 1]).all() and np.isfinite(got["position"][4, 1]).all()


TILE_MATCHES = 640                              # three tiles of 256 mask bytes
TILE_INLIERS = [255, 256, 257, 600, 1, 513]
TILE_NUM = [600, 610, 640, 600, 300, 640]


def test_measurement_edges_cross_the_tiles_of_the_scan(ctx):
    """Lists of 300 .. 640 matches -- two and three tiles of the 256-wide scan -- with 255, 256, 257, 513 and 600 inliers and holes
    in the mask, and one list whose only inlier lies in the second tile: the running offset, the reuse of the scan's LDS from tile
    to tile and the rows written from the second tile on.  Byte for byte, like the others."""
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import DMATCH_DTYPE
    deps, imgs = scene()
    rng = np.random.RandomState(12)
    P = len(TILE_INLIERS)
    desc = rng.randint(0, 256, size=(3, MAP_CAP, 32)).astype(np.uint8)
    fpts = (rng.rand(3, MAP_CAP, 3) * 3 + 0.5).astype(np.float32)
    xyu = (rng.rand(3, MAP_CAP, 2) * [COLS + 2, ROWS + 2] - 1).astype(np.float32)
    pairs = [[p % 2, p % 3] for p in range(P)]
    level = np.zeros((3, MAP_CAP), np.int32)
    batch = D.MapBatchDevice(D.FrameSetDevice(desc[:2], fpts[:2], [MAP_CAP] * 2), level[:2], D.FrameSetDevice(desc, fpts, [MAP_CAP] * 3), level, pairs,
                             TILE_MATCHES)
    matches = np.zeros((P, TILE_MATCHES), DMATCH_DTYPE)
    matches["queryIdx"] = rng.randint(0, MAP_CAP, size=(P, TILE_MATCHES))
    matches["trainIdx"] = rng.randint(0, MAP_CAP, size=(P, TILE_MATCHES))
    mask = np.zeros((P, TILE_MATCHES), np.uint8)
    num = np.array(TILE_NUM, np.int32)
    for p, k in enumerate(TILE_INLIERS):
        mask[p, rng.permutation(num[p])[:k]] = 1
    mask[4] = 0
    mask[4, 277] = 1                            # the first tile has no inlier
    for p in range(1, P, 2):
        mask[p, num[p]:] = 1                    # beyond numMatches: not read
    batch.matches.copy_(dev(matches.view(np.uint8).reshape(P, TILE_MATCHES, 16)))
    batch.num_matches.copy_(dev(num))
    batch.mask.copy_(dev(mask))
    out = D.MeasurementEdges(P, TILE_MATCHES, "cuda:0")
    for name in ("map_row", "cur_row"):
        setattr(out, name, dev(np.full((P, TILE_MATCHES), SENT_I, np.int32)))
    for name in ("position",) + MEMBERS:
        setattr(out, name, dev(np.full((P, TILE_MATCHES, WIDTH[name]), SENT_D, np.uint64).view(np.float64)))
    ddep, dimg = padded_depth(deps), padded_images(imgs)
    torch.cuda.synchronize()
    D.measurement_edges(ctx, batch, dev(xyu), geometry(), ddep, dimg, sensor_struct("scaled"), 2, np.array(EDGE_FRAME, np.int32), out=out)
    torch.cuda.synchronize()
    got = out.download()
    want = U.measurement_edges(matches, num, mask, pairs, 2, fpts, xyu, EDGE_FRAME, list(deps), list(imgs), K, SCALE, U.sensor(**SENSORS["scaled"]), 2,
                               TILE_MATCHES)
    assert got["count"].tolist() == [w["count"] for w in want] == [int(mask[p, :num[p]].sum()) for p in range(P)]
    assert got["count"].tolist()[:3] == [255, 256, 257] and got["count"][4] == 1 and got["count"][3] == 600 and got["count"][5] == 513
    for p, w in enumerate(want):
        n = w["count"]
        idx = np.flatnonzero(mask[p, :num[p]])
        assert (idx >= 256).any() and np.array_equal(got["map_row"][p, :n], matches["queryIdx"][p, idx])
        assert np.array_equal(got["cur_row"][p, :n], matches["trainIdx"][p, idx])
        assert got["uv"][p, :n].tobytes() == xyu[pairs[p][1], w["curRow"]].tobytes()
        for m in ("position",) + MEMBERS:
            same_rows(got[m][p, :n], w[m], (m, p))
        for name in ("map_row", "cur_row", "position") + MEMBERS:
            assert untouched(got[name][p, n:]), (name, p)


def test_measurement_edges_with_outputs_absent_and_without_images(ctx):
    import torch
    from putslam_amd import device_batch as D
    deps, imgs = scene()
    batch, dxyu, host = edge_batch()
    full = D.measurement_edges(ctx, batch, dxyu, geometry(), padded_depth(deps), padded_images(imgs), sensor_struct("scaled"), 1, np.array(EDGE_FRAME, np.int32))
    torch.cuda.synchronize()
    ref = full.download()
    for want in (["info"], ["count", "position", "info"], ["map_row", "cur_row"], ["uv", "normal"]):
        names = [w for w in want if w != "count"]
        out = D.measurement_edges(ctx, batch, dxyu, geometry(), padded_depth(deps), None, sensor_struct("scaled"), 1, np.array(EDGE_FRAME, np.int32),
                                  want=names)
        torch.cuda.synchronize()
        got = out.download()
        assert sorted(got) == sorted(["count"] + names) and got["count"].tolist() == ref["count"].tolist()
        for name in names:
            assert got[name].tobytes() == ref[name].tobytes(), (want, name)


def test_map_pairs_results_flow_into_measurement_edges(ctx):
    """ps_map_pairs_device's own block, with no host step in between: the views are the frames a centimetre off, RANSAC accepts,
    and the edges are the inliers of its mask in its order"""
    import torch
    from putslam_amd import device_batch as D, synth
    from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config
    deps, imgs = scene()
    rng = np.random.default_rng(5)
    cap = 64
    seq = synth.make_sequence(2, cap, config=3, index=77)
    vdesc = seq["desc"] ^ np.packbits(rng.random((2, cap, 256)) < 0.03, axis=2)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)
    level = np.zeros((2, cap), np.int32)
    batch = D.MapBatchDevice(D.FrameSetDevice(vdesc, vpos, [cap, cap]), level, D.FrameSetDevice(seq["desc"], seq["pts"], [cap, cap]), level,
                             [[0, 0], [1, 1], [0, 1]], 4 * cap)
    xyu = (np.random.RandomState(4).rand(2, cap, 2) * [COLS, ROWS]).astype(np.float32)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=17)
    D.run_map_pairs(ctx, prm, cfg, TUM_FR1_K, batch)
    out = D.measurement_edges(ctx, batch, dev(xyu), geometry(), padded_depth(deps), padded_images(imgs), sensor_struct("scaled"), 2,
                              np.array([1, 0], np.int32))
    torch.cuda.synchronize()
    res, got = batch.download(), out.download()
    want = U.measurement_edges(res["matches"], res["numMatches"], res["inlierMask"], [[0, 0], [1, 1], [0, 1]], 2, seq["pts"], xyu, [1, 0], list(deps),
                               list(imgs), K, SCALE, U.sensor(**SENSORS["scaled"]), 2, 4 * cap)
    assert got["count"].tolist() == [w["count"] for w in want]
    assert got["count"][0] >= 15 and got["count"][1] >= 15
    for p, w in enumerate(want):
        n = w["count"]
        if n:
            assert np.array_equal(got["map_row"][p, :n], w["mapRow"]) and np.array_equal(got["cur_row"][p, :n], w["curRow"])
            for m in ("position",) + MEMBERS:
                same_rows(got[m][p, :n], w[m], (m, p))


# ------------------------------------------------------------------------------------------------------------ composition
def test_front_end_rows_feed_feature_uncertainty_with_no_host_step(ctx):
    """xyUndist and pts as ps_front_end_frames leaves them go into ps_feature_uncertainty on the device; the normals equal the host
    form ps_compute_normals on the downloaded frame"""
    import torch
    import frame_assembly_ref as A
    from image_frontend_util import upload_images
    from putslam_amd import device_batch as D
    from putslam_amd._abi import frame_geometry, front_end_params, orb_detect_params, orb_params
    name, p, levels = A.CASES[0]
    det = orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])
    fe = D.FrontEnd(ctx, A.ROWS, A.COLS, 3, 4, front_end_params(det, orb_params(p["scale_factor"], levels), A.DBSCAN_EPS))
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    imgs, deps = A.images(3), A.depths()
    dimg, ddep = upload_images(imgs, False), dev(np.stack(deps).view(np.int16))
    rows = D.front_end_frames_batch(ctx, fe, dimg, ddep, geo, A.CAPACITY)
    out = D.feature_uncertainty(ctx, rows, geo, ddep, dimg, model=1, sensor=sensor_struct("scaled"))
    torch.cuda.synchronize()
    got, fr = out.download(), rows.download()
    assert got["count"].tolist() == fr["nkpts"].tolist() and fr["nkpts"][0] > 10
    for f, n in enumerate(fr["nkpts"].tolist()):
        same_rows(got["normal"][f, :n], ctx.compute_normals(fr["xy_undist"][f, :n], deps[f], geo), f)
        same_rows(got["gradient"][f, :n], ctx.compute_rgb_gradients(fr["xy_undist"][f, :n], imgs[f], deps[f], geo), f)
        same_rows(got["info"][f, :n].reshape(n, 9), ctx.information_matrices(fr["xy_undist"][f, :n], fr["pts"][f, :n], deps[f], geo,
                                                                             sensor_struct("scaled"), 1).reshape(n, 9), f)
        assert not got["normal"][f, n:].any()
    # ... and one frame against the restatement itself
    n = int(fr["nkpts"][0])
    want = U.rows(fr["xy_undist"][0, :n], fr["pts"][0, :n], deps[0], imgs[0], A.K, A.DEPTH_SCALE, U.sensor(**SENSORS["scaled"]), 1)
    for m in MEMBERS:
        same_rows(got[m][0, :n], want[m], m)
    fe.close()


# ----------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_outputs_untouched(ctx):
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import PS_MAX_KPTS, PsDepthSet, PsImageSet, PsMeasurementEdgesOut, PsUncertaintyOut
    L, h = ctx._L, ctx._h
    deps, imgs = scene()
    ddep, dimg = padded_depth(deps), padded_images(imgs)
    xy, pts = row_inputs()
    dxy, dpts, dcnt, dfr = dev(xy), dev(pts), dev(np.array(COUNTS, np.int32)), dev(np.array(IMAGE_FRAME, np.int32))
    out = sentinels()
    geo, sens = geometry(), sensor_struct("scaled")
    good_d, good_i = D.DepthSet(ddep, ROWS, COLS), D._image_set(dimg, ROWS, COLS, 3)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def depth_set(**kw):
        d = PsDepthSet(good_d.pixels, good_d.rowStride, good_d.frameStride, good_d.numFrames, good_d.rows, good_d.cols)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def image_set(**kw):
        s = PsImageSet(good_i.pixels, good_i.rowStride, good_i.frameStride, good_i.numFrames, good_i.rows, good_i.cols, good_i.channels)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def rows_out(**kw):
        o = PsUncertaintyOut(out["normal"].data_ptr(), out["gradient"].data_ptr(), out["info"].data_ptr())
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(g=geo, s=sens, model=2, images=None, depth=None, fr=dfr, x=dxy, p=dpts, n=dcnt, F=len(COUNTS), cap=CAP, o=None, null=()):
        images, depth, o = images or image_set(), depth or depth_set(), o or rows_out()
        ref = lambda v, key: None if key in null else C.byref(v)   # noqa: E731
        return L.ps_feature_uncertainty(h, ref(g, "geometry"), ref(s, "sensor"), model, ref(images, "images"), ref(depth, "depth"), ptr(fr), ptr(x),
                                        ptr(p), ptr(n), F, cap, ref(o, "out"))

    bad = [("null geometry", lambda: call(null=("geometry",))), ("null sensor", lambda: call(null=("sensor",))),
           ("null depth", lambda: call(null=("depth",))), ("null out", lambda: call(null=("out",))),
           ("null images with the gradient", lambda: call(null=("images",))),
           ("null images with model 2", lambda: call(null=("images",), o=rows_out(normal=None, gradient=None))),
           ("model 3", lambda: call(model=3)), ("model -2", lambda: call(model=-2)), ("null imageFrame", lambda: call(fr=None)),
           ("null xy", lambda: call(x=None)), ("null counts", lambda: call(n=None)), ("null pts with model 0", lambda: call(model=0, p=None)),
           ("no output wanted", lambda: call(o=rows_out(normal=None, gradient=None, info=None))),
           ("depth row stride", lambda: call(depth=depth_set(rowStride=COLS * 2 - 2))), ("odd depth row stride", lambda: call(depth=depth_set(rowStride=COLS * 2 + 1))),
           ("depth frame stride below a view", lambda: call(depth=depth_set(frameStride=2))), ("null depth pixels", lambda: call(depth=depth_set(pixels=None))),
           ("image row stride", lambda: call(images=image_set(rowStride=COLS * 3 - 1))), ("image frame stride", lambda: call(images=image_set(frameStride=5))),
           ("images of another shape", lambda: call(images=image_set(rows=ROWS - 1))), ("null pixels", lambda: call(images=image_set(pixels=None))),
           ("negative F", lambda: call(F=-1)), ("F above 65535", lambda: call(F=65536)), ("capacity 0", lambda: call(cap=0))]
    for what, run in bad:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    assert call(images=image_set(channels=1)) == -5 and b"3-channel" in L.ps_last_error(h)
    assert call(cap=PS_MAX_KPTS + 1) == -5
    assert call(F=0) == 0
    # images are not needed, and a sensor is not, where nothing asks for them
    assert call(model=1, null=("images",), o=rows_out(gradient=None)) == 0
    assert call(model=-1, null=("images", "sensor"), o=rows_out(gradient=None, info=None)) == 0
    torch.cuda.synchronize()
    assert (out["gradient"].cpu().numpy().view(np.uint64) == SENT_D).all()

    # ps_measurement_edges
    batch, dxyu, _ = edge_batch()
    eout = edge_sentinels(len(EDGE_PAIRS))
    dframe = dev(np.array(EDGE_FRAME, np.int32))

    def edges(model=2, images=None, depth=None, fr=dframe, b=None, res=None, xyu=dxyu, o=None, null=()):
        images, depth = images or image_set(), depth or depth_set()
        b, res, o = b or batch.batch_view().struct(), res or batch.view().struct(), o or eout.edges_struct()
        ref = lambda v, key: None if key in null else C.byref(v)   # noqa: E731
        return L.ps_measurement_edges(h, C.byref(geo), ref(sens, "sensor"), model, ref(images, "images"), ref(depth, "depth"), ptr(fr), ref(b, "batch"),
                                      ref(res, "results"), ptr(xyu), ref(o, "out"))

    def with_field(s, path, value):
        target = s
        for name in path[:-1]:
            target = getattr(target, name)
        setattr(target, path[-1], value)
        return s

    mb, rs = (lambda: batch.batch_view().struct()), (lambda: batch.view().struct())
    bad = [("null batch", lambda: edges(null=("batch",))), ("null results", lambda: edges(null=("results",))), ("null out", lambda: edges(null=("out",))),
           ("null sensor", lambda: edges(null=("sensor",))), ("null images", lambda: edges(null=("images",))), ("null depth", lambda: edges(null=("depth",))),
           ("null xyUndist", lambda: edges(xyu=None)), ("null imageFrame", lambda: edges(fr=None)), ("model 3", lambda: edges(model=3)),
           ("P < 0", lambda: edges(b=with_field(mb(), ("P",), -1))), ("maxMatches 0", lambda: edges(b=with_field(mb(), ("maxMatches",), 0))),
           ("null pairs", lambda: edges(b=with_field(mb(), ("pairs",), None))), ("null points", lambda: edges(b=with_field(mb(), ("frames", "pts"), None))),
           ("points stride", lambda: edges(b=with_field(mb(), ("frames", "ptsFrameStride"), MAP_CAP * 12 - 4))),
           ("no frames", lambda: edges(b=with_field(mb(), ("frames", "numFrames"), 0))),
           ("null matches", lambda: edges(res=with_field(rs(), ("matches",), None))), ("null numMatches", lambda: edges(res=with_field(rs(), ("numMatches",), None))),
           ("null mask", lambda: edges(res=with_field(rs(), ("inlierMask",), None)))]
    for what, run in bad:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    assert edges(images=image_set(channels=1)) == -5
    assert edges(b=with_field(mb(), ("maxMatches",), (1 << 22) + 1)) == -5
    assert edges(b=with_field(mb(), ("frames", "maxKpts"), PS_MAX_KPTS + 1)) == -5
    assert edges(b=with_field(mb(), ("P",), 0)) == 0
    torch.cuda.synchronize()
    got = eout.download()
    assert all(untouched(v) for v in got.values())
    assert edges() == 0
    torch.cuda.synchronize()
    assert eout.download()["count"].tolist() == EDGE_INLIERS + [0, 0]
    # the host forms
    d0, x0 = np.ascontiguousarray(deps[0]), np.ascontiguousarray(xy[0])
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    nout = np.full((4, 3), 7.0)
    assert L.ps_compute_normals(h, C.byref(geo), pv(d0), ROWS, COLS, 0, pv(x0), PS_MAX_KPTS + 1, pv(nout)) == -5
    assert L.ps_compute_normals(h, C.byref(geo), None, ROWS, COLS, 0, pv(x0), 4, pv(nout)) == -1
    assert L.ps_compute_normals(h, C.byref(geo), pv(d0), ROWS, COLS, COLS * 2 - 2, pv(x0), 4, pv(nout)) == -1
    assert L.ps_compute_normals(h, C.byref(geo), pv(d0), ROWS, COLS, 0, pv(x0), -1, pv(nout)) == -1
    i1 = np.zeros((ROWS, COLS), np.uint8)
    assert L.ps_compute_rgb_gradients(h, C.byref(geo), pv(i1), 1, 0, pv(d0), ROWS, COLS, 0, pv(x0), 4, pv(nout)) == -5
    assert (nout == 7.0).all()


# ------------------------------------------------------------------------------------------------------------ stream order
BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64      # about 10 ms on the MI355X (tests/test_gpu_stream_handover.py measured it)


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def prep_rows(k, ctx):
    """ps_feature_uncertainty: the inputs -- depth, images, xy, pts, counts, imageFrame -- hold zeros before the copies"""
    import stream_order_cases as S
    import torch
    from putslam_amd import device_batch as D
    deps, imgs = scene()
    xy, pts = row_inputs()
    order = [k, 2, 1 - k]
    final = [S._up(deps[order].view(np.int16)), S._up(imgs[order]), S._up(xy[:3]), S._up(pts[:3]), S._up(np.array([N_ROWS, 50 + k, CAP], np.int32)),
             S._up(np.array([2, 0, 1], np.int32))]
    stale = S._stale(final)
    rows = D.FrameRowsDevice(3, CAP, S.DEV, side=("xy_undist",))
    rows.xy_undist, rows.pts, rows.nkpts = stale[2], stale[3], stale[4]
    out = D.MeasurementEdges(3, CAP, S.DEV, MEMBERS, count=stale[4])
    geo, sens = geometry(), sensor_struct("scaled")

    def call(c, direct=False):
        D.feature_uncertainty(c, rows, geo, stale[0], stale[1], sens, 2, stale[5], out=out, use_torch_stream=not direct)
    return S.Case(stale, final, call, lambda: [out.normal, out.gradient, out.info], lambda: stale[4],
                  lambda got: [S.mask_rows(g.view(torch.int64), final[4]) for g in got])


def prep_edges(k, ctx):
    """ps_measurement_edges: the result block, the frames' points, xyUndist, depth and images hold zeros before the copies"""
    import stream_order_cases as S
    from putslam_amd import device_batch as D
    deps, imgs = scene()
    batch, dxyu, host = edge_batch(30 + k)
    final = [batch.matches.clone(), batch.num_matches.clone(), batch.mask.clone(), batch.frames.pts.clone(), dxyu, S._up(deps.view(np.int16)), S._up(imgs)]
    stale = S._stale(final)
    batch.matches, batch.num_matches, batch.mask, batch.frames.pts = stale[0], stale[1], stale[2], stale[3]
    out = D.MeasurementEdges(len(EDGE_PAIRS), MAX_MATCHES, S.DEV)
    geo, sens, fr = geometry(), sensor_struct("scaled"), S._up(np.array(EDGE_FRAME, np.int32))

    def call(c, direct=False):
        D.measurement_edges(c, batch, stale[4], geo, stale[5], stale[6], sens, 2, fr, out=out, use_torch_stream=not direct)

    def outputs():
        return [out.count, out.map_row, out.cur_row, out.uv, out.position, out.normal, out.gradient, out.info]

    def norm(got):
        import torch
        return [got[0]] + [S.mask_rows(g.view(torch.int64) if g.dtype == torch.float64 else g.view(torch.int32), got[0]) for g in got[1:]]
    return S.Case(stale, final, call, outputs, lambda: out.count[:5].clamp(min=1), norm)


PREPS = {"rows": prep_rows, "edges": prep_edges}
_WANT = {}


def order_want(ctx, what, k):
    """What a fully synchronised run of case k computes (computed once)."""
    import torch
    if (what, k) not in _WANT:
        case = PREPS[what](k, ctx)
        for t, f in zip(case.inputs, case.finals):
            t.copy_(f)
        torch.cuda.synchronize()
        case.call(ctx)
        torch.cuda.synchronize()
        assert bool((case.counts() > 0).all()), case.counts()
        _WANT[what, k] = case.norm([t.clone() for t in case.outputs()])
        torch.cuda.synchronize()
        ctx.set_stream(0)
    return _WANT[what, k]


@pytest.mark.parametrize("how", ["default", "side", "direct"])
@pytest.mark.parametrize("what", list(PREPS))
def test_call_keeps_the_order_of_its_stream(ctx, ballast, what, how):
    """The protocol of tests/stream_order_cases.py (its helpers, unchanged) applied to the two new entry points: the inputs hold
    valid stale content (zeros), the real inputs are copied in on the stream under test, which is still busy with a ballast when the
    call is queued; a copy queued behind the call must hold what a fully synchronised run computes."""
    import stream_order_cases as S
    import torch
    expect = order_want(ctx, what, 0)
    other = order_want(ctx, what, 1)
    assert any(not torch.equal(a, b) for a, b in zip(expect, other))      # the two cases differ: stale inputs would show
    case = PREPS[what](0, ctx)
    torch.cuda.synchronize()
    stream = torch.cuda.default_stream() if how == "default" else torch.cuda.Stream()
    if how == "direct":
        ctx.set_stream(stream.cuda_stream)
    with S.quiet_collector(), torch.cuda.stream(stream):
        first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        first.record()
        for _ in range(BALLAST_FILLS):
            ballast.fill_(1)
        last.record()
        for t, f in zip(case.inputs, case.finals):
            t.copy_(f)
        t0 = time.perf_counter()
        case.call(ctx, direct=(how == "direct"))
        t1 = time.perf_counter()
        drained = last.query()
        got = [t.clone() for t in case.outputs()]
    torch.cuda.synchronize()
    ctx.set_stream(0)
    print("%s %s: queued in %.3f ms on the host, ballast %.3f ms" % (what, how, (t1 - t0) * 1e3, first.elapsed_time(last)))
    assert not drained, "ballast too short (or the call synchronised the host): the stream was idle when the call was queued"
    for k, (g, w) in enumerate(zip(case.norm(got), expect)):
        assert torch.equal(g, w), (what, k)
