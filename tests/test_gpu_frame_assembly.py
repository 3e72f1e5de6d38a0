"""Frame assembly on the GPU (ps_frame_assembly.h): ps_gather_keypoints against a numpy gather, ps_assemble_frames against the oracle's
remove_image_distortion + keypoints2Dto3D and the numpy statement of the detection distance, ps_front_end_frames and its host form
against the reference chain (tests/frame_assembly_ref.py), and ps_vo_pairs_device on what the front end wrote against the oracle's
match + RANSAC on the reference chain's arrays.  Everything is compared byte for byte -- floats as uint32 words; where the expected
float is a NaN the device's is a NaN too (payloads are not part of the contract, as in test_gpu_standalone_geometry.py) -- and
sentinel-filled outputs are checked beyond every count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import frame_assembly_ref as A  # noqa: E402
from image_frontend_util import upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)
SENT_D = np.uint64(0x7FF5A5A5A5A5A5A5)
SENT_B = np.uint8(0xA5)
PAD = 0xEEEE                     # what the padding of a depth block holds: 61166 / 5000 = 12.2 m, a depth no frame has
SIDE = ("xy", "xy_undist", "angle", "response", "octave", "src_idx", "det_dist")


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, got[:4], want[:4])
        got, want = got[~nan], want[~nan]
    assert got.tobytes() == want.tobytes(), (what, got[:6], want[:6])


def sentinel(shape, dtype):
    fill = {np.float32: SENT_F, np.int32: SENT_I, np.float64: SENT_D, np.uint8: SENT_B}[dtype]
    return dev(np.full(shape, fill, words(np.zeros(1, dtype)).dtype).view(dtype))


def untouched(t):
    a = t if isinstance(t, np.ndarray) else t.cpu().numpy()
    fill = {np.dtype(np.float32): SENT_F, np.dtype(np.int32): SENT_I, np.dtype(np.float64): SENT_D, np.dtype(np.uint8): SENT_B}[a.dtype]
    return bool((words(a) == fill).all())


STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers", "accepted",
               "bestInlierRatio", "pointInlierRatio")


def same_pairs(got, want):
    """The device's pair results equal the oracle's: matches, masks, every field of the statistics, the poses."""
    assert got["numMatches"].tolist() == want["numMatches"].tolist()
    for q, m in enumerate(want["numMatches"].tolist()):
        assert got["matches"][q, :m].tobytes() == want["matches"][q, :m].tobytes(), q
        assert got["inlierMask"][q, :m].tobytes() == want["inlierMask"][q, :m].tobytes(), q
        for f in STAT_FIELDS:
            a, b = got["stats"][q][f], want["stats"][q][f]
            assert a == b or (np.isnan(a) and np.isnan(b)), (q, f, a, b)
    assert got["pose"].tobytes() == want["pose"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- gather
GATHER_CAP = 300   # two blocks of 256 rows
GATHER_COUNTS = [0, 1, 63, 64, 65, GATHER_CAP, -1, GATHER_CAP + 1]


def gather_inputs(seed=5):
    rng = np.random.RandomState(seed)
    F, cap = len(GATHER_COUNTS), GATHER_CAP
    xy = rng.rand(F, cap, 2).astype(np.float32) * 200
    resp, ang = rng.randn(F, cap).astype(np.float32), (rng.rand(F, cap) * 360).astype(np.float32)
    octv = rng.randint(0, 8, size=(F, cap)).astype(np.int32)
    idx = np.stack([rng.permutation(cap) for _ in range(F)]).astype(np.int32)
    idx[4, 2], idx[4, 5], idx[5, 299], idx[5, 0] = cap, -1, 2 ** 31 - 1, -2 ** 31        # indices outside 0 .. cap-1
    return idx, np.array(GATHER_COUNTS, np.int32), xy, resp, ang, octv


def gather_expected(idx, nidx, arrays, cap):
    """(rows per frame, counts): row j of frame f is arrays[f][idx[f][j]], zeros where the index lies outside"""
    out, counts = [], []
    for f, n in enumerate(nidx.tolist()):
        if not 0 <= n <= cap:
            counts.append(-1)
            out.append(None)
            continue
        counts.append(n)
        i = idx[f, :n].astype(np.int64)
        ok = (i >= 0) & (i < cap)
        rows = []
        for a in arrays:
            r = a[f][np.where(ok, i, 0)].copy()
            r[~ok] = 0
            rows.append(r)
        out.append(rows)
    return out, counts


@pytest.mark.parametrize("optional", ["all", "none", "octave_only"])
def test_gather_equals_numpy(ctx, optional):
    """Counts 0, 1, 63, 64, 65 and the capacity (two blocks); -1 and capacity + 1 give -1 and write nothing; indices of capacity, -1,
    INT_MAX and INT_MIN give zero rows; rows beyond a count keep the sentinel; each optional pair may be absent."""
    import torch
    idx, nidx, xy, resp, ang, octv = gather_inputs()
    F, cap = xy.shape[:2]
    want_resp, want_ang, want_oct = optional == "all", optional == "all", optional != "none"
    ins = [dev(xy), dev(resp) if want_resp else None, dev(ang) if want_ang else None, dev(octv) if want_oct else None]
    outs = [sentinel((F, cap, 2), np.float32), sentinel((F, cap), np.float32) if want_resp else None,
            sentinel((F, cap), np.float32) if want_ang else None, sentinel((F, cap), np.int32) if want_oct else None]
    counts = sentinel((F,), np.int32)
    di, dn = dev(idx), dev(nidx)
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    torch.cuda.synchronize()
    ctx.gather_keypoints(di.data_ptr(), dn.data_ptr(), F, cap, *[ptr(t) for t in ins], *[ptr(t) for t in outs], counts.data_ptr())
    ctx.synchronize()
    host = [a for a, t in zip([xy, resp, ang, octv], ins) if t is not None]
    got = [t.cpu().numpy() for t in outs if t is not None]
    want, wcounts = gather_expected(idx, nidx, host, cap)
    assert counts.cpu().numpy().tolist() == wcounts
    for f in range(F):
        n = max(wcounts[f], 0)
        for g, k in zip(got, range(len(got))):
            if want[f] is not None:
                same_bits(g[f, :n], want[f][k], (f, k))
            assert untouched(g[f, n:]), (f, k)
    # the zero rows are there
    assert (got[0][4, 2] == 0).all() and (got[0][4, 5] == 0).all() and (got[0][5, 299] == 0).all() and (got[0][5, 0] == 0).all()


def test_gather_wrapper_equals_torch_gather(ctx):
    """device_batch.gather_keypoints = the torch.gather the chain used before, on valid indices."""
    import torch
    from putslam_amd import device_batch
    idx, nidx, xy, resp, ang, octv = gather_inputs(9)
    idx = np.stack([np.sort(np.random.RandomState(f).permutation(GATHER_CAP)) for f in range(len(nidx))]).astype(np.int32)
    nidx = np.array([0, 1, 63, 64, 65, GATHER_CAP, 17, 256], np.int32)
    di, dn = dev(idx), dev(nidx)
    gxy, gresp, gang, goct, cnt = device_batch.gather_keypoints(ctx, di, dn, dev(xy), dev(resp), dev(ang), dev(octv))
    torch.cuda.synchronize()
    ix = di.long()
    want = (torch.gather(dev(xy), 1, ix[..., None].expand(-1, -1, 2)), torch.gather(dev(resp), 1, ix), torch.gather(dev(ang), 1, ix),
            torch.gather(dev(octv), 1, ix))
    assert cnt.cpu().numpy().tolist() == nidx.tolist()
    for f, n in enumerate(nidx.tolist()):
        for g, w in zip((gxy, gresp, gang, goct), want):
            same_bits(g[f, :n].cpu().numpy(), w[f, :n].cpu().numpy(), f)
            assert not g[f, n:].cpu().numpy().any(), f     # the wrapper's blocks start zeroed; nothing was written beyond the count


# -------------------------------------------------------------------------------------------------------------- assemble
ROWS, COLS = A.ROWS, A.COLS
ASM_CAP = 300
ASM_COUNTS = [65, ASM_CAP, 64, 0, 1, 63, -1, ASM_CAP + 1]     # frame f reads depth frame f % 3
ZERO_DIST = (0.0,) * 5


def depth_block():
    """Three depth frames in one block whose rows (7 pixels) and frames (2 rows and 3 pixels) are padded with PAD.  Returns (the
    device block as int16 words, the (3, ROWS, COLS) device view, the host views per frame)."""
    import torch
    deps = A.depths()[:3]
    row, frame = COLS + 7, (ROWS + 2) * (COLS + 7) + 3
    flat = np.full(3 * frame, PAD, np.uint16)
    for f, d in enumerate(deps):
        flat[f * frame:f * frame + ROWS * row].reshape(ROWS, row)[:, :COLS] = d
    block = dev(flat.view(np.int16))
    view = torch.as_strided(block, (3, ROWS, COLS), (frame, row, 1))
    return block, view, deps


def distort(uv, K, dist5):
    """The Brown model forwards, in double: where a point must lie in the distorted image to be undistorted to uv."""
    uv = np.asarray(uv, np.float64)
    k1, k2, p1, p2, k3 = dist5
    x, y = (uv[:, 0] - K[2]) / K[0], (uv[:, 1] - K[5]) / K[4]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd, yd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * K[0] + K[2], yd * K[4] + K[5]], 1).astype(np.float32)


def assemble_positions(dist5, seed=11):
    """xy (F, cap, 2): random positions over and around the image, with the named ones in the first rows of every frame.  The first
    four are placed so that they UNDISTORT to the named pixel (the coefficients move a corner point by more than a pixel)."""
    rng = np.random.RandomState(seed)
    F, cap = len(ASM_COUNTS), ASM_CAP
    xy = (rng.rand(F, cap, 2) * [COLS + 20, ROWS + 20] - 10).astype(np.float32)
    edge = distort(np.float32([[COLS - 0.4, 40.0],          # u == cols in an inner row: the next row's first pixel
                               [COLS - 0.4, ROWS - 1.3],    # u == cols in the last row: depth 0
                               [17.0, ROWS - 0.4],          # v == rows: depth 0
                               [COLS - 0.4, ROWS - 0.4]]),  # both
                   A.K, dist5)
    named = np.concatenate([edge, np.float32([[np.nan, 10.0], [10.0, np.nan], [np.inf, 10.0], [10.0, -np.inf], [-np.inf, np.inf], [-3.0, -0.3],
                                              [COLS - 1.0, ROWS - 1.0], [0.0, 0.0], [1e30, 5.0]])])
    xy[:, :len(named)] = named
    return xy, len(named)


def assemble_expected(oracle, xy, kept, counts, deps, dist5, side_in):
    out = []
    for f, n in enumerate(counts):
        if not 0 <= n <= ASM_CAP:
            out.append(None)
            continue
        out.append(A.assemble(oracle, xy[f], kept[f, :n], deps[f % 3], A.K, dist5, A.DEPTH_SCALE, **{k: v[f] for k, v in side_in.items()}))
    return out


@pytest.mark.parametrize("dist5", [ZERO_DIST, A.DIST5], ids=["no_distortion", "tum_fr1"])
def test_assemble_equals_the_oracle(ctx, oracle, dist5):
    """Counts at the block seams; a depth set whose rows and frames are padded; the named positions; -1 and capacity + 1 give a
    count of 0 and write nothing; rows beyond a count keep the sentinel; the padding's depth never appears."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import frame_geometry
    xy, named = assemble_positions(dist5)
    F, cap = xy.shape[:2]
    rng = np.random.RandomState(2)
    kept = np.stack([rng.permutation(cap) for _ in range(F)]).astype(np.int32)
    kept[:, :named] = np.arange(named)       # the named positions are rows of every frame that has that many
    safe = kept.copy()
    kept[1, 290], kept[1, 291] = cap, -1     # indices outside 0 .. cap-1: zero rows
    ang, resp = (rng.rand(F, cap) * 360).astype(np.float32), rng.randn(F, cap).astype(np.float32)
    octv = rng.randint(0, 8, size=(F, cap)).astype(np.int32)
    _, view, deps = depth_block()
    # every frame of the call reads depth frame f % 3: three calls of the frames f = r mod 3 with firstDepthFrame r would need
    # strided inputs, so the set is laid out again with the frames in the call's order
    order = [f % 3 for f in range(F)]
    big = torch.as_strided(dev(np.full(F * (view.stride(0)) + 8, PAD, np.uint16).view(np.int16)), (F, ROWS, COLS), view.stride())
    for f, s in enumerate(order):
        big[f] = view[s]
    geo = frame_geometry(A.K, dist5, A.DEPTH_SCALE)
    out = device_batch.FrameRowsDevice(F, cap, "cuda:0")
    for name in ("pts", "nkpts") + SIDE:
        t = getattr(out, name)
        setattr(out, name, sentinel(tuple(t.shape), {torch.float32: np.float32, torch.int32: np.int32, torch.float64: np.float64}[t.dtype]))
    torch.cuda.synchronize()
    device_batch.assemble_frames(ctx, geo, big, dev(xy), dev(kept), dev(np.array(ASM_COUNTS, np.int32)), dev(ang), dev(resp), dev(octv), out=out)
    torch.cuda.synchronize()
    got = out.download()
    want = assemble_expected(oracle, xy, safe, ASM_COUNTS, deps, dist5, dict(angle=ang, response=resp, octave=octv))
    assert got["nkpts"].tolist() == [n if 0 <= n <= cap else 0 for n in ASM_COUNTS]
    seen_pad = np.float32(PAD / A.DEPTH_SCALE)
    for f, n in enumerate(ASM_COUNTS):
        n = n if 0 <= n <= cap else 0
        for name in ("pts",) + SIDE:
            if n:
                w = want[f][name].copy()
                if f == 1:      # the two indices outside: zero rows (src_idx 0)
                    w[290:292] = 0
                same_bits(got[name][f, :n], w.astype(got[name].dtype), (name, f))
            assert untouched(got[name][f, n:]), (name, f)
        assert not (got["pts"][f, :n, 2] == seen_pad).any(), f
    # the named positions did what their names say (frame 1 holds them all)
    w = want[1]
    und = w["xy_undist"][:4]
    assert [oracle.round_size(u[0], COLS) for u in und] == [COLS, COLS, 17, COLS] and [oracle.round_size(u[1], ROWS) for u in und] == [40, ROWS - 1, ROWS, ROWS]
    assert w["pts"][0, 2] == np.float32(deps[1][41, 0] / A.DEPTH_SCALE) and deps[1][41, 0] != 0      # the next row's first pixel
    assert (w["pts"][1:4, 2] == 0).all() and (w["det_dist"][1:4] == 0).all()
    assert w["pts"][4, 2] == 0 and np.isnan(w["pts"][4, 0]) and w["pts"][5, 2] == 0 and np.isnan(w["pts"][5, 1])
    same_bits(got["det_dist"][1, :cap], A.det_dist(got["pts"][1, :cap]), "det_dist")


def test_assemble_first_depth_frame_and_each_optional_output_absent(ctx, oracle):
    """firstDepthFrame 1 of the padded set of three: frames 0 and 1 of the call read depth frames 1 and 2.  Each optional output
    absent in turn, all absent: the others are what they were."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import frame_geometry
    xy, named = assemble_positions(A.DIST5, 3)
    xy = xy[:2, :64]
    kept = np.stack([np.random.RandomState(f).permutation(64) for f in range(2)]).astype(np.int32)
    counts = np.array([64, 37], np.int32)
    ang, resp = np.random.RandomState(5).rand(2, 64).astype(np.float32), np.random.RandomState(6).rand(2, 64).astype(np.float32)
    octv = np.random.RandomState(7).randint(0, 8, size=(2, 64)).astype(np.int32)
    _, view, deps = depth_block()
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    want = [A.assemble(oracle, xy[f], kept[f, :counts[f]], deps[f + 1], angle=ang[f], response=resp[f], octave=octv[f]) for f in range(2)]
    for absent in [()] + [(s,) for s in SIDE] + [SIDE]:
        side = [s for s in SIDE if s not in absent]
        out = device_batch.assemble_frames(ctx, geo, view, dev(xy), dev(kept), dev(counts), dev(ang), dev(resp), dev(octv), first_depth_frame=1,
                                           side=side)
        torch.cuda.synchronize()
        got = out.download()
        assert sorted(got) == sorted(["desc", "pts", "nkpts"] + side)
        assert got["nkpts"].tolist() == counts.tolist()
        for f in range(2):
            for name in ["pts"] + side:
                same_bits(got[name][f, :counts[f]], want[f][name].astype(got[name].dtype), (absent, name, f))
                assert not got[name][f, counts[f]:].any(), (absent, name, f)


# ----------------------------------------------------------------------------------------------------------------- chain
def fe_params(p, levels):
    from putslam_amd._abi import front_end_params, orb_detect_params, orb_params
    det = orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])
    return front_end_params(det, orb_params(p["scale_factor"], levels), A.DBSCAN_EPS)


def sentinel_rows(F, cap):
    import torch
    from putslam_amd import device_batch
    out = device_batch.FrameRowsDevice(F, cap, "cuda:0")
    kinds = {torch.float32: np.float32, torch.int32: np.int32, torch.float64: np.float64, torch.uint8: np.uint8}
    for name in ("desc", "pts", "nkpts") + SIDE:
        t = getattr(out, name)
        setattr(out, name, sentinel(tuple(t.shape), kinds[t.dtype]))
    torch.cuda.synchronize()
    return out


def assert_chain(got, frames, order, what):
    assert got["nkpts"].tolist() == [len(frames[s]["pts"]) for s in order], what
    for f, s in enumerate(order):
        w, n = frames[s], len(frames[s]["pts"])
        for name in ("desc", "pts") + SIDE:
            same_bits(got[name][f, :n], np.asarray(w[name]).astype(got[name].dtype), (what, name, f))
            assert untouched(got[name][f, n:]), (what, name, f)


@pytest.mark.parametrize("cn", [1, 3], ids=["grey", "colour"])
@pytest.mark.parametrize("case", A.CASES, ids=[c[0] for c in A.CASES])
def test_front_end_equals_the_reference_chain_and_feeds_vo_pairs(ctx, oracle, case, cn):
    """Four frames in, a frame set out: desc, pts, nkpts and every side array equal the reference chain, sentinels beyond every
    count; the same handle on the frames in another order equals it again; ps_vo_pairs_device on the produced arrays equals the
    oracle's match + RANSAC on the reference's arrays for (0, 1), (1, 2), (2, 3) -- the last frame is empty."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import EST_RANSAC, default_ransac_params, frame_geometry, make_config
    name, p, levels = case
    imgs, deps = A.images(cn), A.depths()
    frames, _ = A.chain(oracle, imgs, deps, p, levels)
    fe = device_batch.FrontEnd(ctx, A.ROWS, A.COLS, cn, 4, fe_params(p, levels))
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    dimg = upload_images(imgs, True)
    ddep = dev(np.stack(deps).view(np.int16))
    out = sentinel_rows(4, A.CAPACITY)
    device_batch.front_end_frames_batch(ctx, fe, dimg, ddep, geo, A.CAPACITY, out=out)
    torch.cuda.synchronize()
    assert_chain(out.download(), frames, [0, 1, 2, 3], (name, cn, "first"))
    # the pairs, on the arrays where they lie
    pairs = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    prm = default_ransac_params(0)
    cfg, _ = make_config(EST_RANSAC, 487, 1)
    batch = device_batch.PairBatchDevice(pairs, A.CAPACITY, "cuda:0")
    device_batch.run_pairs(ctx, prm, cfg, A.K, out, batch)
    got = batch.download()
    desc, pts, n = A.frame_set(frames, A.CAPACITY)
    want = oracle.vo_pairs(prm, cfg, A.K, desc, pts, n, pairs)
    same_pairs(got, want)
    assert want["stats"]["accepted"].tolist() == [1, 0, 0] and want["numMatches"][2] == 0
    # another order through the same handle: no state leaks from call to call
    order = [3, 2, 0, 1]
    out2 = sentinel_rows(4, A.CAPACITY)
    device_batch.front_end_frames_batch(ctx, fe, upload_images([imgs[s] for s in order], False), dev(np.stack([deps[s] for s in order]).view(np.int16)),
                                        geo, A.CAPACITY, out=out2)
    torch.cuda.synchronize()
    assert_chain(out2.download(), frames, order, (name, cn, "second"))
    fe.close()


def test_run_image_sequence_is_the_two_calls(ctx, oracle):
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import EST_RANSAC, default_ransac_params, frame_geometry, make_config
    name, p, levels = A.CASES[0]
    imgs, deps = A.images(1), A.depths()
    frames, _ = A.chain(oracle, imgs, deps, p, levels)
    fe = device_batch.FrontEnd(ctx, A.ROWS, A.COLS, 1, 4, fe_params(p, levels))
    cfg, _ = make_config(EST_RANSAC, 487, 1)
    prm = default_ransac_params(0)
    fs, batch = device_batch.run_image_sequence(ctx, fe, upload_images(imgs, False), dev(np.stack(deps).view(np.int16)),
                                                frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE), prm, cfg, A.CAPACITY)
    torch.cuda.synchronize()
    got = batch.download()
    desc, pts, n = A.frame_set(frames, A.CAPACITY)
    want = oracle.vo_pairs(prm, cfg, A.K, desc, pts, n, np.array([[0, 1], [1, 2], [2, 3]], np.int32))
    assert fs.nkpts.cpu().numpy().tolist() == n.tolist()
    same_pairs(got, want)
    fe.close()


def test_host_form_equals_the_device_forms_frame(ctx, oracle):
    """ps_front_end_frame on an image and a depth image that are regions of larger ones = the reference chain's frame, for a frame
    with key points and for the one without; a cap below the rows reports the rows needed and writes nothing."""
    from putslam_amd._abi import PsFrameRowsOut, frame_geometry
    name, p, levels = A.CASES[1]
    imgs, deps = A.images(3), A.depths()
    frames, _ = A.chain(oracle, imgs, deps, p, levels)
    geo, prm = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE), fe_params(p, levels)
    for f in (0, 3):
        parent = np.full((A.ROWS + 4, A.COLS + 9, 3), 0x33, np.uint8)
        parent[2:2 + A.ROWS, 5:5 + A.COLS] = imgs[f]
        dparent = np.full((A.ROWS + 3, A.COLS + 6), PAD, np.uint16)
        dparent[1:1 + A.ROWS, 2:2 + A.COLS] = deps[f]
        got = ctx.front_end_frame(parent[2:2 + A.ROWS, 5:5 + A.COLS], dparent[1:1 + A.ROWS, 2:2 + A.COLS], geo, prm)
        assert len(got["pts"]) == len(frames[f]["pts"])
        for k in ("desc", "pts") + SIDE:
            same_bits(got[k], np.asarray(frames[f][k]).astype(got[k].dtype), (f, k))
    # the capacity it needs
    n = len(frames[0]["pts"])
    L, img, dep = ctx._L, np.ascontiguousarray(imgs[0]), np.ascontiguousarray(deps[0])
    desc, pts = np.full((n, 32), SENT_B, np.uint8), np.full((n, 3), SENT_F, np.uint32)
    out = PsFrameRowsOut(pts.ctypes.data, None, None, None, None, None, None, None, None, None, None, None)
    nout = C.c_int(-7)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    args = (ctx._h, pv(img), pv(dep), A.ROWS, A.COLS, 3, 0, 0, C.byref(prm), None, C.byref(geo), pv(desc), C.byref(out))
    assert L.ps_front_end_frame(*args, n - 1, C.byref(nout)) == -1 and nout.value == n and b"cap" in L.ps_last_error(ctx._h)
    assert (desc == SENT_B).all() and (pts == SENT_F).all()
    assert L.ps_front_end_frame(*args, n, C.byref(nout)) == 0 and nout.value == n
    assert np.array_equal(desc, frames[0]["desc"])
    same_bits(pts.view(np.float32), frames[0]["pts"], "pts")


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_outputs_untouched(ctx):
    """Every refused argument of the three device calls and of create returns its code, leaves a text in ps_last_error and writes
    nothing; zero frames is PS_OK and writes nothing either; then the same arguments, all in order, work."""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import PS_MAX_KPTS, PsDepthSet, PsFrameRowsOut, PsImageSet, frame_geometry
    L, h = ctx._L, ctx._h
    name, p, levels = A.CASES[0]
    prm = fe_params(p, levels)
    fe = device_batch.FrontEnd(ctx, A.ROWS, A.COLS, 1, 2, prm)
    imgs = upload_images(A.images(1)[:2], False)
    deps = dev(np.stack(A.depths()[:2]).view(np.int16))
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    cap = A.CAPACITY
    rows = sentinel_rows(2, cap)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def image_set(frames=2, r=A.ROWS, c=A.COLS, cn=1, row_stride=0, frame_stride=0, pixels=True):
        return PsImageSet(imgs.data_ptr() if pixels else None, row_stride, frame_stride, frames, r, c, cn)

    def depth_set(frames=2, r=A.ROWS, c=A.COLS, row_stride=0, frame_stride=0, pixels=True):
        return PsDepthSet(deps.data_ptr() if pixels else None, row_stride, frame_stride, frames, r, c)

    def rows_out(pts=True, nkpts=True):
        o = rows.out_struct()
        o.pts = o.pts if pts else None
        o.nkpts = o.nkpts if nkpts else None
        return o

    def frames_call(s=None, d=None, g=geo, capacity=cap, desc=rows.desc, o=None, f=fe.handle, null=()):
        s, d, o = s or image_set(), d or depth_set(), o or rows_out()
        ref = lambda x, k: None if k in null else C.byref(x)   # noqa: E731
        return L.ps_front_end_frames(h, f, ref(s, "images"), ref(d, "depth"), ref(g, "geometry"), capacity, ptr(desc), ref(o, "out"))

    bad = [
        ("null handle", lambda: frames_call(f=None)), ("null images", lambda: frames_call(null=("images",))),
        ("null depth", lambda: frames_call(null=("depth",))), ("null geometry", lambda: frames_call(null=("geometry",))),
        ("null out", lambda: frames_call(null=("out",))), ("null desc", lambda: frames_call(desc=None)),
        ("null pts", lambda: frames_call(o=rows_out(pts=False))), ("null nkpts", lambda: frames_call(o=rows_out(nkpts=False))),
        ("null pixels", lambda: frames_call(s=image_set(pixels=False))), ("null depth pixels", lambda: frames_call(d=depth_set(pixels=False))),
        ("other rows", lambda: frames_call(s=image_set(r=A.ROWS - 1))), ("other channels", lambda: frames_call(s=image_set(cn=3))),
        ("other depth rows", lambda: frames_call(d=depth_set(r=A.ROWS - 1))), ("other depth cols", lambda: frames_call(d=depth_set(c=A.COLS + 1))),
        ("image row stride", lambda: frames_call(s=image_set(row_stride=A.COLS - 1))),
        ("image frame stride", lambda: frames_call(s=image_set(frame_stride=A.ROWS * A.COLS - 1))),
        ("depth row stride", lambda: frames_call(d=depth_set(row_stride=A.COLS * 2 - 2))),
        ("odd depth row stride", lambda: frames_call(d=depth_set(row_stride=A.COLS * 2 + 1))),
        ("depth frame stride below a view", lambda: frames_call(d=depth_set(frame_stride=A.ROWS * A.COLS * 2 - 2))),
        ("frames differ", lambda: frames_call(d=depth_set(frames=1))), ("more frames than the handle holds", lambda: frames_call(s=image_set(frames=3), d=depth_set(frames=3))),
        ("negative frames", lambda: frames_call(s=image_set(frames=-1), d=depth_set(frames=-1))),
        ("capacity below what a frame can emit", lambda: frames_call(capacity=cap - 7)),
        ("capacity above the handle's rows", lambda: frames_call(capacity=cap + 1)), ("capacity 0", lambda: frames_call(capacity=0)),
    ]
    for what, run in bad:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    assert frames_call(capacity=8001) == -5 and len(L.ps_last_error(h)) > 0
    assert frames_call(s=image_set(frames=0), d=depth_set(frames=0)) == 0

    # ps_gather_keypoints and ps_assemble_frames on the same blocks
    idx, nidx = dev(np.zeros((2, cap), np.int32)), dev(np.array([3, 3], np.int32))
    xy_in, oct_in = dev(np.ones((2, cap, 2), np.float32)), dev(np.ones((2, cap), np.int32))

    def gather(i=idx, n=nidx, F=2, capacity=cap, x=xy_in, o=oct_in, xo=rows.xy, oo=rows.octave, c=rows.nkpts):
        return L.ps_gather_keypoints(h, ptr(i), ptr(n), F, capacity, ptr(x), None, None, ptr(o), ptr(xo), None, None, ptr(oo), ptr(c))

    for what, run in [("null idx", lambda: gather(i=None)), ("null nidx", lambda: gather(n=None)), ("null xy", lambda: gather(x=None)),
                      ("null xy out", lambda: gather(xo=None)), ("null counts", lambda: gather(c=None)),
                      ("octave in without out", lambda: gather(oo=None)), ("octave out without in", lambda: gather(o=None)),
                      ("negative F", lambda: gather(F=-1)), ("F above 65535", lambda: gather(F=65536)), ("capacity 0", lambda: gather(capacity=0))]:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    assert gather(capacity=PS_MAX_KPTS + 1) == -5
    assert gather(F=0) == 0

    def side_out(**kw):
        o = rows.out_struct(None, None, oct_in)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def assemble(g=geo, d=None, first=0, x=xy_in, k=idx, n=nidx, F=2, capacity=cap, o=None, null=()):
        d, o = d or depth_set(), o or side_out(angle=None, response=None)
        ref = lambda v, key: None if key in null else C.byref(v)   # noqa: E731
        return L.ps_assemble_frames(h, ref(g, "geometry"), ref(d, "depth"), first, ptr(x), ptr(k), ptr(n), F, capacity, ref(o, "out"))

    for what, run in [("null geometry", lambda: assemble(null=("geometry",))), ("null depth", lambda: assemble(null=("depth",))),
                      ("null out", lambda: assemble(null=("out",))), ("null xy", lambda: assemble(x=None)), ("null keptIdx", lambda: assemble(k=None)),
                      ("null numKept", lambda: assemble(n=None)), ("null pts", lambda: assemble(o=side_out(angle=None, response=None, pts=None))),
                      ("null nkpts", lambda: assemble(o=side_out(angle=None, response=None, nkpts=None))),
                      ("angle without its input", lambda: assemble(o=side_out(response=None))),
                      ("response without its input", lambda: assemble(o=side_out(angle=None))),
                      ("octave without its input", lambda: assemble(o=side_out(angle=None, response=None, octaveIn=None))),
                      ("null depth pixels", lambda: assemble(d=depth_set(pixels=False))), ("depth frames outside the set", lambda: assemble(first=1)),
                      ("negative first frame", lambda: assemble(first=-1)), ("depth row stride", lambda: assemble(d=depth_set(row_stride=A.COLS * 2 - 2))),
                      ("depth frame stride below a view", lambda: assemble(d=depth_set(frame_stride=A.ROWS * A.COLS * 2 - 2))),
                      ("depth rows 0", lambda: assemble(d=depth_set(r=0))), ("negative F", lambda: assemble(F=-1)), ("capacity 0", lambda: assemble(capacity=0))]:
        assert run() == -1, what
        assert len(L.ps_last_error(h)) > 0, what
    assert assemble(capacity=PS_MAX_KPTS + 1) == -5
    assert assemble(F=0) == 0

    # create
    def create(r=A.ROWS, c=A.COLS, cn=1, p=prm, frames=1, out=True):
        hd = C.c_void_p(0x55)
        rc = L.ps_front_end_create(h, r, c, cn, C.byref(p) if p is not None else None, None, frames, C.byref(hd) if out else None)
        assert not out or rc == 0 or not hd.value
        if rc == 0:
            L.ps_front_end_destroy(hd)
        return rc

    def with_field(part, name, value):
        q = fe_params(p, levels)
        setattr(getattr(q, part), name, value)
        return q

    for what, run, code in [("null params", lambda: create(p=None), -1), ("null out", lambda: create(out=False), -1), ("rows 0", lambda: create(r=0), -1),
                            ("channels 2", lambda: create(cn=2), -1), ("no frames", lambda: create(frames=0), -1),
                            ("gridRows 0", lambda: create(p=with_field("detect", "gridRows", 0)), -1),
                            ("describe levels 9", lambda: create(p=with_field("describe", "nLevels", 9)), -1),
                            ("describe reserved", lambda: create(p=with_field("detect", "reserved", 1)), -1),
                            ("rows above 8192", lambda: create(r=8193), -5),
                            ("maximum above PS_DBSCAN_MAX_KPTS", lambda: create(p=with_field("detect", "maximalTrackedFeatures", 8001)), -5)]:
        assert run() == code, what
        assert len(L.ps_last_error(h)) > 0, what

    # nothing above wrote anything
    torch.cuda.synchronize()
    for name_ in ("desc", "pts", "nkpts") + SIDE:
        assert untouched(getattr(rows, name_)), name_
    # ... and the same arguments, all in order, work
    assert frames_call() == 0 and gather(xo=dev(np.zeros((2, cap, 2), np.float32)), oo=dev(np.zeros((2, cap), np.int32)), c=dev(np.zeros(2, np.int32))) == 0
    torch.cuda.synchronize()
    assert (rows.nkpts.cpu().numpy() > 0).all()
    assert assemble() == 0
    torch.cuda.synchronize()
    assert rows.nkpts.cpu().numpy().tolist() == [3, 3]
    fe.close()
