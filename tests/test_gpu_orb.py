"""ORB description on the GPU (ps_orb.h): the raw and blurred planes of every level, ps_describe_features_device, the host form
ps_describe_features and the Python wrappers equal the restatements (tests/orb_ref.py) byte for byte -- rows, kept indices and
counts, with sentinel-filled outputs checked beyond every count -- and the chain detect -> describe -> match equals the
restatements chained."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orb_ref as R  # noqa: E402
from image_frontend_util import upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_B = 0x5A
SENT_I = np.int32(-0x5A5A5A5B)
ROWS, COLS, NL, CAP = 80, 96, 8, 257


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.mark.parametrize("rows,cols", [(9, 13), (37, 53), (63, 64), (80, 96)])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("padded", [False, True])
def test_planes_equal_the_restatement(ctx, rows, cols, cn, padded):
    """five scenes, three frames a call into slots 1 .. 3 of five; also scaleFactor 1.5 with 6 levels"""
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import orb_params
    imgs = [R.scene(name, rows, cols, cn, seed=i) for i, name in enumerate(R.SCENES)]
    for sf, nl, calls in ((1.2, 8, (imgs[0:3], imgs[2:5])), (1.5, 6, (imgs[0:3],))):
        pyr = device_batch.OrbPyramids(ctx, rows, cols, cn, 5, orb_params(sf, nl))
        geo = R.level_geometry(rows, cols, sf, nl)
        for l, (r, c, scale) in enumerate(geo):
            (gr, gc), gs = pyr.level(l)
            assert (gr, gc) == (r, c) and np.float32(gs).tobytes() == np.float32(scale).tobytes(), (l, gr, gc, gs)
        with pytest.raises(ValueError):
            pyr.level(nl)
        for batch in calls:
            pyr.build(upload_images(batch, padded), first_slot=1)
            torch.cuda.synchronize()
            for f, img in enumerate(batch):
                want = R.pyramid(img, sf, nl)
                for l in range(nl):
                    raw, blr = pyr.planes(1 + f, l)
                    assert raw.tobytes() == want[l][0].tobytes(), ("raw", sf, f, l)
                    assert blr.tobytes() == want[l][1].tobytes(), ("blurred", sf, f, l)
        pyr.close()


@functools.lru_cache(maxsize=None)
def slot_images():
    return tuple(R.texture(ROWS, COLS, 3 + s) for s in range(3))


@functools.lru_cache(maxsize=None)
def slot_pyramids():
    return tuple(R.pyramid(img, 1.2, NL) for img in slot_images())


def row_frames():
    """[(slot, count, xy, angle, octave)]: the counts 0, 1, 63, 64, 65, 257, the named edge cases, a count of -1 and one above the
    capacity, slots outside the set, one slot named by two frames, an all-zero octave list"""
    frames = []
    for k, (n, slot) in enumerate(((0, 0), (1, 1), (63, 2), (64, 2), (65, 1), (257, 0))):
        frames.append((slot, n) + R.random_keypoints(n, ROWS, COLS, NL, seed=20 + k))
    frames.append((1, None) + R.edge_keypoints(ROWS, COLS, NL))
    frames.append((0, -1) + R.random_keypoints(9, ROWS, COLS, NL, seed=40))
    frames.append((1, CAP + 1) + R.random_keypoints(9, ROWS, COLS, NL, seed=41))
    frames.append((3, 9) + R.random_keypoints(9, ROWS, COLS, NL, seed=42))
    frames.append((-1, 9) + R.random_keypoints(9, ROWS, COLS, NL, seed=43))
    xy, ang, _ = R.random_keypoints(70, ROWS, COLS, NL, seed=44)
    frames.append((2, 70, xy, ang, np.zeros(70, np.int32)))
    return [(s, len(o) if n is None else n, xy, a, o) for s, n, xy, a, o in frames]


def pack(frames):
    F = len(frames)
    xy, ang, octv = np.zeros((F, CAP, 2), np.float32), np.zeros((F, CAP), np.float32), np.zeros((F, CAP), np.int32)
    for f, (_, _, x, a, o) in enumerate(frames):
        xy[f, :len(o)], ang[f, :len(o)], octv[f, :len(o)] = x, a, o
    slots = np.array([fr[0] for fr in frames], np.int32)
    counts = np.array([fr[1] for fr in frames], np.int32)
    return slots, xy, ang, octv, counts


def check_frames(frames, desc, kept, num, pattern):
    pyrs = slot_pyramids()
    for f, (slot, n, xy, ang, octv) in enumerate(frames):
        if n < 0 or n > CAP:
            want_n, wd, wk = -1, np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
        elif not 0 <= slot < 3:
            want_n, wd, wk = 0, np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
        else:
            wd, wk = R.describe(pyrs[slot], xy[:n], ang[:n], octv[:n], pattern)
            want_n = len(wk)
        assert int(num[f]) == want_n, (f, int(num[f]), want_n)
        k = max(want_n, 0)
        assert kept[f, :k].tolist() == wk.tolist(), (f, kept[f, :k][:8], wk[:8])
        assert desc[f, :k].tobytes() == wd.tobytes(), (f, np.nonzero((desc[f, :k] != wd).any(axis=1))[0][:8])
        assert (desc[f, k:] == SENT_B).all() and (kept[f, k:] == SENT_I).all(), f


@pytest.mark.parametrize("custom", [False, True])
def test_rows_equal_the_restatement(ctx, custom):
    import torch
    from putslam_amd import device_batch
    pattern = R.corner_pattern() if custom else None
    pyr = device_batch.OrbPyramids(ctx, ROWS, COLS, 1, 3, pattern=pattern)
    pyr.build(upload_images(slot_images(), False))
    frames = row_frames()
    F = len(frames)
    dev = torch.device("cuda:0")
    slots, xy, ang, octv, counts = (torch.from_numpy(a).to(dev) for a in pack(frames))
    desc = torch.full((F, CAP, 32), SENT_B, dtype=torch.uint8, device=dev)
    kept = torch.full((F, CAP), int(SENT_I), dtype=torch.int32, device=dev)
    num = torch.full((F,), int(SENT_I), dtype=torch.int32, device=dev)
    out = device_batch.describe_features_batch(ctx, pyr, slots, xy, ang, octv, counts, desc, kept, num)
    torch.cuda.synchronize()
    assert out[0] is desc and out[1] is kept and out[2] is num
    check_frames(frames, desc.cpu().numpy(), kept.cpu().numpy(), num.cpu().numpy(), pattern)
    if custom:   # a pair of equal points: its bit is 0 in every row
        d = desc.cpu().numpy()
        for f, n in enumerate(num.cpu().numpy()):
            assert not (d[f, :max(int(n), 0), 0] & 2).any()
    pyr.close()


def test_restatement_meets_its_conditions_on_these_inputs():
    """some samples fall outside their level, none more than 32 px, and the random rows are all different"""
    cnt = R.new_counters()
    slot, n, xy, ang, octv = row_frames()[3]
    desc, kept = R.describe_loops(slot_pyramids()[slot], xy, ang, octv, None, cnt)
    print(cnt)
    assert len(kept) == 64 and cnt["outside"] > 0 and cnt["reach"] <= 32 and len(set(bytes(r) for r in desc)) == 64


def test_small_pyramid_where_samples_bounce_twice(ctx):
    """63 x 64, scaleFactor 1.5, 6 levels: level 5 is 8 x 8, a sample reflects more than once"""
    from putslam_amd._abi import orb_params
    img = R.texture(63, 64, 9)
    xy = np.array([[31, 31], [32.5, 31.5], [32.99, 31.99]] * 6, np.float32)
    angle = np.linspace(0, 350, 18).astype(np.float32)
    octave = np.repeat(np.arange(6), 3).astype(np.int32)[::-1].copy()
    cnt = R.new_counters()
    wd, wk = R.describe_loops(R.pyramid(img, 1.5, 6), xy, angle, octave, None, cnt)
    assert cnt["bounced"] > 0 and len(wk) == 18
    desc, kept = ctx.describe_features(img, xy, angle, octave, orb_params(1.5, 6))
    assert kept.tolist() == wk.tolist() and desc.tobytes() == wd.tobytes()


def test_host_form_and_errors(ctx):
    from putslam_amd import api
    from putslam_amd._abi import orb_params
    imgs = slot_images()
    colour = R.scene("noise", ROWS, COLS, 3, seed=7)
    block = np.full((ROWS, COLS + 7, 3), 0xEE, np.uint8)
    block[:, :COLS] = colour
    for slot, n, xy, ang, octv in row_frames():
        if not (0 <= slot < 3 and 0 <= n <= CAP):
            continue
        for pattern in (None, R.corner_pattern()):
            wd, wk = R.describe(slot_pyramids()[slot], xy, ang, octv, pattern)
            desc, kept = ctx.describe_features(imgs[slot], xy, ang, octv, pattern=pattern)
            assert kept.tolist() == wk.tolist() and desc.tobytes() == wd.tobytes(), (slot, n)
    xy, ang, octv = R.random_keypoints(65, ROWS, COLS, NL, seed=3)
    wd, wk = R.describe(R.pyramid(colour), xy, ang, octv)
    for img in (colour, block[:, :COLS]):   # three channels, dense and with padded rows
        desc, kept = ctx.describe_features(img, xy, ang, octv)
        assert kept.tolist() == wk.tolist() and desc.tobytes() == wd.tobytes()
    # the defaults: angle -1, octave 0
    wd, wk = R.describe(R.pyramid(colour), xy, np.full(65, -1, np.float32), np.zeros(65, np.int32))
    desc, kept = ctx.describe_features(colour, xy)
    assert kept.tolist() == wk.tolist() and desc.tobytes() == wd.tobytes()
    bad = R.default_pattern().copy()
    bad[200, 3] = 16
    for call, code in ((lambda: ctx.describe_features(colour, xy, pattern=bad), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 1, orb_params(), bad, 1), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 1, orb_params(1.0, 8), None, 1), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 1, orb_params(2.5, 8), None, 1), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 1, orb_params(1.2, 9), None, 1), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 1, orb_params(1.2, 0), None, 1), -1),
                       (lambda: ctx.orb_pyramids_create(ROWS, COLS, 2, orb_params(), None, 1), -1),
                       (lambda: ctx.orb_pyramids_create(1, 2, 1, orb_params(2.0, 3), None, 1), -1),        # an empty level
                       (lambda: ctx.orb_pyramids_create(ROWS, 8193, 1, orb_params(), None, 1), -5),
                       (lambda: ctx.describe_features(np.zeros((ROWS, COLS), np.uint8), np.zeros((16385, 2), np.float32)), -5)):
        with pytest.raises(api.PsError) as e:
            call()
        assert e.value.code == code, (e.value, code)
    p = orb_params()
    p.reserved[1] = 1
    with pytest.raises(api.PsError):
        ctx.orb_pyramids_create(ROWS, COLS, 1, p, None, 1)


def test_capacity_above_the_limit_is_unsupported(ctx):
    import ctypes as C
    from putslam_amd import device_batch
    pyr = device_batch.OrbPyramids(ctx, ROWS, COLS, 1, 1)
    one = C.c_void_p(16)   # (never dereferenced: the call is refused first)
    rc = ctx._L.ps_describe_features_device(ctx._h, pyr.handle, one, one, one, one, one, 1, 16385, one, one, one)
    assert rc == -5
    pyr.close()


def test_chain_detect_describe_match(ctx):
    """detect_features_batch -> describe_features_batch -> ps_match_hamming256 on a frame and its copy shifted by 2 px equals the
    restatements chained (tests/fast_ref.py, tests/orb_ref.py, the oracle's matcher); most matches pair a key point with its
    shifted self -- the share the restatements reach, minus nothing."""
    import torch
    import fast_ref as F
    from oracle import oracle_py as po
    from putslam_amd import device_batch
    from putslam_amd._abi import detect_params
    rows, cols, cap = 128, 160, 300
    base = R.texture(rows, cols + 2, 11)
    imgs = [np.ascontiguousarray(base[:, 2:]), np.ascontiguousarray(base[:, :-2])]   # (x, y) of the first is (x + 2, y) of the second
    p = detect_params(20, True, 2, 2, cap)
    dev = torch.device("cuda:0")
    t = upload_images(imgs, False)
    det = device_batch.FastDetector(ctx, rows, cols, 1, 2)
    pyr = device_batch.OrbPyramids(ctx, rows, cols, 1, 2)
    xy, _, counts = device_batch.detect_features_batch(ctx, det, t, p, cap)
    pyr.build(t)
    angle = torch.full((2, cap), -1.0, dtype=torch.float32, device=dev)   # what the FAST detector leaves
    octave = torch.zeros((2, cap), dtype=torch.int32, device=dev)
    slots = torch.arange(2, dtype=torch.int32, device=dev)
    desc, kept, num = device_batch.describe_features_batch(ctx, pyr, slots, xy, angle, octave, counts)
    torch.cuda.synchronize()
    desc, kept, num, xy = desc.cpu().numpy(), kept.cpu().numpy(), num.cpu().numpy(), xy.cpu().numpy()
    want = []
    for f, img in enumerate(imgs):
        wxy, _ = F.detect_closed(img, 20, True, 2, 2, cap)
        wd, wk = R.describe(R.pyramid(img), wxy, np.full(len(wxy), -1, np.float32), np.zeros(len(wxy), np.int32))
        assert int(num[f]) == len(wk) and kept[f, :len(wk)].tolist() == wk.tolist() and desc[f, :len(wk)].tobytes() == wd.tobytes()
        want.append((wxy[wk], wd))
    got = ctx.match_hamming256(np.ascontiguousarray(desc[0, :num[0]]), np.ascontiguousarray(desc[1, :num[1]]))
    ref = po.match_hamming256(want[0][1], want[1][1])
    assert got.tobytes() == ref.tobytes() and len(ref) > 20

    def share(m, a, b):
        return float(np.mean((b[m["trainIdx"]] == a[m["queryIdx"]] + np.float32([2, 0])).all(axis=1)))
    s_ref = share(ref, want[0][0], want[1][0])
    s_got = share(got, xy[0][kept[0, :num[0]]], xy[1][kept[1, :num[1]]])
    print("matches %d, shifted-self share: restatement %.3f, device %.3f" % (len(ref), s_ref, s_got))
    assert s_ref > 0.5 and s_got >= s_ref
    det.close()
    pyr.close()
