"""What the GPU tests of the tracking VO step share: uploads, sentinels, word-wise comparison, and the scene of
tests/track_vo_ref.py on the device."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import track_vo_ref as R  # noqa: E402

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)
SENT_D = np.uint64(0x7FF5A5A5A5A5A5A5)
SENT_B = np.uint8(0xA5)
PAD = 0xEEEE                     # what the padding of a depth block holds: 61166 / 5000 = 12.2 m, a depth no frame has
_FILL = {np.dtype(np.float32): SENT_F, np.dtype(np.int32): SENT_I, np.dtype(np.float64): SENT_D, np.dtype(np.uint8): SENT_B}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, got[:4], want[:4])
        got, want = got[~nan], want[~nan]
    assert got.tobytes() == want.tobytes(), (what, got[:6], want[:6])


def fill_sentinel(t):
    """the device tensor t filled with its type's sentinel, in place"""
    import torch
    a = np.zeros(tuple(t.shape), {torch.float32: np.float32, torch.int32: np.int32, torch.float64: np.float64, torch.uint8: np.uint8}[t.dtype])
    w = words(a)
    w[...] = _FILL[a.dtype]
    t.copy_(torch.from_numpy(w.view(a.dtype)))
    return t


def untouched(a):
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return bool((words(a) == _FILL[a.dtype]).all())


def same_stats(a, b, what):
    for f in a.dtype.names:
        x, y = a[f], b[f]
        assert x == y or (np.isnan(x) and np.isnan(y)), (what, f, a, b)


def depth_block(deps):
    """The depth frames in one block whose rows (7 pixels) and frames (2 rows and 3 pixels) are padded with PAD.  Returns the
    (F, ROWS, COLS) device view."""
    import torch
    rows, cols = deps[0].shape
    row, frame = cols + 7, (rows + 2) * (cols + 7) + 3
    flat = np.full(len(deps) * frame, PAD, np.uint16)
    for f, d in enumerate(deps):
        flat[f * frame:f * frame + rows * row].reshape(rows, row)[:, :cols] = d
    return torch.as_strided(dev(flat.view(np.int16)), (len(deps), rows, cols), (frame, row, 1))


def device_scene(ctx, cn):
    """(KltPyramids of the scene's five frames, the padded depth view)"""
    from putslam_amd import device_batch as db
    imgs = np.stack(R.images(cn))
    pyr = db.KltPyramids(ctx, R.ROWS, R.COLS, cn, len(imgs), R.WIN, R.LEVELS)
    pyr.build(dev(imgs if cn == 3 else imgs[..., 0]))
    return pyr, depth_block(R.depths())


def rows_to_device(rows_list, cap, carried=R.CARRIED):
    """A TrackedRows of the pairs' previous rows (dicts of tests/track_vo_ref.first_rows), sentinel beyond every count"""
    from putslam_amd import device_batch as db
    P = len(rows_list)
    t = db.TrackedRows(P, cap, "cuda:0", carried)
    for name in ("xy", "pts") + tuple(carried):
        fill_sentinel(getattr(t, name))
    counts = np.zeros(P, np.int32)
    for p, r in enumerate(rows_list):
        n = len(r["xy"])
        counts[p] = n
        for name in ("xy", "pts") + tuple(carried):
            getattr(t, name)[p, :n] = dev(r[name])
    t.counts.copy_(dev(counts))
    return t
