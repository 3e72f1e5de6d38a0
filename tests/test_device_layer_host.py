"""Host half of the Python device layer (no GPU, no torch device): the one conversion of each pointer holder of api.py to its
ctypes struct, the table of ABI structs, the single repeat with the reported capacity and the packed frame layout."""
import ctypes as C

import numpy as np
import pytest

from putslam_amd import _lib, api
from putslam_amd._abi import PsFrameSet, PsMapBatch, PsPairResults

FRAME_FIELDS = ("desc", "pts", "nkpts", "numFrames", "maxKpts", "descFrameStride", "ptsFrameStride")


def _fields(s):
    return tuple(getattr(s, n) for n, _ in s._fields_)


@pytest.mark.parametrize("strides", [(), (4096, 4112)], ids=["dense", "strided"])
def test_device_frames_struct(strides):
    fs = api.DeviceFrames(0x1000, 0x2000, 0x3000, 7, 93, *strides).struct()
    assert isinstance(fs, PsFrameSet) and tuple(n for n, _ in fs._fields_) == FRAME_FIELDS
    assert _fields(fs) == (0x1000, 0x2000, 0x3000, 7, 93) + (strides or (0, 0))


def test_device_frames_struct_null_pointer():
    assert _fields(api.DeviceFrames(None, 0, 0x3000, 1, 64).struct()) == (None, None, 0x3000, 1, 64, 0, 0)


def test_device_results_struct():
    r = api.DeviceResults(0x10, 0x20, 0x30, 0x40, 0x50).struct()
    assert isinstance(r, PsPairResults)
    assert tuple(n for n, _ in r._fields_) == ("matches", "numMatches", "inlierMask", "pose", "stats")
    assert _fields(r) == (0x10, 0x20, 0x30, 0x40, 0x50)
    assert _fields(api.DeviceResults(0x10, None, 0, 0x40, 0x50).struct()) == (0x10, None, None, 0x40, 0x50)


@pytest.mark.parametrize("per_pair", [False, True], ids=["scalar", "per_pair"])
def test_device_map_batch_struct(per_pair):
    maps = api.DeviceFrames(0x1000, 0x2000, 0x3000, 6, 700)
    frames = api.DeviceFrames(0x8000, 0x8000 + 512 * 32, 0x9000, 8, 512, 22528, 22528)
    f32 = float(np.float32(0.0144))
    tail = (0.0, 0.0, 0xA000, 0xB000) if per_pair else (f32, 0.55)
    b = api.DeviceMapBatch(maps, 0x4000, frames, 0x5000, 0x6000, 64, 2800, *tail)
    mb = b.struct()
    assert isinstance(mb, PsMapBatch)
    assert _fields(mb.maps) == (0x1000, 0x2000, 0x3000, 6, 700, 0, 0)
    assert _fields(mb.frames) == (0x8000, 0x8000 + 512 * 32, 0x9000, 8, 512, 22528, 22528)
    assert (mb.mapLevel, mb.curLevel, mb.pairs, mb.P, mb.maxMatches) == (0x4000, 0x5000, 0x6000, 64, 2800)
    if per_pair:
        assert (mb.radiusBound, mb.acceptRatio, mb.radiusBoundPerPair, mb.acceptRatioPerPair) == (0.0, 0.0, 0xA000, 0xB000)
    else:
        assert (mb.radiusBound, mb.acceptRatio, mb.radiusBoundPerPair, mb.acceptRatioPerPair) == (f32, 0.55, None, None)
    # the same bytes as a struct filled field by field (padding included)
    want = PsMapBatch()
    for dst, f in ((want.maps, maps), (want.frames, frames)):
        dst.desc, dst.pts, dst.nkpts, dst.numFrames, dst.maxKpts = f.desc_ptr, f.pts_ptr, f.nkpts_ptr, f.num_frames, f.max_kpts
        dst.descFrameStride, dst.ptsFrameStride = f.desc_stride, f.pts_stride
    want.mapLevel, want.curLevel, want.pairs, want.P, want.maxMatches = 0x4000, 0x5000, 0x6000, 64, 2800
    want.radiusBound, want.acceptRatio = b.radius_bound, b.accept_ratio
    want.radiusBoundPerPair, want.acceptRatioPerPair = b.radius_bound_per_pair_ptr, b.accept_ratio_per_pair_ptr
    assert bytes(mb) == bytes(want)


def test_struct_sizes_come_from_the_one_table():
    sizes = _lib.struct_sizes()
    assert set(sizes) == set(_lib.ABI_STRUCTS) and len(sizes) == 16
    for name, cls in _lib.ABI_STRUCTS.items():
        assert issubclass(cls, C.Structure) and sizes[name] == C.sizeof(cls), name
        assert "ps_abi_sizeof_" + name in _lib.EXPORTED, name


class _Runs:
    """run(cap) of the retry helper: reports `needs` in turn, records the capacities it was called with."""

    def __init__(self, *needs):
        self.needs, self.caps = list(needs), []

    def __call__(self, cap):
        self.caps.append(cap)
        return "result at %d" % cap, self.needs[len(self.caps) - 1]


def test_retry_runs_once_when_nothing_overflows():
    for need in (0, 7, 100):
        run = _Runs(need)
        assert api.retry_with_reported_capacity(run, 100) == ("result at 100", 100) and run.caps == [100]


def test_retry_repeats_once_with_the_reported_need():
    run = _Runs(260, 260)
    assert api.retry_with_reported_capacity(run, 100) == ("result at 260", 260) and run.caps == [100, 260]


def test_retry_never_runs_a_third_time():
    run = _Runs(260, 900, 2000)
    assert api.retry_with_reported_capacity(run, 100) == ("result at 260", 260) and run.caps == [100, 260]


def test_retry_respects_its_limit():
    run = _Runs(50000, 50000)
    assert api.retry_with_reported_capacity(run, 1024, limit=16384) == ("result at 16384", 16384) and run.caps == [1024, 16384]
    run = _Runs(50000)      # already at the limit: nothing to gain from a repeat
    assert api.retry_with_reported_capacity(run, 16384, limit=16384) == ("result at 16384", 16384) and run.caps == [16384]


def test_pack_and_unpack_frames_are_inverses():
    from putslam_amd.device_batch import pack_frames, unpack_frames
    rng = np.random.default_rng(5)
    F, cap, stride = 3, 5, 5 * 44 + 36
    desc = rng.integers(0, 256, (F, cap, 32), dtype=np.uint8)
    pts = rng.normal(0.0, 2.0, (F, cap, 3)).astype(np.float32)
    blocks = pack_frames(desc, pts, stride)
    assert blocks.shape == (F, stride) and blocks.dtype == np.uint8 and not blocks[:, cap * 44:].any()
    d, p = unpack_frames(blocks, cap)
    assert d.dtype == np.uint8 and p.dtype == np.float32 and d.shape == desc.shape and p.shape == pts.shape
    assert d.tobytes() == desc.tobytes() and p.tobytes() == pts.tobytes()
    assert pack_frames(d, p, stride).tobytes() == blocks.tobytes()
    assert pack_frames(desc, pts).shape == (F, 224)         # the default stride: cap x 44 rounded up to 16
    d, p = unpack_frames(pack_frames(desc, pts), cap)
    assert d.tobytes() == desc.tobytes() and p.tobytes() == pts.tobytes()


def test_depth_view_bytes_is_where_the_last_row_ends():
    """ps_depth_view_bytes (csrc/ps_glue.h: depth_view_bytes) -- what ps_keypoints2Dto3D copies from the host and what its
    kernel may read: (rows - 1) x depthStep + cols x 2, not rows x depthStep.  Against numpy's own account of a view: the
    distance from its first byte to the byte behind its last pixel."""
    f = _lib.load().ps_depth_view_bytes
    assert f(480, 640, 1280) == 480 * 1280                      # dense: the whole image
    assert f(480, 560, 1280) == 479 * 1280 + 1120               # pitched: 160 bytes short of rows x depthStep
    assert f(1, 1, 2) == 2 and f(1, 1, 4096) == 2               # 1 x 1, whatever the pitch
    assert f(1, 40, 80) == 80 and f(1, 40, 1280) == 80          # rows = 1: the pitch does not matter
    assert f(40, 1, 2) == 80 and f(40, 1, 1280) == 39 * 1280 + 2
    full = np.zeros((480, 640), np.uint16)
    for view in (full, full[:, 40:600], full[10:400, :], full[5:, 600:], full[7:8, 9:10], full[3:4, 10:50], full[20:60, 17:18]):
        rows, cols = view.shape
        first = view.__array_interface__["data"][0]
        behind_last = view[rows - 1:, cols - 1:].__array_interface__["data"][0] + 2
        assert f(rows, cols, view.strides[0]) == behind_last - first
        assert first + f(rows, cols, view.strides[0]) <= full.__array_interface__["data"][0] + full.nbytes
    assert full[5:, 600:].__array_interface__["data"][0] + 475 * 1280 > full.__array_interface__["data"][0] + full.nbytes  # rows x step was not
    # shapes the call rejects
    assert f(0, 640, 1280) == 0 and f(480, 0, 1280) == 0 and f(-1, 5, 10) == 0 and f(480, 640, 1279) == 0
    assert f(2, 0x7fffffff, 2 * 0x7fffffff) == 2 * 2 * 0x7fffffff     # no 32-bit arithmetic


def test_host_image_keeps_a_usable_image_and_copies_the_rest():
    """api._host_image, the one conversion of a numpy image for the host forms of the image front end: uint8 with dense rows any
    stride apart is used where it lies, anything else comes back as a dense uint8 copy of equal values."""
    rng = np.random.default_rng(9)
    grey = rng.integers(0, 256, (60, 80), dtype=np.uint8)
    colour = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    for a, cn in ((grey, 1), (colour, 3)):
        got, n = api._host_image(a)
        assert n == cn and got is a and np.shares_memory(got, a) and got.strides == a.strides
    for parent, cn in ((grey, 1), (colour, 3)):     # a region of a larger image: no copy, the parent's row stride
        region = parent[2:50, 5:69]
        got, n = api._host_image(region)
        assert n == cn and np.shares_memory(got, parent) and got.shape == region.shape and got.strides[0] == parent.strides[0] == 80 * cn
        assert got.__array_interface__["data"][0] == region.__array_interface__["data"][0]
    flt = rng.uniform(0.0, 255.0, (60, 80)).astype(np.float32)
    for what, a in (("column-strided", grey[:, ::2]), ("transposed", grey.T), ("row-reversed", grey[::-1]), ("float", flt),
                    ("column-strided colour", colour[:, ::2]), ("row-reversed colour", colour[::-1])):
        got, n = api._host_image(a)
        assert n == (1 if a.ndim == 2 else 3) and got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and got.shape == a.shape, what
        assert not np.shares_memory(got, a) and np.array_equal(got, a.astype(np.uint8)), what
