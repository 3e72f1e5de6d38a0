"""The image-set rule (csrc/ps_glue.h: check_image_set over csrc/ps_image_rule.h) at the three entry points that take a PsImageSet --
ps_klt_pyramids_build_device, ps_orb_pyramids_build_device, ps_detect_features_device -- case by case from ONE table of bad sets:
every case is PS_ERR_BAD_ARG with a text through ps_last_error and writes nothing; and the size limit of the three create
functions."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fast_ref as F  # noqa: E402
from image_frontend_util import u32, upload_images  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)
ROWS, COLS, CAP = 48, 64, 40


def test_bad_image_sets_are_refused_alike_and_write_nothing():
    import torch
    from putslam_amd import api, device_batch
    from putslam_amd._abi import PsImageSet, detect_params
    ctx = api.Context(0)
    L, h = ctx._L, ctx._h
    good = upload_images([F.SCENES["noise256"](ROWS, COLS), F.SCENES["blocks"](ROWS, COLS)], False)
    other = upload_images([F.SCENES["noise4"](ROWS, COLS)] * 3, False)   # what the bad sets point to: other pixels, room for three frames
    klt = device_batch.KltPyramids(ctx, ROWS, COLS, 1, 2, 7, 3)
    orb = device_batch.OrbPyramids(ctx, ROWS, COLS, 1, 2)
    det = device_batch.FastDetector(ctx, ROWS, COLS, 1, 2)
    prm = detect_params(10, True, 1, 1, CAP)
    xy = torch.from_numpy(np.full((2, CAP, 2), SENT_F, np.uint32).view(np.float32)).to("cuda:0")
    resp = torch.from_numpy(np.full((2, CAP), SENT_F, np.uint32).view(np.float32)).to("cuda:0")
    cnt = torch.from_numpy(np.full((2,), SENT_I, np.int32)).to("cuda:0")
    torch.cuda.synchronize()

    def image_set(t=other, frames=2, r=ROWS, c=COLS, cn=1, row_stride=0, frame_stride=0, pixels=True):
        return PsImageSet(t.data_ptr() if pixels else None, row_stride, frame_stride, frames, r, c, cn)

    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    entries = {
        "ps_klt_pyramids_build_device": lambda s, first=0: L.ps_klt_pyramids_build_device(h, klt.handle, ref(s), first),
        "ps_orb_pyramids_build_device": lambda s, first=0: L.ps_orb_pyramids_build_device(h, orb.handle, ref(s), first),
        "ps_detect_features_device": lambda s: L.ps_detect_features_device(h, det.handle, ref(s), C.byref(prm), CAP, ptr(xy), ptr(resp), ptr(cnt)),
    }
    builds = ("ps_klt_pyramids_build_device", "ps_orb_pyramids_build_device")

    def stored():
        torch.cuda.synchronize()
        return klt.level(0, 0)[0].tobytes(), orb.planes(0, 0)[0].tobytes()

    # a good build first: what level 0 of slot 0 holds from here on
    for name in builds:
        assert entries[name](image_set(good)) == 0, name
    before = stored()
    assert np.frombuffer(before[1], np.uint8).tolist() == good[0].cpu().numpy().reshape(-1).tolist()   # (ORB's level 0 is the grey image)

    bad_sets = [
        ("a null set", None),
        ("null pixels", image_set(pixels=False)),
        ("-1 frames", image_set(frames=-1)),
        ("three frames", image_set(frames=3)),
        ("rows 47", image_set(r=ROWS - 1)),
        ("cols 65", image_set(c=COLS + 1)),
        ("channels 3", image_set(cn=3)),
        ("row stride 63", image_set(row_stride=COLS - 1)),
        ("frame stride one below a frame", image_set(frame_stride=ROWS * COLS - 1)),
    ]
    for name, call in entries.items():
        for what, s in bad_sets:
            assert call(s) == -1, (name, what)
            assert len(L.ps_last_error(h)) > 0, (name, what)
    for name in builds:
        for what, first in (("two frames from slot 1", 1), ("first slot -1", -1)):
            assert entries[name](image_set(), first) == -1, (name, what)
            assert len(L.ps_last_error(h)) > 0, (name, what)
    for name, call in entries.items():   # no frames: PS_OK, and nothing to do
        assert call(image_set(frames=0)) == 0, name

    # nothing was written
    assert stored() == before
    assert (u32(xy.cpu().numpy()) == SENT_F).all() and (u32(resp.cpu().numpy()) == SENT_F).all() and (cnt.cpu().numpy() == SENT_I).all()
    # ... and the same good calls work once more
    for name in builds:
        assert entries[name](image_set(good)) == 0, name
    assert stored() == before
    assert entries["ps_detect_features_device"](image_set(good)) == 0
    torch.cuda.synchronize()
    want = [len(F.detect_closed(img, 10, True, 1, 1, CAP)[1]) for img in good.cpu().numpy()]
    assert cnt.cpu().numpy().tolist() == want and max(want) > 0

    # the size limit of the three create functions: PS_ERR_UNSUPPORTED, *out = NULL
    from putslam_amd._abi import orb_params
    creates = {
        "ps_klt_pyramids_create": lambda out: L.ps_klt_pyramids_create(h, 8193, COLS, 1, 7, 3, 2, C.byref(out)),
        "ps_orb_pyramids_create": lambda out: L.ps_orb_pyramids_create(h, 8193, COLS, 1, C.byref(orb_params()), None, 2, C.byref(out)),
        "ps_fast_detector_create": lambda out: L.ps_fast_detector_create(h, 8193, COLS, 1, 2, C.byref(out)),
    }
    for name, create in creates.items():
        out = C.c_void_p(0x55)
        assert create(out) == -5 and not out.value, name
        assert len(L.ps_last_error(h)) > 0, name
    for own in (klt, orb, det):
        own.close()
