"""The sequential C++ restatement of the measurement uncertainty (putslam_amd/csrc/ps_uncertainty_host.h) -- the control of
profiles/scripts/uncertainty_times.py (profiles/scripts/uncertainty_host_loop.cpp) and the arithmetic of the drop-in's
DepthSensorModel -- against the numpy restatement (tests/uncertainty_ref.py), byte for byte, on the scene of the GPU tests.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import test_gpu_uncertainty as T  # noqa: E402  (the scene; nothing of it runs on a GPU here)
import uncertainty_ref as U  # noqa: E402


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("unc") / "uncertainty_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "profiles", "scripts", "uncertainty_host_loop.cpp"),
                           "-o", so])
    return C.CDLL(so).unc_host_edges


def host_edges(fn, model, sensor, deps, imgs, image_frame, pairs, num_maps, matches, num, mask, pts, xyu, max_matches):
    from putslam_amd._abi import frame_geometry, sensor_model
    P, (F, cap) = len(pairs), pts.shape[:2]
    deps, imgs = np.ascontiguousarray(deps), np.ascontiguousarray(imgs)
    out = dict(count=np.zeros(P, np.int32), mapRow=np.zeros((P, max_matches), np.int32), curRow=np.zeros((P, max_matches), np.int32),
               uv=np.zeros((P, max_matches, 2), np.float32), position=np.zeros((P, max_matches, 3)), normal=np.zeros((P, max_matches, 3)),
               gradient=np.zeros((P, max_matches, 3)), info=np.zeros((P, max_matches, 9)))
    pv = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)   # noqa: E731
    geo, sens = frame_geometry(T.K, (0.0,) * 5, T.SCALE), sensor_model(**sensor)
    keep = [np.ascontiguousarray(a) for a in (np.array(image_frame, np.int32), np.array(pairs, np.int32), matches, num, mask, pts, xyu)]
    rows, cols = deps.shape[1:]
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                   C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13
    assert fn(C.byref(geo), C.byref(sens), model, pv(imgs), cols * 3, rows * cols * 3, len(imgs), pv(deps), cols * 2, rows * cols * 2, len(deps), rows,
              cols, pv(keep[0]), pv(keep[1]), P, num_maps, F, cap, max_matches, pv(keep[2]), pv(keep[3]), pv(keep[4]), pv(keep[5]), pv(keep[6]),
              *[pv(out[k]) for k in ("count", "mapRow", "curRow", "uv", "position", "normal", "gradient", "info")]) == 0
    return out


@pytest.mark.parametrize("sensor", ["scaled", "default"])
@pytest.mark.parametrize("model", [-1, 0, 1, 2])
def test_host_loop_equals_the_restatement(loop, model, sensor):
    """Every pixel of the three frames and the named positions as the current rows of three pairs whose every match is an inlier,
    then lists with holes, an overflowed pair and a pair outside the set"""
    from putslam_amd._abi import DMATCH_DTYPE
    deps, imgs = T.scene()
    xy, pts = T.row_inputs()
    n, cap = T.N_ROWS, T.CAP
    rng = np.random.RandomState(21)
    pairs = [[0, 0], [1, 1], [0, 2], [1, 0], [0, 1], [0, 3]]
    P = len(pairs)
    matches = np.zeros((P, cap), DMATCH_DTYPE)
    matches["trainIdx"] = np.arange(cap)
    matches["queryIdx"] = rng.randint(0, cap, size=(P, cap))
    mask = np.ones((P, cap), np.uint8)
    mask[3] = rng.rand(cap) < 0.5
    num = np.array([n, n, n, n, -5, 40], np.int32)
    image_frame = [2, 0, 1]
    got = host_edges(loop, model, T.SENSORS[sensor], deps, imgs, image_frame, pairs, 2, matches, num, mask, pts[:3], xy[:3], cap)
    want = U.measurement_edges(matches, num, mask, pairs, 2, pts[:3], xy[:3], image_frame, list(deps), list(imgs), T.K, T.SCALE,
                               U.sensor(**T.SENSORS[sensor]), model, cap)
    assert got["count"].tolist() == [w["count"] for w in want] and got["count"][:3].tolist() == [n] * 3 and got["count"][4:].tolist() == [0, 0]
    for p, w in enumerate(want):
        k = w["count"]
        if not k:
            continue
        assert np.array_equal(got["mapRow"][p, :k], w["mapRow"]) and np.array_equal(got["curRow"][p, :k], w["curRow"])
        assert got["uv"][p, :k].tobytes() == w["uv"].tobytes()
        for m in ("position",) + T.MEMBERS:
            T.same_rows(got[m][p, :k], w[m], (model, sensor, m, p))
