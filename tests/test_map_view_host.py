"""Host half of the device-built map views (no GPU): the level thresholds against ps_predicted_level, ps_view_angles against
the restatement, struct sizes, argument checks, and the restatement of tests/map_view_ref.py against its second formulation."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_view_ref as vref  # noqa: E402

from putslam_amd import _lib, api  # noqa: E402
from putslam_amd._abi import PS_LEVEL_OCTAVE_MAX, PS_LEVEL_OCTAVE_MIN, PsFrameSet, PsMapStore, PsMapViewOut, PsMapViewRequest  # noqa: E402


def count_rule(t, x):
    """The level rule of include/putslam_hip.h on x itself."""
    return int(sum(x >= tk for tk in t)) if math.isfinite(x) else 0


def test_thresholds_are_the_switching_points_of_predicted_level():
    L = _lib.load()
    t = api.level_thresholds()
    assert t.shape == (7,) and (np.diff(t) > 0).all()
    for k, tk in enumerate(t):
        # 0, 1 or 2 ulps above 1.2^k on glibc; in any case next to it
        assert abs(tk - 1.2 ** k) <= 8 * np.spacing(tk), (k, tk)
        x = tk
        for _ in range(64):
            x = np.nextafter(x, 0.0)
        for _ in range(129):                         # every double within 64 ulps of t[k]; x passes through unchanged
            assert count_rule(t, float(x)) == L.ps_predicted_level(0, float(x), 1.0), (k, float(x).hex())
            x = np.nextafter(x, np.inf)
        assert L.ps_predicted_level(0, float(tk), 1.0) == k + 1
        assert L.ps_predicted_level(0, float(np.nextafter(tk, 0.0)), 1.0) == k


def test_level_rule_equals_predicted_level_on_random_and_special_inputs():
    L = _lib.load()
    t = api.level_thresholds()
    rng = np.random.default_rng(5)
    n = 100000
    octave = rng.integers(PS_LEVEL_OCTAVE_MIN, PS_LEVEL_OCTAVE_MAX + 1, n)
    octave[: n // 2] = rng.integers(0, 8, n // 2)
    det = np.exp(rng.uniform(-3, 3, n))
    cur = np.exp(rng.uniform(-3, 3, n))
    hist = np.zeros(8, int)
    for o, d, c in zip(octave, det, cur):
        x = (math.pow(1.2, int(o)) * float(d)) / float(c)          # the rule's x, left to right
        lv = L.ps_predicted_level(int(o), float(d), float(c))
        assert count_rule(t, x) == lv, (o, d, c)
        hist[lv] += 1
    assert (hist > 500).all(), hist
    nan, inf = float("nan"), float("inf")
    for d, c in ((nan, 1.0), (1.0, nan), (inf, 1.0), (-inf, 1.0), (1.0, inf), (0.0, 1.0), (-0.0, 1.0), (-2.0, 1.0), (1.0, 0.0),
                 (1.0, -0.0), (0.0, 0.0), (1e308, 1e-308), (5e-324, 1.0), (3.0, 1.0), (1.0, 1.0)):
        with np.errstate(all="ignore"):
            x = float(np.float64(1.0) * np.float64(d) / np.float64(c))
        assert count_rule(t, x) == L.ps_predicted_level(0, d, c), (d, c, x)
    assert L.ps_level_thresholds(None) == -1


def _angles_bitwise(cur, poses):
    got, want = api.view_angles(cur, poses), vref.view_angles(cur, poses)
    assert got.tobytes() == want.tobytes() or (np.isnan(got) == np.isnan(want)).all() and \
        got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes()
    return got


def test_view_angles_match_the_restatement():
    rng = np.random.default_rng(11)
    poses = vref.make_poses(rng, 400, max_rot=3.1)
    for cur in vref.make_poses(rng, 6, max_rot=2.0):
        a = _angles_bitwise(cur, poses)
        assert a.min() >= 0 and a.max() <= math.pi and a.std() > 0.3
    # identical poses: r sits at or next to 1 (acos of 1 is 0, of the float above 1 NaN, of the float below 3.4e-4)
    seen = set()
    for P in vref.make_poses(rng, 300, max_rot=3.1):
        a = _angles_bitwise(P, P[None])
        seen.add("nan" if a[0] != a[0] else ("zero" if a[0] == 0 else "next"))
        assert a[0] != a[0] or a[0] < 1e-3
    assert "zero" in seen and len(seen) >= 2, seen
    # a zero third column: 0 / 0
    Z = np.eye(4)
    Z[:3, 2] = 0
    a = _angles_bitwise(np.eye(4), np.stack([Z, np.eye(4)]))
    assert a[0] != a[0] and a[1] == 0
    assert _angles_bitwise(Z, np.eye(4)[None])[0] != _angles_bitwise(Z, np.eye(4)[None])[0]
    L = _lib.load()
    out = np.zeros(2)
    assert L.ps_view_angles(None, None, 0, None) == -1
    assert L.ps_view_angles(Z.ctypes.data_as(C.c_void_p), None, 2, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.ps_view_angles(Z.ctypes.data_as(C.c_void_p), Z.ctypes.data_as(C.c_void_p), -1, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.ps_view_angles(Z.ctypes.data_as(C.c_void_p), None, 0, None) == 0


def test_struct_sizes():
    L = _lib.load()
    sizes = _lib.struct_sizes()
    for name, cls in (("map_store", PsMapStore), ("map_view_request", PsMapViewRequest), ("map_view_out", PsMapViewOut)):
        assert getattr(L, "ps_abi_sizeof_" + name)() == C.sizeof(cls) == sizes[name], name
    assert C.sizeof(PsMapStore) == 64 and C.sizeof(PsMapViewRequest) == 104 and C.sizeof(PsMapViewOut) == C.sizeof(PsFrameSet) + 56


def test_device_calls_reject_a_null_context():
    """Without a context there is nothing to run on and nowhere to leave an error text: PS_ERR_BAD_ARG, no GPU needed."""
    L = _lib.load()
    st, rq, out, fs = PsMapStore(), PsMapViewRequest(), PsMapViewOut(), PsFrameSet()
    assert L.ps_map_views_device(None, C.byref(st), C.byref(rq), C.byref(out)) == -1
    assert L.ps_map_views_device(None, None, None, None) == -1
    assert L.ps_frame_levels_device(None, C.byref(fs), None, None, None) == -1


def test_sequential_restatement_equals_the_matrix_formulation():
    rng = np.random.default_rng(2026)
    for F, N, V, nan in ((1500, 50, 3, 0), (800, 400, 2, 40), (300, 7, 2, 2)):
        store = vref.make_store(rng, F, N)
        cam_inv, ang, _, _ = vref.make_request(rng, store, V, nan_entries=nan)
        cand, cc = vref.ragged_candidates(rng, F, V, F // 2)
        for vis in (False, True):
            for c, n in ((None, None), (cand, cc)):
                a = vref.build_views(store, cam_inv, ang, 0.45, vref.K_TUM, vref.IMAGE, F, c, n, vis)
                b = vref.build_views(store, cam_inv, ang, 0.45, vref.K_TUM, vref.IMAGE, F, c, n, vis, fast=True)
                for x, y in zip(a, b):
                    assert x["viewCount"] == y["viewCount"] and vref.rows_equal(x["rows"], y["rows"])
                assert any(0 < x["viewCount"] < (F if c is None else max(int(n.max()), 1)) for x in a)
    # ties keep the first pose; a bad pose id, octave or index invalidates the view in both
    store = vref.make_store(rng, 40, 10, obs_per_feature=4)
    cam_inv, ang, _, _ = vref.make_request(rng, store, 1)
    ang[0, :] = 0.25
    a = vref.build_views(store, cam_inv, ang, 0.3, vref.K_TUM, vref.IMAGE, 40)
    assert (a[0]["rows"]["obsIdx"] % 4 == 0).all() and a[0]["viewCount"] == 40
    for key, val in (("obs_pose", 10), ("obs_pose", -1), ("obs_octave", 48), ("obs_octave", -17)):
        s2 = dict(store)
        s2[key] = store[key].copy()
        s2[key][8] = val                                         # (observation 8 is feature 2's first: the chosen one)
        for fast in (False, True):
            assert vref.build_views(s2, cam_inv, ang, 0.3, vref.K_TUM, vref.IMAGE, 40, fast=fast)[0]["viewCount"] == -2 ** 31
    for fast in (False, True):
        w = vref.build_views(store, cam_inv, ang, 0.3, vref.K_TUM, vref.IMAGE, 40, np.array([[3, 40]], np.int32), np.array([2]), fast=fast)
        assert w[0]["viewCount"] == -2 ** 31
        w = vref.build_views(store, cam_inv, ang, 0.3, vref.K_TUM, vref.IMAGE, 12)
        assert w[0]["viewCount"] == -40 and w[0]["nkpts"] == 0


def test_level_edge_inputs_hit_every_threshold():
    t = api.level_thresholds()
    edges = vref.level_edge_inputs(t)
    for k in range(7):
        for kind in ("on", "below"):
            assert any(e[2] == k and e[3] == kind and e[0] == 0 for e in edges)
    assert any(e[0] != 0 for e in edges)
    for o, d, k, kind in edges:
        assert vref.predicted_level(o, d, 2.0) == (k + 1 if kind == "on" else k), (o, d, k, kind)
