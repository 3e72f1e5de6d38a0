"""Host side of the spatial-exclusion filters (include/putslam_hip.h: ps_sqrt_bound_f64, the PsExclusionRule constructors,
argument checks) and the numpy restatement they are measured against (tests/exclusion_ref_py.py).  No GPU."""
import ctypes as C
import math
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exclusion_ref_py as R  # noqa: E402

F32, F64 = np.float32, np.float64


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _dbl(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _step32(x, k):
    """float32 x moved by k ulps (positive finite values)."""
    return np.array([int(np.array([x], F32).view(np.uint32)[0]) + k], np.uint32).view(F32)[0]


@pytest.fixture(scope="module")
def L():
    from putslam_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def api():
    from putslam_amd import api
    return api


SPREAD = [1e-300, 5e-324, 1e-160, 1e-8, 0.003, 0.03, 0.1, 1.0 / 3.0, 0.5, 1.0, math.sqrt(2.0), 2.0, 3.0, 7.5, 10.0, 100.0, 1e4,
          123456.789, 1e8, 1e150, 1.3e154, float(F32(0.03)), float(F32(2.0)), float(F32(0.1))]


def test_sqrt_bound_f64_brute_force(L):
    """s = ps_sqrt_bound_f64(d) is the least double whose root reaches d: checked on the 129 doubles around it."""
    for d in SPREAD:
        s = L.ps_sqrt_bound_f64(d)
        b = _bits(s)
        for k in range(-64, 65):
            if b + k < 0 or b + k > 0x7FF0000000000000:
                continue
            t = _dbl(b + k)
            assert (math.sqrt(t) < d) == (k < 0), (d, k, t)


def test_sqrt_bound_f64_special_values(L):
    assert L.ps_sqrt_bound_f64(0.0) == 0.0 and L.ps_sqrt_bound_f64(-0.0) == 0.0
    assert L.ps_sqrt_bound_f64(-1.0) == 0.0 and L.ps_sqrt_bound_f64(float("-inf")) == 0.0
    assert L.ps_sqrt_bound_f64(float("nan")) == 0.0
    assert L.ps_sqrt_bound_f64(float("inf")) == float("inf")
    big = 1.7e308     # finite, but no finite double's root reaches it
    assert L.ps_sqrt_bound_f64(big) == float("inf")
    assert L.ps_sqrt_bound_f64(1.0) == 1.0 and L.ps_sqrt_bound_f64(2.0) == 4.0


def test_sizeof_and_fields(L, api):
    from putslam_amd._abi import PsExclusionRule
    assert L.ps_abi_sizeof_exclusion_rule() == C.sizeof(PsExclusionRule) == 56
    r = api.rule_new_map_features(0.03, 2.0, 200)
    assert (r.form3, r.form2, r.mode, r.maxKeep, r.depthGate, r.reserved) == (1, 2, 0, 200, 1, 0)
    assert (r.depthMin, r.depthMax) == (0.8, 6.0)
    assert api.rule_new_map_features(0.03, 2.0, 0).maxKeep == 0 and api.rule_new_map_features(0.03, 2.0, -7).maxKeep == 0
    r = api.rule_merge_tracked(5.0)
    assert (r.form3, r.form2, r.mode, r.maxKeep, r.depthGate) == (0, 2, 0, -1, 0)
    r = api.rule_too_close(0.1, 5.0)
    assert (r.form3, r.form2, r.mode, r.maxKeep, r.depthGate) == (2, 2, 1, -1, 0)


def _rule_near(r, p3, p2, q3, q2):
    """The rule's predicate as the kernel evaluates it (squared sums against the bounds), in numpy."""
    hit = False
    with np.errstate(invalid="ignore", over="ignore"):
        if r.form3:
            d = (np.asarray(p3, F32) - np.asarray(q3, F32)).astype(F32)
            if r.form3 == 1:
                s = F32(d[0] * d[0]) + F32(F32(d[1] * d[1]) + F32(d[2] * d[2]))
                hit = bool(F64(F32(s)) < r.bound3)
            else:
                x = d.astype(F64)
                hit = bool(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] < r.bound3)
        if r.form2:
            e = (np.asarray(p2, F32) - np.asarray(q2, F32)).astype(F32).astype(F64)
            hit = hit or bool(e[0] * e[0] + e[1] * e[1] < r.bound2)
    return hit


def _straddles(d):
    """Pairs of float32 coordinates on one axis whose difference lies one ulp inside, on and outside d, and a few ulps around."""
    out = []
    for base in (0.0, 1.0, 3.25, 100.0, 317.5):
        for k in range(-3, 4):
            hi = _step32(F32(F32(base) + F32(d)), k) if F32(F32(base) + F32(d)) > 0 else F32(0)
            out.append((F32(base), F32(hi)))
    return out


def test_rule_new_map_features_straddles(api):
    """C1's bounds against the restatement's predicate on one-ulp straddles, with thresholds that are NOT floats: the rule must
    round them through float as the reference's parameter does (PUTSLAM.cpp:101)."""
    far2, far3 = np.array([1e4, 1e4], F32), np.array([50.0, 50.0, 50.0], F32)
    for dE, dI in ((0.03, 2.0), (0.1, 5.0), (0.0300000001, 1.9999999), (1.0 / 3.0, 10.0 / 3.0), (0.8, 0.7)):
        r = api.rule_new_map_features(dE, dI, 5)
        fE, fI = float(F32(dE)), float(F32(dI))
        for axis in range(3):
            for a, b in _straddles(fE):
                p, q = np.zeros(3, F32), np.zeros(3, F32)
                p[axis], q[axis] = a, b
                want = bool(R.near_new_map(p, far2, q, np.zeros(2, F32), F32(dE), F32(dI)))
                assert _rule_near(r, p, far2, q, np.zeros(2, F32)) == want, (dE, axis, a, b)
        for axis in range(2):
            for a, b in _straddles(fI):
                p, q = np.zeros(2, F32), np.zeros(2, F32)
                p[axis], q[axis] = a, b
                want = bool(R.near_new_map(far3, p, np.zeros(3, F32), q, F32(dE), F32(dI)))
                assert _rule_near(r, far3, p, np.zeros(3, F32), q) == want, (dI, axis, a, b)
    # the float round trip itself: 0.03 as a double is above (float)0.03; a float norm in between tells the two apart
    r = api.rule_new_map_features(0.03, 2.0, 5)
    assert r.bound3 == api.map_sphere_bound(float(F32(0.03))) and r.bound2 == api.dbscan_bound(float(F32(2.0)))
    # a pair exactly (float)0.03 apart: its float norm equals the rounded threshold and lies below the double 0.03
    p, q = np.zeros(3, F32), np.array([F32(0.03), 0, 0], F32)
    assert float(F32(0.03)) < 0.03 and not _rule_near(r, p, far2, q, np.zeros(2, F32))
    assert not bool(R.near_new_map(p, far2, q, np.zeros(2, F32), F32(0.03), F32(2.0)))


def test_rule_merge_and_too_close_straddles(api):
    rng = np.random.default_rng(5)
    for d in (0.5, 2.0, 5.0, 10.0 / 3.0, 0.1):
        rm = api.rule_merge_tracked(d)
        rt = api.rule_too_close(d / 10.0, d)
        assert rm.bound2 == api.sqrt_bound_f64(d) and rt.bound3 == api.sqrt_bound_f64(d / 10.0) and rt.bound2 == rm.bound2
        far3 = np.array([50.0, 50.0, 50.0], F32)
        for axis in range(2):
            for a, b in _straddles(d):
                p, q = np.zeros(2, F32), np.zeros(2, F32)
                p[axis], q[axis] = a, b
                assert _rule_near(rm, None, p, None, q) == bool(R.near_merge(p, q, d)), (d, a, b)
                assert _rule_near(rt, far3, p, np.zeros(3, F32), q) == \
                    bool(R.near_too_close(far3, p, np.zeros(3, F32), q, d / 10.0, d)), (d, a, b)
        for axis in range(3):
            for a, b in _straddles(d / 10.0):
                p, q = np.zeros(3, F32), np.zeros(3, F32)
                p[axis], q[axis] = a, b
                far2 = np.array([1e4, 1e4], F32)
                assert _rule_near(rt, p, far2, q, np.zeros(2, F32)) == \
                    bool(R.near_too_close(p, far2, q, np.zeros(2, F32), d / 10.0, d)), (d, a, b)
        # oblique pairs near the bound
        for _ in range(300):
            ang = rng.uniform(0, 2 * np.pi)
            rad = d * (1 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-9, -5))
            p = rng.uniform(0, 600, 2).astype(F32)
            q = (p + rad * np.array([np.cos(ang), np.sin(ang)])).astype(F32)
            assert _rule_near(rm, None, p, None, q) == bool(R.near_merge(p, q, d))


def test_null_and_bad_arguments_without_a_gpu(L):
    from putslam_amd._abi import PsExclusionRule
    assert L.ps_exclusion_rule_new_map_features(0.03, 2.0, 200, None) == -1
    assert L.ps_exclusion_rule_merge_tracked(5.0, None) == -1
    assert L.ps_exclusion_rule_too_close(0.1, 5.0, None) == -1
    r = PsExclusionRule()
    assert L.ps_exclusion_rule_merge_tracked(5.0, C.byref(r)) == 0
    kept = np.full(4, -7, np.int32)
    nk = C.c_int(-7)
    xy = np.zeros((4, 2), np.float32)
    # no context: PS_ERR_BAD_ARG, outputs untouched
    assert L.ps_exclude(None, C.byref(r), None, xy.ctypes.data, 4, None, None, 0, kept.ctypes.data, C.byref(nk)) == -1
    assert L.ps_exclude_device(None, C.byref(r), None, None, None, 4, None, None, None, 0, 1, None, None) == -1
    assert nk.value == -7 and (kept == -7).all()


def _conflict_scan_new_map(f3, f2, m3, m2, cap, dE, dI):
    """Second formulation of C1: the full conflict matrix first, then a scan over it."""
    n = len(f3)
    gate = np.array([(F64(z) > 0.8) and (F64(z) < 6.0) for z in f3[:, 2]], bool) if n else np.zeros(0, bool)
    blocked = np.array([R.near_new_map(m3, m2, f3[j], f2[j], dE, dI).any() for j in range(n)], bool) if n else np.zeros(0, bool)
    conf = np.zeros((n, n), bool)
    for j in range(n):
        conf[j] = R.near_new_map(f3, f2, f3[j], f2[j], dE, dI)
    acc = np.zeros(n, bool)
    for j in range(n):
        if gate[j] and not blocked[j] and not (conf[j, :j] & acc[:j]).any():
            acc[j] = True
    return np.flatnonzero(acc)[:max(cap, 0)].astype(np.int32)


def _scene(rng, n, m):
    m3 = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(0.5, 6.5, m)], 1).astype(F32)
    m2 = np.stack([rng.uniform(0, 640, m), rng.uniform(0, 480, m)], 1).astype(F32)
    f3 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 6.5, n)], 1).astype(F32)
    f2 = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(F32)
    for j in range(n):          # half of the candidates sit on a map feature or on an earlier candidate
        u = rng.random()
        if u < 0.3 and m:
            k = rng.integers(m)
            f3[j] = m3[k] + rng.normal(0, 0.02, 3).astype(F32)
            f2[j] = m2[k] + rng.normal(0, 1.5, 2).astype(F32)
        elif u < 0.55 and j:
            k = rng.integers(j)
            f3[j] = f3[k] + rng.normal(0, 0.02, 3).astype(F32)
            f2[j] = f2[k] + rng.normal(0, 1.5, 2).astype(F32)
    return f3, f2, m3, m2


def test_restatement_against_conflict_matrix_scan():
    rng = np.random.default_rng(11)
    for trial in range(30):
        n, m = int(rng.integers(0, 120)), int(rng.integers(0, 150))
        f3, f2, m3, m2 = _scene(rng, n, m)
        dE, dI = F32(rng.choice([0.03, 0.1, 0.3])), F32(rng.choice([2.0, 5.0, 20.0]))
        cap = int(rng.choice([0, 1, 5, 40, 1000]))
        got, cnt = R.choose_features_to_add_to_map(f3, f2, m3, m2, 0, cap, dE, dI)
        want = _conflict_scan_new_map(f3, f2, m3, m2, cap, F64(dE), F64(dI))
        assert got.tobytes() == want.tobytes() and cnt == len(want), trial
        # a count that continues: the first k, then the rest with the first k as existing features, is the same set
        if len(want) >= 2:
            k = len(want) // 2
            a, c1 = R.choose_features_to_add_to_map(f3, f2, m3, m2, 0, k, dE, dI)
            assert a.tobytes() == want[:k].tobytes() and c1 == k
        # C2: greedy over the conflict matrix
        d = float(rng.choice([2.0, 5.0, 12.5]))
        got = R.merge_tracked_features(m2, f2, d)
        acc = []
        for j in range(n):
            if not R.near_merge(m2, f2[j], d).any() and not any(R.near_merge(f2[i], f2[j], d) for i in acc):
                acc.append(j)
        assert got.tobytes() == np.asarray(acc, np.int32).tobytes(), trial
        # C3: the pair loop written as the reference writes it, i outer, j inner
        a3, b2 = float(rng.choice([0.05, 0.2])), float(rng.choice([3.0, 8.0]))
        rm = set()
        for i in range(n):
            for j in range(i + 1, n):
                if R.near_too_close(f3[i], f2[i], f3[j], f2[j], a3, b2):
                    rm.add(j)
        assert R.remove_too_close_features(f3, f2, a3, b2).tolist() == sorted(rm), trial


def test_restatement_nan_blocks_nothing():
    f3 = np.array([[0, 0, 1], [np.nan, 0, 1], [0, 0, 1], [0, 0, np.nan]], F32)
    f2 = np.array([[10, 10], [10, 10], [500, 400], [300, 300]], F32)
    got, _ = R.choose_features_to_add_to_map(f3, f2, np.zeros((0, 3)), np.zeros((0, 2)), 0, 10, 0.03, 2.0)
    # 1: its 3-D test is NaN but the 2-D test blocks it; 2: blocked in 3-D by 0; 3: NaN depth fails the gate
    assert got.tolist() == [0]
    f2 = np.array([[10, 10], [np.nan, 10], [10.5, 10]], F32)
    assert R.merge_tracked_features(np.zeros((0, 2)), f2, 2.0).tolist() == [0, 1]
