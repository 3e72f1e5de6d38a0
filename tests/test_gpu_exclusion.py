"""Spatial-exclusion filters on the GPU (ps_exclusion.h): ps_exclude, ps_exclude_device, the Python methods and the drop-in equal
the sequential numpy restatement of the reference's loops (tests/exclusion_ref_py.py) byte for byte."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import exclusion_ref_py as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
E3, E2 = np.zeros((0, 3), F32), np.zeros((0, 2), F32)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def _same(a, b):
    return np.asarray(a, np.int32).tobytes() == np.asarray(b, np.int32).tobytes()


def _ref_c1(f3, f2, m3, m2, dE, dI, cap):
    return R.choose_features_to_add_to_map(f3, f2, m3, m2, 0, cap, F32(dE), F32(dI))[0]


def _ref_c3(f3, f2, a, b):
    rm = R.remove_too_close_features(f3, f2, a, b)
    return np.setdiff1d(np.arange(len(f3), dtype=np.int32), rm).astype(np.int32)


def _step32(x, k):
    return np.array([int(np.array([x], F32).view(np.uint32)[0]) + k], np.uint32).view(F32)[0]


def _batch(ctx, rule, frames, cap=None, ecap=None):
    """frames: list of (cand3, cand2, exist3, exist2) (None where the rule does not read) -> kept index arrays (None for -1)."""
    import torch
    from putslam_amd import device_batch
    F = len(frames)
    n = [len(f[1]) for f in frames]
    m = [len(f[3]) if f[3] is not None else 0 for f in frames]
    cap = cap or max(1, max(n))
    ecap = max(m) if ecap is None else ecap
    use3 = frames[0][0] is not None
    c3, c2 = np.zeros((F, cap, 3), F32), np.zeros((F, cap, 2), F32)
    e3, e2 = np.zeros((F, max(ecap, 1), 3), F32), np.zeros((F, max(ecap, 1), 2), F32)
    for i, (a3, a2, b3, b2) in enumerate(frames):
        c2[i, :n[i]] = a2
        if use3:
            c3[i, :n[i]] = a3
        if m[i]:
            e2[i, :m[i]] = b2
            if use3:
                e3[i, :m[i]] = b3
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    kept, nk = device_batch.exclude_device(ctx, rule, t(c3) if use3 else None, t(c2), t(np.asarray(n, np.int32)),
                                           (t(e3) if use3 else None) if ecap else None, t(e2) if ecap else None,
                                           t(np.asarray(m, np.int32)) if ecap else None)
    torch.cuda.synchronize()
    kept, nk = kept.cpu().numpy(), nk.cpu().numpy()
    return [kept[i, :nk[i]].copy() if nk[i] >= 0 else None for i in range(F)]


def _scene(rng, n, m, near=0.55):
    """Candidates and map features in a camera frustum; a share `near` of the candidates sits on a map feature or on an earlier
    candidate, at about the thresholds' distance."""
    def cloud(k):
        return (np.stack([rng.uniform(-2, 2, k), rng.uniform(-1.5, 1.5, k), rng.uniform(0.5, 6.5, k)], 1).astype(F32),
                np.stack([rng.uniform(0, 640, k), rng.uniform(0, 480, k)], 1).astype(F32))
    m3, m2 = cloud(m)
    f3, f2 = cloud(n)
    u = rng.random(n)
    for j in range(n):
        if u[j] < near * 0.55 and m:
            k = rng.integers(m)
            f3[j] = m3[k] + rng.normal(0, 0.02, 3).astype(F32)
            f2[j] = m2[k] + rng.normal(0, 1.5, 2).astype(F32)
        elif u[j] < near and j:
            k = rng.integers(j)
            f3[j] = f3[k] + rng.normal(0, 0.02, 3).astype(F32)
            f2[j] = f2[k] + rng.normal(0, 1.5, 2).astype(F32)
    return f3, f2, m3, m2


# ---------------------------------------------------------------- random sweeps
def test_random_sweep_new_map_features(ctx):
    from putslam_amd import api
    rng = np.random.default_rng(1)
    bad = []
    for trial in range(60):
        n, m = int(rng.integers(0, 1500)), int(rng.integers(0, 2500))
        f3, f2, m3, m2 = _scene(rng, n, m, near=rng.choice([0.1, 0.55, 0.9]))
        dE, dI = float(rng.choice([0.03, 0.01, 0.1, 0.25])), float(rng.choice([2.0, 0.5, 5.0, 12.0]))
        cap = int(rng.choice([200, 1, 17, 100000]))
        want = _ref_c1(f3, f2, m3, m2, dE, dI, cap)
        got = ctx.choose_new_features(f3, f2, m3, m2, dE, dI, cap)
        got2 = ctx.exclude(api.rule_new_map_features(dE, dI, cap), f3, f2, m3, m2)
        if not (_same(got, want) and _same(got2, want)):
            bad.append((trial, n, m, dE, dI, cap, len(got), len(want)))
    assert not bad, bad[:10]


def test_random_sweep_merge_and_too_close(ctx):
    rng = np.random.default_rng(2)
    bad = []
    for trial in range(40):
        n, m = int(rng.integers(0, 1500)), int(rng.integers(0, 1500))
        f3, f2, m3, m2 = _scene(rng, n, m)
        d = float(rng.choice([3.0, 1.0, 7.5, 10.0 / 3.0]))
        if not _same(ctx.merge_tracked_features(m2, f2, d), R.merge_tracked_features(m2, f2, d)):
            bad.append(("merge", trial, n, m, d))
        a = float(rng.choice([0.01, 0.03, 0.2]))
        if not _same(ctx.remove_too_close_features(f3, f2, a, d), _ref_c3(f3, f2, a, d)):
            bad.append(("close", trial, n, a, d))
    assert not bad, bad[:10]


def test_random_sweep_device_batches(ctx):
    from putslam_amd import api
    rng = np.random.default_rng(3)
    for dE, dI, cap in ((0.03, 2.0, 200), (0.1, 5.0, 100000)):
        frames = [_scene(rng, int(rng.integers(0, 700)), int(rng.integers(0, 900))) for _ in range(24)]
        got = _batch(ctx, api.rule_new_map_features(dE, dI, cap), frames)
        assert all(_same(g, _ref_c1(*f, dE, dI, cap)) for g, f in zip(got, frames))
    frames = [_scene(rng, int(rng.integers(0, 700)), int(rng.integers(0, 900))) for _ in range(24)]
    got = _batch(ctx, api.rule_merge_tracked(3.0), [(None, f[1], None, f[3]) for f in frames])
    assert all(_same(g, R.merge_tracked_features(f[3], f[1], 3.0)) for g, f in zip(got, frames))
    got = _batch(ctx, api.rule_too_close(0.02, 3.0), [(f[0], f[1], None, None) for f in frames], ecap=0)
    assert all(_same(g, _ref_c3(f[0], f[1], 0.02, 3.0)) for g, f in zip(got, frames))


# ---------------------------------------------------------------- one ulp inside, on and outside each of the four bounds
def _straddle_pairs(rng, d, dim, count=120, z=None):
    """Pairs (p, q) of float32 points in `dim` dimensions whose distance lies within a few ulps of d: axis-aligned ones stepped by
    ulps (base 0: the float difference IS the stepped value), and oblique ones.  z: depth given to the pairs that differ in x or y
    (3-D pairs that must pass C1's depth gate)."""
    out = []
    for base in (0.0, 1.0, 3.25, 100.0, 317.5):
        for axis in range(dim):
            for k in range(-3, 4):
                p, q = np.zeros(dim, F32), np.zeros(dim, F32)
                p[:] = F32(base)
                q[:] = F32(base)
                q[axis] = _step32(F32(F32(base) + F32(d)), k)
                if z is not None and axis != 2:
                    p[2] = q[2] = F32(z)
                out.append((p, q))
    for _ in range(count):
        v = rng.normal(size=dim)
        v /= np.linalg.norm(v)
        p = rng.uniform(1.5, 4.5, dim).astype(F32)
        q = (p.astype(F64) + v * d * (1 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-9, -6))).astype(F32)
        for k in (-1, 0, 1):
            q2 = q.copy()
            q2[0] = _step32(q2[0], k)
            out.append((p, q2))
    return out


def test_pairs_straddling_the_four_bounds(ctx):
    from putslam_amd import api
    rng = np.random.default_rng(4)
    far3a, far3b = np.array([0, 0, 1], F32), np.array([3, 3, 4], F32)
    far2a, far2b = np.array([0, 0], F32), np.array([600, 400], F32)
    inside = outside = 0
    # C1 3-D (float norm), as candidate against candidate and as candidate against map feature; depth inside the gate
    for dE in (0.03, 0.1, 1.0 / 3.0):
        prs = [(p, q) for p, q in _straddle_pairs(rng, float(F32(dE)), 3, z=2.0) if 0.9 < p[2] < 5 and 0.9 < q[2] < 5]
        rule = api.rule_new_map_features(dE, 2.0, 10)
        got = _batch(ctx, rule, [(np.stack([p, q]), np.stack([far2a, far2b]), E3, E2) for p, q in prs], ecap=0)
        got += _batch(ctx, rule, [(q[None], far2b[None], p[None], far2a[None]) for p, q in prs])
        want = [_ref_c1(np.stack([p, q]), np.stack([far2a, far2b]), E3, E2, dE, 2.0, 10) for p, q in prs]
        want += [_ref_c1(q[None], far2b[None], p[None], far2a[None], dE, 2.0, 10) for p, q in prs]
        assert all(_same(g, w) for g, w in zip(got, want)), dE
        inside += sum(len(w) == 1 for w in want[:len(prs)])
        outside += sum(len(w) == 2 for w in want[:len(prs)])
    # C1 2-D ((float) of the double root)
    for dI in (2.0, 0.7, 10.0 / 3.0):
        prs = _straddle_pairs(rng, float(F32(dI)), 2)
        rule = api.rule_new_map_features(0.03, dI, 10)
        got = _batch(ctx, rule, [(np.stack([far3a, far3b]), np.stack([p, q]), E3, E2) for p, q in prs], ecap=0)
        want = [_ref_c1(np.stack([far3a, far3b]), np.stack([p, q]), E3, E2, 0.03, dI, 10) for p, q in prs]
        assert all(_same(g, w) for g, w in zip(got, want)), dI
        inside += sum(len(w) == 1 for w in want)
        outside += sum(len(w) == 2 for w in want)
    # C2 2-D (double root), C3 2-D and 3-D
    for d in (3.0, 0.7, 10.0 / 3.0):
        prs = _straddle_pairs(rng, d, 2)
        got = _batch(ctx, api.rule_merge_tracked(d), [(None, np.stack([p, q]), None, None) for p, q in prs], ecap=0)
        got += _batch(ctx, api.rule_merge_tracked(d), [(None, q[None], None, p[None]) for p, q in prs])
        want = [R.merge_tracked_features(E2, np.stack([p, q]), d) for p, q in prs]
        want += [R.merge_tracked_features(p[None], q[None], d) for p, q in prs]
        assert all(_same(g, w) for g, w in zip(got, want)), d
        got = _batch(ctx, api.rule_too_close(0.01, d), [(np.stack([far3a, far3b]), np.stack([p, q]), None, None) for p, q in prs], ecap=0)
        want3 = [_ref_c3(np.stack([far3a, far3b]), np.stack([p, q]), 0.01, d) for p, q in prs]
        assert all(_same(g, w) for g, w in zip(got, want3)), d
        inside += sum(len(w) == 1 for w in want3)
        outside += sum(len(w) == 2 for w in want3)
    for a in (0.01, 0.2, 1.0 / 3.0):
        prs = _straddle_pairs(rng, a, 3)
        got = _batch(ctx, api.rule_too_close(a, 3.0), [(np.stack([p, q]), np.stack([far2a, far2b]), None, None) for p, q in prs], ecap=0)
        want3 = [_ref_c3(np.stack([p, q]), np.stack([far2a, far2b]), a, 3.0) for p, q in prs]
        assert all(_same(g, w) for g, w in zip(got, want3)), a
        inside += sum(len(w) == 1 for w in want3)
        outside += sum(len(w) == 2 for w in want3)
    assert inside > 200 and outside > 200      # the pairs do fall on both sides


# ---------------------------------------------------------------- the cap, the depth gate
def test_cap_values(ctx):
    rng = np.random.default_rng(5)
    f3, f2, m3, m2 = _scene(rng, 1200, 800)
    full = _ref_c1(f3, f2, m3, m2, 0.03, 2.0, 10 ** 6)
    assert 300 < len(full) < 1100
    for cap in (0, -3, 1, 2, len(full) - 1, len(full), len(full) + 1, 10 ** 6):
        got = ctx.choose_new_features(f3, f2, m3, m2, 0.03, 2.0, cap)
        assert _same(got, full[:max(cap, 0)]) and _same(got, _ref_c1(f3, f2, m3, m2, 0.03, 2.0, cap)), cap


def test_depth_gate_edges(ctx):
    zs = []
    for z in (0.8, 6.0):
        zs += [_step32(F32(z), k) for k in range(-2, 3)]
    zs += [F32(0), F32(-1), F32(3), F32(np.inf), F32(np.nan), F32(0.1), F32(5.9999995), F32(0.80000001)]
    zs = np.asarray(zs, F32)
    n = len(zs)
    f3 = np.stack([np.arange(n, dtype=F32), np.zeros(n, F32), zs], 1)
    f2 = np.stack([np.arange(n, dtype=F32) * 50, np.zeros(n, F32)], 1)
    want = _ref_c1(f3, f2, E3, E2, 0.03, 2.0, 100)
    assert float(F32(0.8)) > 0.8 and 2 in want and 6 in want and 7 not in want      # (float)0.8 passes the gate, 6.0f does not
    assert _same(ctx.choose_new_features(f3, f2, E3, E2, 0.03, 2.0, 100), want)
    # a candidate outside the gate never blocks a later one
    f3 = np.array([[0, 0, 7.0], [0, 0, 3.0], [0, 0, 3.0]], F32)
    f2 = np.array([[5, 5], [5, 5], [5.5, 5]], F32)
    assert ctx.choose_new_features(f3, f2, E3, E2, 0.03, 2.0, 100).tolist() == [1] == _ref_c1(f3, f2, E3, E2, 0.03, 2.0, 100).tolist()


# ---------------------------------------------------------------- adversarial inputs
def _blob(n):
    rng = np.random.default_rng(30)
    f3 = (np.array([0.5, 0.2, 2.0]) + rng.uniform(-0.002, 0.002, (n, 3))).astype(F32)
    f2 = (np.array([320.0, 240.0]) + rng.uniform(-0.3, 0.3, (n, 2))).astype(F32)
    return f3, f2


def _chain(n):
    """Every point conflicts with its neighbours only: one component of n members, n / 2 accepted."""
    i = np.arange(n)
    f2 = np.stack([10 + 1.5 * i, 20 + 0.0 * i], 1).astype(F32)          # 1.5 px apart, threshold 2
    f3 = np.stack([0.05 * i, 0 * i, 2 + 0 * i], 1).astype(F32)
    return f3, f2


@pytest.mark.parametrize("case", ["blob3000", "chain5000", "identical", "nan_cand", "nan_map", "n0", "m0", "n0m0", "all_blocked",
                                  "two_chains_and_blobs"])
def test_adversarial(ctx, case):
    rng = np.random.default_rng(31)
    m3, m2 = E3, E2
    if case == "blob3000":
        f3, f2 = _blob(3000)
    elif case == "chain5000":
        f3, f2 = _chain(5000)
    elif case == "identical":
        f3, f2 = np.tile(np.array([[1, 1, 2]], F32), (700, 1)), np.tile(np.array([[9, 9]], F32), (700, 1))
    elif case == "nan_cand":
        f3, f2, m3, m2 = _scene(rng, 900, 600)
        f3[rng.random(900) < 0.2, 0] = np.nan
        f2[rng.random(900) < 0.2, 1] = np.nan
        f3[rng.random(900) < 0.1, 2] = np.nan
    elif case == "nan_map":
        f3, f2, m3, m2 = _scene(rng, 900, 600)
        m3[rng.random(600) < 0.3, 1] = np.nan
        m2[rng.random(600) < 0.3, 0] = np.nan
    elif case == "n0":
        f3, f2 = E3, E2
        _, _, m3, m2 = _scene(rng, 1, 300)
    elif case == "m0":
        f3, f2, _, _ = _scene(rng, 800, 0)
    elif case == "n0m0":
        f3, f2 = E3, E2
    elif case == "all_blocked":
        _, _, m3, m2 = _scene(rng, 1, 1500)
        pick = rng.integers(0, 1500, 1000)
        f3, f2 = m3[pick].copy(), (m2[pick] + F32(0.25)).astype(F32)
    else:
        a3, a2 = _chain(1500)
        b3, b2 = _blob(800)
        c3, c2 = _chain(900)
        c2[:, 1] += 200
        c3[:, 1] += 1
        f3, f2 = np.concatenate([a3, b3, c3]), np.concatenate([a2, b2, c2])
        perm = rng.permutation(len(f3))
        f3, f2 = f3[perm], f2[perm]
    want = _ref_c1(f3, f2, m3, m2, 0.03, 2.0, 10 ** 6)
    if case == "blob3000":
        assert want.tolist() == [0]
    if case == "chain5000":
        assert want.tolist() == list(range(0, 5000, 2))
    if case == "all_blocked":
        assert len(want) == 0
    assert _same(ctx.choose_new_features(f3, f2, m3, m2, 0.03, 2.0, 10 ** 6), want)
    assert _same(ctx.choose_new_features(f3, f2, m3, m2, 0.03, 2.0, 200), want[:200])
    assert _same(ctx.merge_tracked_features(m2, f2, 2.0), R.merge_tracked_features(m2, f2, 2.0))
    assert _same(ctx.remove_too_close_features(f3, f2, 0.03, 2.0), _ref_c3(f3, f2, 0.03, 2.0))


def test_largest_frame(ctx):
    """n = PS_EXCL_MAX_CAND candidates (the most dynamic LDS the resolving kernel asks for) against PS_MAX_KPTS map features."""
    from putslam_amd import api
    from putslam_amd._abi import PS_EXCL_MAX_CAND, PS_MAX_KPTS
    rng = np.random.default_rng(8192)
    n, m = PS_EXCL_MAX_CAND, PS_MAX_KPTS
    f3, f2, m3, m2 = _scene(rng, n, m, near=0.4)
    f2[:300] = (np.array([100.0, 100.0]) + rng.uniform(0, 12, (300, 2))).astype(F32)     # one large component
    want = _ref_c1(f3, f2, m3, m2, 0.03, 2.0, 10 ** 6)
    assert _same(ctx.choose_new_features(f3, f2, m3, m2, 0.03, 2.0, 10 ** 6), want)
    got = _batch(ctx, api.rule_new_map_features(0.03, 2.0, 10 ** 6), [(f3, f2, m3, m2), (f3[:8000], f2[:8000], m3[:9000], m2[:9000])])
    assert _same(got[0], want) and _same(got[1], _ref_c1(f3[:8000], f2[:8000], m3[:9000], m2[:9000], 0.03, 2.0, 10 ** 6))
    assert _same(ctx.remove_too_close_features(f3, f2, 0.01, 3.0), _ref_c3(f3, f2, 0.01, 3.0))
    assert _same(ctx.merge_tracked_features(m2, f2, 3.0), R.merge_tracked_features(m2, f2, 3.0))


# ---------------------------------------------------------------- batches
def test_ragged_batch_equals_single_calls_and_repeats(ctx):
    from putslam_amd import api
    rng = np.random.default_rng(6)
    frames = [_scene(rng, int(rng.integers(0, 1200)), int(rng.integers(0, 1500))) for _ in range(120)]
    frames[7] = _chain(1100) + (E3, E2)
    frames[8] = _blob(900) + frames[8][2:]
    rule = api.rule_new_map_features(0.03, 2.0, 200)
    got = _batch(ctx, rule, frames)
    for i, f in enumerate(frames):
        assert _same(got[i], ctx.choose_new_features(*f, 0.03, 2.0, 200)), i
    for i in range(0, 120, 10):
        assert _same(got[i], _ref_c1(*frames[i], 0.03, 2.0, 200)), i
    for _ in range(2):
        again = _batch(ctx, rule, frames)
        assert all(_same(a, b) for a, b in zip(got, again))


def test_counts_outside_capacity_mark_the_frame(ctx):
    import torch
    from putslam_amd import api, device_batch
    dev = torch.device("cuda:0")
    c2 = torch.zeros((5, 16, 2), dtype=torch.float32, device=dev)
    c3 = torch.ones((5, 16, 3), dtype=torch.float32, device=dev)
    e2 = torch.full((5, 8, 2), 100.0, dtype=torch.float32, device=dev)
    e3 = torch.full((5, 8, 3), 9.0, dtype=torch.float32, device=dev)
    cn = torch.tensor([4, 17, -1, 3, 2], dtype=torch.int32, device=dev)
    en = torch.tensor([2, 2, 2, 9, -1], dtype=torch.int32, device=dev)
    kept, nk = device_batch.exclude_device(ctx, api.rule_new_map_features(0.03, 2.0, 200), c3, c2, cn, e3, e2, en)
    torch.cuda.synchronize()
    assert nk.cpu().tolist() == [1, -1, -1, -1, -1] and kept[0, 0].item() == 0


def test_bad_arguments(ctx):
    from putslam_amd import api
    from putslam_amd._abi import PsExclusionRule
    rule = api.rule_new_map_features(0.03, 2.0, 200)
    with pytest.raises(api.PsError) as e:
        ctx.exclude(rule, np.zeros((8193, 3), F32), np.zeros((8193, 2), F32))
    assert e.value.code == -5 and "PS_EXCL_MAX_CAND" in str(e.value)           # PS_ERR_UNSUPPORTED
    with pytest.raises(api.PsError) as e:
        ctx.exclude(rule, None, np.zeros((4, 2), F32))                             # the rule reads 3-D data
    assert e.value.code == -1
    with pytest.raises(api.PsError) as e:
        ctx.exclude(rule, np.ones((4, 3), F32), np.zeros((4, 2), F32), None, np.zeros((2, 2), F32))
    assert e.value.code == -1
    bad = PsExclusionRule()
    bad.form3 = 7
    with pytest.raises(api.PsError) as e:
        ctx.exclude(bad, np.ones((4, 3), F32), np.zeros((4, 2), F32))
    assert e.value.code == -1 and "form3" in str(e.value)
    with pytest.raises(api.PsError) as e:
        ctx.exclude_device(rule, 0, 0, 0, 8193, 0, 0, 0, 0, 1, 0, 0)
    assert e.value.code == -5
    with pytest.raises(api.PsError) as e:
        ctx.exclude_device(rule, 0, 0, 0, 64, 0, 0, 0, 0, 1, 0, 0)
    assert e.value.code == -1
    # the context still works
    assert ctx.merge_tracked_features(E2, np.array([[0, 0], [1, 0], [5, 0]], F32), 2.0).tolist() == [0, 2]


def test_repeats_beside_a_vo_batch_on_a_second_context(ctx, oracle):
    import torch
    from putslam_amd import api, synth
    from putslam_amd._abi import EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    rng = np.random.default_rng(7)
    frames = [_scene(rng, int(rng.integers(200, 1500)), int(rng.integers(200, 2000))) for _ in range(48)]
    frames[3] = _chain(1400) + frames[3][2:]
    rule = api.rule_new_map_features(0.03, 2.0, 100000)
    want = [_ref_c1(*f, 0.03, 2.0, 100000) for f in frames]
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    seq = synth.make_sequence(9, 600, config=3, index=77)
    cfg_vo, _ = make_config(EST_RANSAC, 487, seed=1234)
    c_vo = oracle.vo_pairs(prm, cfg_vo, TUM_FR1_K, seq["desc"], seq["pts"], seq["nkpts"], seq["pairs"], threads=4)
    other = api.Context(0)
    s_ex, s_vo = torch.cuda.Stream(), torch.cuda.Stream()
    fs = FrameSetDevice(seq["desc"], seq["pts"], seq["nkpts"])
    pb = PairBatchDevice(seq["pairs"], fs.max_kpts)
    for rep in range(20):
        with torch.cuda.stream(s_vo):
            run_pairs(other, prm, cfg_vo, TUM_FR1_K, fs, pb)
            run_pairs(other, prm, cfg_vo, TUM_FR1_K, fs, pb)
        with torch.cuda.stream(s_ex):
            got = _batch(ctx, rule, frames)
        assert all(_same(g, w) for g, w in zip(got, want)), rep
    assert pb.download()["pose"].tobytes() == c_vo["pose"].tobytes()
    ctx.set_stream(0)      # (back to the context's own stream: s_ex ends with this test)
    other.close()


# ---------------------------------------------------------------- the drop-in
def test_dropin_equals_restatement(tmp_path):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_dropin()
    lib = os.path.join(ROOT, "putslam_amd")
    exe = str(tmp_path / "test_exclusion_dropin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(lib, "csrc", "dropin"), os.path.join(HERE, "cpp", "test_exclusion_dropin.cpp"), "-o", exe,
                           "-L", lib, "-lputslam_dropin", "-lputslam_hip", "-Wl,-rpath," + lib])
    rng = np.random.default_rng(8)
    cases, want = [], []
    for trial in range(12):
        n, m = int(rng.integers(0, 900)), int(rng.integers(0, 1200))
        f3, f2, m3, m2 = _scene(rng, n, m)
        mp = np.concatenate([m3, m2], 1).astype(F64) + rng.uniform(-1e-9, 1e-9, (m, 5))      # doubles the glue casts to float
        start, cap = int(rng.choice([0, 0, 5, 150, 300])), int(rng.choice([200, 200, 1, 100000]))
        dE, dI = F32(rng.choice([0.03, 0.1])), F32(rng.choice([2.0, 5.0]))
        cases.append(struct.pack("<iiiiiff", 1, n, m, start, cap, dE, dI) + f3.tobytes() + f2.tobytes() + mp.tobytes())
        idx, cnt = R.choose_features_to_add_to_map(f3, f2, mp[:, :3].astype(F32), mp[:, 3:].astype(F32), start, cap, dE, dI)
        want.append(np.concatenate([[cnt, len(idx)], idx]).astype(np.int32))
    for trial in range(8):
        n, s = int(rng.integers(0, 900)), int(rng.integers(0, 900))
        sb3, sb2, _, have2 = _scene(rng, s, n)
        d = float(rng.choice([3.0, 7.5]))
        cases.append(struct.pack("<iiid", 2, n, s, d) + have2.tobytes() + sb2.tobytes())
        add = R.merge_tracked_features(have2, sb2, d)
        want.append(np.concatenate([[n + len(add)], np.arange(n), 1000000 + add]).astype(np.int32))
    for trial in range(8):
        n, nm = int(rng.integers(0, 1200)), int(rng.integers(0, 600))
        f3, f2, _, _ = _scene(rng, n, 0)
        a, b = float(rng.choice([0.01, 0.05])), float(rng.choice([3.0, 6.0]))
        qt = np.stack([rng.integers(0, 500, nm), rng.integers(-1, max(n, 1) + 3, nm)], 1).astype(np.int32)
        cases.append(struct.pack("<iiidd", 3, n, nm, a, b) + f3.tobytes() + f2.tobytes() + qt.tobytes())
        rm = R.remove_too_close_features(f3, f2, a, b)
        stay, mstay = R.erase_too_close(n, rm, qt[:, 1])
        # the surviving matches keep their trainIdx: NOT renumbered to the compacted lists (matcher.cpp:960-963)
        want.append(np.concatenate([[len(rm)], rm, [len(stay)], stay, [len(mstay)], qt[mstay].reshape(-1)]).astype(np.int32))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)) + b"".join(cases))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    pos, bad = 0, []
    for i, w in enumerate(want):
        if raw[pos:pos + len(w)].tobytes() != w.tobytes():
            bad.append(i)
        pos += len(w)
    assert not bad and pos == len(raw), (bad[:10], pos, len(raw))
