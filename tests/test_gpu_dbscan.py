"""DBScan keypoint thinning on the GPU (ps_dbscan.h): ps_dbscan_thin, ps_dbscan_thin_device and the drop-in's ::DBScan equal
the reference's own dbscan.cpp (tests/golden/dbscan_reference.npz) and the numpy restatement (tests/dbscan_ref_py.py) byte for byte."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dbscan_ref_py as R  # noqa: E402
from test_dbscan_ref import golden_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


def _same(a, b):
    return np.asarray(a, np.int32).tobytes() == np.asarray(b, np.int32).tobytes()


def _batch(ctx, frames, eps, mp, ffc, with_octave=True):
    """frames: list of (xy, octave) -> list of kept index arrays through ps_dbscan_thin_device."""
    import torch
    from putslam_amd import device_batch
    F = len(frames)
    cap = max(1, max(len(f[0]) for f in frames))
    xy = np.zeros((F, cap, 2), np.float32)
    oc = np.zeros((F, cap), np.int32)
    cnt = np.zeros(F, np.int32)
    for i, (p, o) in enumerate(frames):
        xy[i, :len(p)] = p
        oc[i, :len(p)] = o
        cnt[i] = len(p)
    dev = torch.device("cuda:0")
    kept, nk = device_batch.dbscan_thin_device(ctx, torch.from_numpy(xy).to(dev), torch.from_numpy(cnt).to(dev),
                                               torch.from_numpy(oc).to(dev) if with_octave else None, eps, mp, ffc)
    torch.cuda.synchronize()
    kept, nk = kept.cpu().numpy(), nk.cpu().numpy()
    return [kept[i, :nk[i]].copy() for i in range(F)]


def test_golden_host_entry(ctx):
    bad = []
    for i, (xy, octave, eps, mp, ffc, kept) in enumerate(golden_cases()):
        if not _same(ctx.dbscan_thin(xy, octave, eps, mp, ffc), kept):
            bad.append((i, len(xy), eps, mp, ffc))
    assert not bad, bad[:10]


def test_golden_device_entry(ctx):
    cs = list(golden_cases())
    groups = {}
    for i, c in enumerate(cs):   # one batch per parameter set (the device entry takes one set per call)
        groups.setdefault((np.float64(c[2]).tobytes(), c[3], c[4]), []).append(i)
    bad = []
    for key, idx in groups.items():
        eps, mp, ffc = cs[idx[0]][2], cs[idx[0]][3], cs[idx[0]][4]
        got = _batch(ctx, [(cs[i][0], cs[i][1]) for i in idx], eps, mp, ffc)
        bad += [i for i, g in zip(idx, got) if not _same(g, cs[i][5])]
    assert not bad, bad[:10]


def _random_frame(rng, n):
    kind = rng.integers(0, 4)
    if kind == 0:
        xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
        dup = rng.random(n) < 0.25
        for i in np.flatnonzero(dup)[np.flatnonzero(dup) > 0]:
            xy[i] = xy[i - 1] + 0.5 * np.array([np.cos(i), np.sin(i)])
    elif kind == 1:
        xy = rng.uniform(0, np.sqrt(n) * rng.choice([0.5, 1.0, 2.0]), (n, 2))
    elif kind == 2:
        c = int(np.ceil(np.sqrt(n)))
        xy = (np.array([(i % c, i // c) for i in range(n)], np.float64) * 0.5)[rng.permutation(n)]
    else:
        xy = np.repeat(rng.uniform(0, 50, ((n + 3) // 4, 2)), 4, 0)[:n] + rng.choice([0.0, 0.3], (n, 1)) * rng.random((n, 2))
    octave = rng.integers(-6, 4, n).astype(np.int32)
    return np.asarray(xy, np.float32).reshape(n, 2), octave


def test_random_sweep_against_restatement(ctx):
    rng = np.random.default_rng(1234)
    bad = []
    sizes = [int(x) for x in rng.choice([0, 1, 2, 5, 17, 33, 64, 100, 257, 700], 140)] + [1500, 2000, 3100, 5000]
    for t, n in enumerate(sizes):
        xy, octave = _random_frame(rng, n)
        eps = float(rng.choice([0.0, 0.5, 1.0, 1.5, 2.0]))
        mp, ffc = int(rng.integers(0, 5)), int(rng.integers(0, 4))
        oc = octave if t % 2 else None
        want = R.dbscan_keep(xy, oc, eps, mp, ffc)
        if not _same(ctx.dbscan_thin(xy, oc, eps, mp, ffc), want):
            bad.append((t, n, eps, mp, ffc))
    assert not bad, bad[:10]


def test_pairs_straddling_the_bound(ctx):
    """Two-point frames whose squared distance lies one ulp below, at and above the square-domain bound, in several directions."""
    from putslam_amd import api
    rng = np.random.default_rng(5)
    for eps in (0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 10.0):
        b = api.dbscan_bound(eps)
        frames = []
        for t in range(64):
            if t < 8:   # on an axis: s = d * d exactly
                d = np.float32(np.sqrt(b))
                d = [np.nextafter(d, np.float32(0)), d, np.nextafter(d, np.float32(np.inf))][t % 3]
                p = np.array([[0, 0], [d, 0] if t < 4 else [0, d]], np.float32)
            else:       # oblique: dy chosen around sqrt(b - dx^2)
                dx = np.float32(rng.uniform(0, eps))
                dy = np.float32(np.sqrt(max(b - float(dx) * float(dx), 0.0)))
                dy = dy if t % 3 == 0 else np.nextafter(dy, np.float32(np.inf if t % 3 == 1 else 0))
                p = np.array([[0, 0], [dx, dy]], np.float32)
            frames.append((p, np.zeros(2, np.int32)))
        got = _batch(ctx, frames, eps, 2, 1)
        want = [R.dbscan_keep(p, None, eps, 2, 1) for p, _ in frames]
        assert all(_same(g, w) for g, w in zip(got, want)), eps
        assert any(len(w) == 1 for w in want) and any(len(w) == 2 for w in want)
        for p, _ in frames:
            assert _same(ctx.dbscan_thin(p, None, eps, 2, 1), R.dbscan_keep(p, None, eps, 2, 1))


@pytest.mark.parametrize("case", ["blob3000", "chain5000", "identical", "nan", "n0", "n1", "octave"])
def test_adversarial(ctx, case):
    rng = np.random.default_rng(11)
    octave = None
    params = [(1.0, 2, 1), (1.0, 2, 2), (1.0, 0, 0), (1.5, 3, 3)]
    if case == "blob3000":
        xy = rng.uniform(0, 0.7, (3000, 2))
    elif case == "chain5000":
        xy = np.stack([np.arange(5000) * 0.9, np.zeros(5000)], 1)
    elif case == "identical":
        xy = np.full((1000, 2), 3.25)
    elif case == "nan":
        xy = rng.uniform(0, 3, (200, 2))
        xy[rng.random(200) < 0.2, rng.integers(0, 2)] = np.nan
        xy[5] = [np.inf, 1.0]
    elif case == "n0":
        xy = np.zeros((0, 2))
    elif case == "n1":
        xy = np.array([[1.0, 2.0]])
    else:
        xy = rng.uniform(0, 5, (300, 2))
        octave = np.where(rng.random(300) < 0.3, -5, 1).astype(np.int32)
    xy = np.asarray(xy, np.float32)
    for eps, mp, ffc in params:
        want = R.dbscan_keep(xy, octave, eps, mp, ffc)
        assert _same(ctx.dbscan_thin(xy, octave, eps, mp, ffc), want), (case, eps, mp, ffc)


def test_strided_host_input(ctx):
    """xy / octave read with byte strides (the pt / octave fields of a cv::KeyPoint array: 28 bytes apart)."""
    rng = np.random.default_rng(3)
    kp = np.zeros(800, dtype=[("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                              ("octave", "<i4"), ("class_id", "<i4")])
    xy, octave = _random_frame(rng, 800)
    kp["x"], kp["y"], kp["octave"] = xy[:, 0], xy[:, 1], octave
    raw = kp.view(np.float32).reshape(800, 7)
    got = ctx.dbscan_thin(raw[:, 0:2], kp["octave"], 1.0, 2, 1)
    assert _same(got, R.dbscan_keep(xy, octave, 1.0, 2, 1))


def test_ragged_batch_equals_single_calls_and_repeats(ctx):
    rng = np.random.default_rng(99)
    frames = [_random_frame(rng, int(n)) for n in rng.integers(0, 2001, 500)]
    got = _batch(ctx, frames, 1.0, 2, 1)
    for i in range(0, 500, 1):
        assert _same(got[i], ctx.dbscan_thin(frames[i][0], frames[i][1], 1.0, 2, 1)), i
    for i in range(0, 500, 50):
        assert _same(got[i], R.dbscan_keep(frames[i][0], frames[i][1], 1.0, 2, 1)), i
    for _ in range(2):
        again = _batch(ctx, frames, 1.0, 2, 1)
        assert all(_same(a, b) for a, b in zip(got, again))


def test_bad_arguments(ctx):
    from putslam_amd import api
    with pytest.raises(api.PsError) as e:
        ctx.dbscan_thin(np.zeros((8001, 2), np.float32))
    assert e.value.code == -1 and "PS_DBSCAN_MAX_KPTS" in str(e.value)
    with pytest.raises(api.PsError):
        ctx.dbscan_thin_device(0, 0, 0, 1, 8001, 0, 0)


def test_counts_outside_capacity_mark_the_frame(ctx):
    import torch
    from putslam_amd import device_batch
    dev = torch.device("cuda:0")
    xy = torch.zeros((3, 16, 2), dtype=torch.float32, device=dev)
    cnt = torch.tensor([4, 17, -1], dtype=torch.int32, device=dev)
    kept, nk = device_batch.dbscan_thin_device(ctx, xy, cnt, None, 1.0, 2, 1)
    torch.cuda.synchronize()
    assert nk.cpu().tolist() == [1, -1, -1] and kept[0, 0].item() == 0


def _write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for xy, octave, eps, mp, ffc in cs:
            f.write(struct.pack("<idii", len(xy), eps, mp, ffc))
            f.write(np.ascontiguousarray(xy, np.float32).tobytes())
            f.write(np.ascontiguousarray(octave, np.int32).tobytes())


def test_dropin_dbscan_equals_golden(tmp_path):
    """::DBScan through a program compiled here against the drop-in (linked as build_dropin links its test programs)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_dropin()
    lib = os.path.join(ROOT, "putslam_amd")
    exe = str(tmp_path / "test_dbscan_dropin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(lib, "csrc", "dropin"), os.path.join(HERE, "cpp", "test_dbscan_dropin.cpp"), "-o", exe,
                           "-L", lib, "-lputslam_dropin", "-lputslam_hip", "-Wl,-rpath," + lib])
    cs = list(golden_cases())
    _write_cases(str(tmp_path / "in.bin"), [c[:5] for c in cs])
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    pos, bad = 0, []
    for i, c in enumerate(cs):
        k = int(raw[pos])
        if not _same(raw[pos + 1:pos + 1 + k], c[5]):
            bad.append(i)
        pos += 1 + k
    assert pos == len(raw) and not bad, bad[:10]


def test_largest_frame(ctx):
    """n = capacity = PS_DBSCAN_MAX_KPTS: the most dynamic LDS the kernel asks for (20 bytes a point), through both entries."""
    rng = np.random.default_rng(8000)
    n = 8000
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(np.float32)
    near = np.flatnonzero(rng.random(n) < 0.3)
    near = near[near > 0]
    xy[near] = xy[near - 1] + np.float32(0.5)
    xy[:200] = rng.uniform(0, 6, (200, 2)).astype(np.float32)          # one large component, replayed cooperatively
    octave = np.where(rng.random(n) < 0.05, -5, 0).astype(np.int32)
    for eps, mp, ffc in ((1.0, 2, 1), (1.5, 3, 2)):
        want = R.dbscan_keep(xy, octave, eps, mp, ffc)
        assert _same(ctx.dbscan_thin(xy, octave, eps, mp, ffc), want), (eps, mp, ffc)
        got = _batch(ctx, [(xy, octave), (xy[:7000], octave[:7000])], eps, mp, ffc)
        assert _same(got[0], want) and _same(got[1], R.dbscan_keep(xy[:7000], octave[:7000], eps, mp, ffc))
