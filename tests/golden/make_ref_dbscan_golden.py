"""tests/golden/dbscan_reference.npz: the reference's own DBScan (src/Matcher/dbscan.cpp of the reference tree) on chosen keypoint
sets.  The reference source is compiled into a temporary directory against a two-name OpenCV shim (dbscan_shim/Defs/opencv.h)
and driven by dbscan_shim/dbscan_harness.cpp; nothing compiled is kept.  Tests read only the .npz.

    python tests/golden/make_ref_dbscan_golden.py [/path/to/reference]

Re-running it reproduces the committed arrays (the cases come from a fixed seed)."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dbscan_reference.npz")


def _uniform_with_dupes(rng, n, w=640.0, h=480.0, frac=0.25, off=0.5):
    """Uniform in w x h; about `frac` of the points sit `off` px from their predecessor (the bench frames' kind of data)."""
    xy = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32)
    for i in range(1, n):
        if rng.random() < frac:
            a = rng.uniform(0, 2 * np.pi)
            xy[i] = xy[i - 1] + np.float32(off) * np.array([np.cos(a), np.sin(a)], np.float32)
    return xy


def _small_case(rng, kind, n):
    if kind == 0:   # dense box: many neighbours at eps 1 .. 2
        s = rng.choice([2.0, 4.0, 8.0])
        xy = rng.uniform(0, s, (n, 2))
    elif kind == 1:  # 0.5-px grid: distances of exactly eps = 0.5 / 1 / 1.5
        c = max(1, int(np.ceil(np.sqrt(n))))
        g = np.array([(i % c, i // c) for i in range(n)], np.float64) * 0.5
        xy = g[rng.permutation(n)] + rng.choice([0.0, 100.0])
    elif kind == 2:  # chain with steps around eps
        steps = rng.choice([0.5, 0.9, 1.0, 1.5], n)
        xy = np.stack([np.cumsum(steps), np.zeros(n)], 1)
        xy = xy[rng.permutation(n)] if rng.random() < 0.5 else xy
    elif kind == 3:  # duplicates and near duplicates
        base = rng.uniform(0, 6, (max(1, n // 3), 2))
        xy = base[rng.integers(0, len(base), n)] + rng.choice([0.0, 0.25], (n, 1)) * rng.standard_normal((n, 2))
    else:            # sparse clumps
        xy = _uniform_with_dupes(rng, n, 20.0, 20.0, 0.4)
    xy = np.asarray(xy, np.float32).reshape(n, 2)
    if n and rng.random() < 0.1:
        xy[rng.integers(0, n)] = np.nan
    octave = rng.integers(0, 4, n).astype(np.int32)
    if n and rng.random() < 0.3:
        octave[rng.random(n) < 0.15] = -5
    return xy, octave


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    eps_set = [0.0, 0.5, 1.0, 1.5, 2.0]
    for c in range(320):
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 13, 21, 34, 48, 64]))
        xy, octave = _small_case(rng, c % 5, n)
        eps = float(rng.choice(eps_set)) if c % 16 else float(rng.choice([-1.0, np.nan, np.inf, 10.0, 0.75]))
        out.append((xy, octave, eps, int(rng.integers(0, 5)) if c % 11 else int(rng.integers(-2, 1)),
                    int(rng.integers(0, 4)) if c % 13 else -1))
    for n, reps in ((500, 6), (1000, 3), (2000, 3)):
        for r in range(reps):
            xy = _uniform_with_dupes(rng, n)
            octave = rng.integers(0, 8, n).astype(np.int32)
            out.append((xy, octave, [1.0, 1.5, 2.0, 10.0, 0.5, 1.0][r], [2, 1, 3, 2, 0, 4][r], [1, 2, 1, 3, 1, 0][r]))
    xy = _uniform_with_dupes(rng, 5000)
    out.append((xy, rng.integers(0, 8, 5000).astype(np.int32), 1.0, 2, 1))
    blob = rng.uniform(0, 0.7, (3000, 2)).astype(np.float32)                        # every pair are neighbours at eps 1
    out.append((blob, np.zeros(3000, np.int32), 1.0, 2, 2))
    chain = np.stack([np.arange(5000) * 0.9, np.zeros(5000)], 1).astype(np.float32)  # one long 0.9-px chain
    out.append((chain, np.zeros(5000, np.int32), 1.0, 2, 1))
    return out


def run_reference(ref_root, cs):
    src = os.path.join(ref_root, "src", "Matcher", "dbscan.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dbscan_harness")
        subprocess.check_call(["g++", "-O3", "-DNDEBUG", "-ffp-contract=off", "-std=c++11", "-I", os.path.join(HERE, "dbscan_shim"),
                               "-I", os.path.join(ref_root, "include"), os.path.join(HERE, "dbscan_shim", "dbscan_harness.cpp"),
                               src, "-o", exe])
        inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<i", len(cs)))
            for xy, octave, eps, mp, ffc in cs:
                f.write(struct.pack("<idii", len(xy), eps, mp, ffc))
                f.write(np.ascontiguousarray(xy, np.float32).tobytes())
                f.write(np.ascontiguousarray(octave, np.int32).tobytes())
        subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL)
        raw = np.fromfile(outp, np.int32)
    kept, pos = [], 0
    for _ in cs:
        k = int(raw[pos])
        kept.append(raw[pos + 1:pos + 1 + k].copy())
        pos += 1 + k
    assert pos == len(raw)
    return kept


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cs = cases()
    kept = run_reference(ref_root, cs)
    offs = np.cumsum([0] + [len(c[0]) for c in cs]).astype(np.int64)
    koffs = np.cumsum([0] + [len(k) for k in kept]).astype(np.int64)
    np.savez_compressed(OUT, xy=np.concatenate([c[0] for c in cs]).astype(np.float32),
                        octave=np.concatenate([c[1] for c in cs]).astype(np.int32), offsets=offs,
                        eps=np.array([c[2] for c in cs], np.float64), min_pts=np.array([c[3] for c in cs], np.int32),
                        features_from_cluster=np.array([c[4] for c in cs], np.int32),
                        kept=np.concatenate(kept).astype(np.int32), kept_offsets=koffs)
    print("%s: %d cases, %d keypoints, %d bytes" % (OUT, len(cs), offs[-1], os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
