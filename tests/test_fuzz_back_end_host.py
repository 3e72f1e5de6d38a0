"""What the slices of tests/test_gpu_fuzz_back_end_slice.py reach, shown on the restatements alone: the draws of
tests/fuzz_back_end.py (SLICE_SEEDS x SLICE_DRAWS, the very draws the GPU tests make) run through patches_ref, uncertainty_ref and
frame_assembly_ref, and the conditions a slice must meet to be worth its GPU time asserted on the results -- every class of patch
size against the wave and the work-group, every status, every neighbour count, gradient branch and tie, lists on both sides of
the scan's tiles, every trainIdx outside the frame on an inlier.

Named MUTANTS of the restatements -- test-only code, no kernel is touched -- state the errors the slices were built to catch: each
must differ from the restatement on at least one draw of every slice.  A mutant that no draw separates means the draws are too
tame.

The restatement time of every slice is printed and held below that of the front end's klt slice, measured in the same run.  No
GPU."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fuzz_back_end as Z  # noqa: E402
import fuzz_front_end as FE  # noqa: E402
import patches_ref as R  # noqa: E402
import uncertainty_ref as U  # noqa: E402

SEEDS = Z.SLICE_SEEDS
REDRAW_CAP = 10          # at most one redraw in this many draws: the front end's cap


@pytest.fixture(scope="module")
def klt_seconds():
    """What test_fuzz_front_end_host.py::test_klt_slice spends on its restatement, here and now (the slower of its two seeds would
    be the laxer bound: the faster one is taken)"""
    best = None
    for seed in FE.SLICE_SEEDS:
        t0 = time.perf_counter()
        for cfg in FE.slice_draws("klt", seed):
            FE.klt_reference(cfg)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def timed(family, seed, klt_seconds, seconds):
    print("%s slice, seed %d: restatement %.2f s (the klt slice: %.2f s)" % (family, seed, seconds, klt_seconds))
    assert seconds <= klt_seconds, (family, seed, seconds, klt_seconds)


def test_the_slices_are_what_the_issue_starts_from():
    assert Z.SLICE_SEEDS == (11, 2026) and Z.FAMILIES == ("patches", "uncertainty", "edges", "assemble") == tuple(Z.SLICE_DRAWS)
    for family in Z.FAMILIES:     # a draw is plain data and the same every time
        a, b = Z.slice_draws(family, 3, 4), Z.slice_draws(family, 3, 4)
        assert repr(a) == repr(b) and all(isinstance(d, dict) and "redraws" in d for d in a)


def test_the_patch_classes_cover_every_legal_size():
    sizes = list(range(3, 32, 2))
    assert sorted(s for members in Z.PATCH_CLASSES.values() for s in members) == sizes
    for cls, members in Z.PATCH_CLASSES.items():
        assert all(Z.patch_class(ps) == cls for ps in members), cls
    # patch_block_waves as ps_patches_rule.h states it: 31 x 31 takes 26 992 bytes, two such waves share 64 KiB
    assert Z.patch_wave_bytes(31) == 26992 and [Z.patch_block_waves(ps) for ps in (3, 23, 25, 27, 29, 31)] == [4, 4, 3, 3, 2, 2]
    assert 7 * 7 < 64 < 9 * 9
    for cap in Z.PATCH_CAPS:          # the index rule reaches every point once, whatever the class
        for waves in (2, 3, 4):
            for n in (0, 1, cap - 1, cap):
                assert Z.points_reached(cap, n, waves) == list(range(n))


# ------------------------------------------------------------------------------------------------------------------ patches
@pytest.mark.parametrize("seed", SEEDS)
def test_patches_slice(seed, klt_seconds):
    draws = Z.slice_draws("patches", seed)
    t0 = time.perf_counter()
    wants = []
    for cfg in draws:
        inp = Z.patches_inputs(cfg)
        wants.append((inp, Z.patches_reference(cfg, inp)))
    seconds = time.perf_counter() - t0
    classes, residues, status, shapes = {}, {3: set(), 4: set()}, set(), set()
    several = ran_out = no_legal = four_for_three = past_count = 0
    for cfg, (inp, want) in zip(draws, wants):
        cls = tuple(cfg["cls"])
        assert cls == Z.patch_class(cfg["ps"])
        classes[cls] = classes.get(cls, 0) + 1
        if cls[0] in residues:
            residues[cls[0]].add(cfg["cap"] % cls[0])
        shapes.add(cfg["shape"])
        h = R.half(cfg["ps"])
        no_legal += cfg["rows"] < 2 * h + 3 or cfg["cols"] < 2 * h + 3
        if cfg["rows"] < 2 * h + 3 or cfg["cols"] < 2 * h + 3:
            assert all((w["status"] == R.OLD_TAPS_OUTSIDE).all() for w in want)
        wrong_waves = past = False
        for p, w in enumerate(want):
            status |= set(w["status"].tolist())
            several += bool((w["iterations"] > 1).any())
            ran_out += bool(cfg["max_iter"] == 50 and ((w["iterations"] == 50) & (w["status"] == R.MAX_ITERATIONS)).any())
            n, c = w["n"], cfg["counts"][p]
            assert Z.points_reached(cfg["cap"], c, cls[0]) == list(range(n))
            # MUTANT: the point index built with 4 waves in a work-group that has 3
            wrong_waves |= cls[0] == 3 and Z.points_reached(cfg["cap"], c, 3, index_waves=4) != list(range(n))
            # MUTANT: `i > n` in place of `i >= n` (the row at the count is written, or the next pair's first row)
            past |= Z.points_reached(cfg["cap"], c, cls[0], past=True) != list(range(n))
        four_for_three, past_count = four_for_three + wrong_waves, past_count + past
    print("patches", seed, "classes", classes, "cap % waves", residues, "status", sorted(status), "several iterations", several, "maxIter 50 run out",
          ran_out, "no legal point", no_legal, "mutants: 4 waves for 3:", four_for_three, "i > n:", past_count)
    assert set(classes) == set(Z.PATCH_CLASSES) and min(classes.values()) >= 3, classes
    assert residues[3] == {0, 1, 2} and residues[4] == {0, 1, 2, 3}, residues
    assert status == set(range(7)), status
    assert several >= 1 and ran_out >= 1 and no_legal >= 1
    assert shapes == set(Z.PATCH_SHAPES)
    assert four_for_three >= 1 and past_count >= 1
    assert REDRAW_CAP * sum(d["redraws"] for d in draws) <= len(draws)
    timed("patches", seed, klt_seconds, seconds)


# -------------------------------------------------------------------------------------------------------------- uncertainty
def float_division(x, y, depth, K, scale):
    """MUTANT of uncertainty_ref.point2Dto3D: the depth divided in float"""
    x, y = np.float32(x), np.float32(y)
    rows, cols = depth.shape
    off = U.round_size(x, cols) + U.round_size(y, rows) * cols
    dv = int(depth[off // cols, off % cols]) if off < rows * cols else 0
    Z_ = np.float32(np.float32(dv) / np.float32(scale))
    u = (x - np.float32(K[2])) / np.float32(K[0])
    v = (y - np.float32(K[5])) / np.float32(K[4])
    return u * Z_, v * Z_, Z_


def rows_differ(a, b):
    """two lists of per-set results (None or dicts of arrays) differ somewhere"""
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return True
        if x is not None and any(x[m].tobytes() != y[m].tobytes() for m in x):
            return True
    return False


@pytest.mark.parametrize("seed", SEEDS)
def test_uncertainty_slice(seed, klt_seconds, monkeypatch):
    draws = Z.slice_draws("uncertainty", seed)
    U.SEEN.clear()
    t0 = time.perf_counter()
    wants = []
    for cfg in draws:
        inp = Z.uncertainty_inputs(cfg)
        wants.append((inp, Z.uncertainty_reference(cfg, inp)))
    seconds = time.perf_counter() - t0
    seen = dict(U.SEEN)
    outside_depth = outside_images = below = above = finite = non_finite = bound_mutant = 0
    for cfg, (inp, want) in zip(draws, wants):
        D, I = cfg["depth_frames"], cfg["image_frames"]
        live = [(n, g) for n, g in zip(cfg["counts"], cfg["image_frame"]) if 0 < n <= cfg["cap"]]
        outside_depth += any(not 0 <= g < D for _, g in live)
        outside_images += Z.images_passed(cfg) and any(I <= g < D for _, g in live)
        below, above = below + any(0 < n < 256 for n, _ in live), above + any(n > 256 for n, _ in live)
        for w in want:
            if w is not None and "info" in w and len(w["info"]):
                ok = np.isfinite(w["info"]).all(axis=1)
                finite, non_finite = finite + bool(ok.any()), non_finite + bool((~ok).any())
        # MUTANT: the image set's bound ignored (`frame < a.iFrames` of unc_row)
        bound_mutant += rows_differ(want, Z.uncertainty_reference(cfg, inp, image_bound=False))
    # MUTANT: the depth division done in float32 (it shows where the scale is no float)
    division_mutant = 0
    monkeypatch.setattr(U, "point2Dto3D", float_division)
    for cfg, (inp, want) in zip(draws, wants):
        if float(np.float32(cfg["scale"])) != cfg["scale"]:
            division_mutant += rows_differ(want, Z.uncertainty_reference(cfg, inp, variant="float division"))
    monkeypatch.undo()
    models, subsets = {d["model"] for d in draws}, {tuple(d["outs"]) for d in draws}
    print("uncertainty", seed, seen, "outside the depth set", outside_depth, "outside a shorter image set", outside_images, "counts below / above 256",
          below, above, "info finite / not", finite, non_finite, "mutants: image bound", bound_mutant, "float division", division_mutant)
    for k in range(9):
        assert seen.get(("kept", k), 0) > 0, (k, seen)
    for b in ("border", "end-beg", "cen-beg", "end-cen", "fallback"):
        assert seen.get(("branch", b), 0) > 0, (b, seen)
    for t in U.TIE_CASES:
        assert seen.get(("tie", t[0], t[1]), 0) > 0, (t, seen)
    assert seen.get("bad pixel", 0) > 0
    assert outside_depth >= 1 and outside_images >= 1 and below >= 1 and above >= 1
    assert models == {-1, 0, 1, 2} and len(subsets) >= 5, (models, subsets)
    assert finite >= 1 and non_finite >= 1
    assert any(d["rows"] <= 3 or d["cols"] <= 3 for d in draws)
    assert bound_mutant >= 1 and division_mutant >= 1
    assert REDRAW_CAP * sum(d["redraws"] for d in draws) <= len(draws)
    timed("uncertainty", seed, klt_seconds, seconds)


# -------------------------------------------------------------------------------------------------------------------- edges
def without_carry(idx, tile=Z.EDGE_TILE):
    """MUTANT of the compaction: the running offset not carried from tile to tile -- every tile's inliers land on the first rows.
    idx: the ascending inlier indices of a list; returns what the first rows then hold"""
    rows = []
    for t in sorted(set((idx // tile).tolist())):
        part = idx[idx // tile == t].tolist()
        rows[:len(part)] = part
    return rows


def edges_differ(cfg, a, b):
    names = [Z.EDGE_NAMES.get(n, n) for n in cfg["outs"]]
    return any(x[n] is not y[n] and np.asarray(x[n]).tobytes() != np.asarray(y[n]).tobytes() for x, y in zip(a, b) for n in names if n in x)


@pytest.mark.parametrize("seed", SEEDS)
def test_edges_slice(seed, klt_seconds):
    draws = Z.slice_draws("edges", seed)
    t0 = time.perf_counter()
    wants = []
    for cfg in draws:
        inp = Z.edges_inputs(cfg)
        wants.append((inp, Z.edges_reference(cfg, inp)))
    seconds = time.perf_counter() - t0
    counts, first_tile_empty, outside_pair, none, too_many, carry_mutant, follow_mutant = set(), 0, 0, 0, 0, 0, 0
    planted = set()
    for cfg, (inp, want) in zip(draws, wants):
        cap, M = cfg["max_kpts"], cfg["max_matches"]
        outside_pair += any(not (0 <= v < cfg["views"] and 0 <= f < cfg["frames"]) for v, f in cfg["pairs"])
        none, too_many = none + any(m <= 0 for m in cfg["num_matches"]), too_many + any(m > M for m in cfg["num_matches"])
        carry = False
        for p, w in enumerate(want):
            if not Z.edge_pair_valid(cfg, p):
                assert w["count"] == 0
                continue
            counts.add(w["count"])
            idx = np.flatnonzero(inp["mask"][p, :cfg["num_matches"][p]])
            assert len(idx) == w["count"]
            first_tile_empty += bool(len(idx) and idx[0] >= Z.EDGE_TILE)
            carry |= bool(cfg["outs"]) and without_carry(idx) != idx.tolist()
        carry_mutant += carry
        for p, k, t in inp["planted"]:
            assert want[p]["curRow"][k] == t and np.isnan(want[p]["uv"][k]).all() and (want[p]["position"][k].view(np.uint64) == U.NAN_BITS).all()
            assert all((want[p][m][k].view(np.uint64) == U.NAN_BITS).all() for m in Z.MEMBERS if m in want[p])
            planted.add(t if t in (-1, Z.INT32_MIN, Z.INT32_MAX) else "maxKpts")
        # MUTANT: `trainIdx <= maxKpts` followed -- the frames have one row more, and the index maxKpts reads it
        if any(t == cap for _, _, t in inp["planted"]):
            more = lambda a: np.concatenate([a, np.ones_like(a[:, :1])], axis=1)   # noqa: E731
            images = inp["imgs"] if Z.images_passed(cfg) else None
            mutant = U.measurement_edges(inp["matches"], inp["num"], inp["mask"], cfg["pairs"], cfg["views"], more(inp["pts"][:cfg["frames"]]),
                                         more(inp["xyu"]), cfg["image_frame"], inp["deps"], images, np.array(cfg["K"], np.float32), cfg["scale"],
                                         U.sensor(**cfg["sensor"]), cfg["model"], M, want=tuple(m for m in Z.MEMBERS if m in cfg["outs"]))
            follow_mutant += edges_differ(cfg, want, mutant)
    print("edges", seed, "inlier counts", sorted(counts), "first tile empty", first_tile_empty, "pair outside", outside_pair, "numMatches <= 0", none,
          "numMatches > maxMatches", too_many, "trainIdx outside", planted, "mutants: no carry", carry_mutant, "trainIdx <= maxKpts", follow_mutant)
    assert 0 in counts and 1 in counts and any(256 < c <= 512 for c in counts) and any(c > 512 for c in counts), sorted(counts)
    assert first_tile_empty >= 1 and outside_pair >= 1 and none >= 1 and too_many >= 1
    assert planted == {-1, "maxKpts", Z.INT32_MIN, Z.INT32_MAX}, planted
    assert any("count" not in d["outs"] for d in draws) and any(not set(d["outs"]) - {"count"} for d in draws)      # count NULL; no member
    assert carry_mutant >= 1 and follow_mutant >= 1
    assert REDRAW_CAP * sum(d["redraws"] for d in draws) <= len(draws)
    timed("edges", seed, klt_seconds, seconds)


# ----------------------------------------------------------------------------------------------------------------- assemble
def count_class(c, cap):
    return "cap + 1" if c == cap + 1 else ("cap" if c == cap else c)


@pytest.mark.parametrize("seed", SEEDS)
def test_assemble_slice(seed, klt_seconds, oracle):
    draws = Z.slice_draws("assemble", seed)
    t0 = time.perf_counter()
    wants = []
    for cfg in draws:
        inp = Z.assemble_inputs(cfg)
        wants.append((inp, Z.assemble_reference(cfg, oracle, inp)))
    seconds = time.perf_counter() - t0
    classes, gather_classes, distorted, next_row, outside, repeats = set(), set(), 0, 0, 0, 0
    for cfg, (inp, ((g, gcounts), frames)) in zip(draws, wants):
        assert np.isfinite(cfg["K"]).all() and cfg["K"][0] > 0 and cfg["K"][4] > 0          # the premise
        classes |= {count_class(c, cfg["cap"]) for c in cfg["counts"]}
        gather_classes |= {count_class(c, cfg["cap"]) for c in cfg["gather_counts"]}
        distorted += any(cfg["dist5"])
        repeats += cfg["kept"] == "repeats"
        rows, cols = cfg["rows"], cfg["cols"]
        for w in frames:
            if w is None or not len(w["pts"]):
                continue
            und = w["xy_undist"][np.isfinite(w["xy_undist"]).all(axis=1)]
            ru = np.array([oracle.round_size(u, cols) for u in und[:, 0]])
            rv = np.array([oracle.round_size(v, rows) for v in und[:, 1]])
            next_row += bool(((ru == cols) & (rv < rows - 1)).any())
            outside += bool(((und[:, 0] < 0) | (und[:, 1] < 0) | (rv == rows) | ((ru == cols) & (rv >= rows - 1))).any())
    print("assemble", seed, "count classes", classes, gather_classes, "distorted", distorted, "next row read", next_row, "outside", outside)
    every = {0, 1, 63, 64, 65, -1, "cap", "cap + 1"}
    assert classes == every and gather_classes == every, (classes, gather_classes)
    assert distorted >= 1 and distorted < len(draws) and next_row >= 1 and outside >= 1 and 0 < repeats < len(draws)
    assert REDRAW_CAP * sum(d["redraws"] for d in draws) <= len(draws)
    timed("assemble", seed, klt_seconds, seconds)
