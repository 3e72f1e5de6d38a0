"""Slices of the front end's randomised soak (tests/fuzz_front_end.py) collected under `-m gpu`: per family two seeds of drawn
shapes, windows, grids, level counts, thresholds, strides and counts, device against restatement byte for byte.  What each slice
reaches is asserted on the restatements alone, over the same draws, in tests/test_fuzz_front_end_host.py."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_front_end as Z  # noqa: E402


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_klt_slice(ctx, seed):
    """Every stored pyramid level, nextPts / status / err per pair and the selection on the result, over windows of all three
    classes of W cn against the wave width.  The same draws: tests/test_fuzz_front_end_host.py::test_klt_slice."""
    assert Z.run_klt(Z.SLICE_DRAWS["klt"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_fast_slice(ctx, seed):
    """The grey / score / corner maps and the lists.  The same draws: tests/test_fuzz_front_end_host.py::test_fast_slice."""
    assert Z.run_fast(Z.SLICE_DRAWS["fast"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_orb_detect_slice(ctx, seed):
    """Every output column, and the levels of every ROI where they are few.  The same draws:
    tests/test_fuzz_front_end_host.py::test_orb_detect_slice."""
    assert Z.run_orb_detect(Z.SLICE_DRAWS["orb_detect"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_orb_describe_slice(ctx, seed):
    """Every plane of every slot, desc, keptIdx and numKept.  The same draws:
    tests/test_fuzz_front_end_host.py::test_orb_describe_slice."""
    assert Z.run_orb_describe(Z.SLICE_DRAWS["orb_describe"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_merge_slice(ctx, seed):
    """srcIdx, the closed rows, desc and refill of ps_track_close_pairs over tracked and candidate counts on both sides of the
    tile seams.  The same draws: tests/test_fuzz_front_end_host.py::test_merge_slice."""
    assert Z.run_merge(Z.SLICE_DRAWS["merge"], seed, ctx=ctx, verbose=False) == 0
