"""Slices of the back end's randomised soak (tests/fuzz_back_end.py) collected under `-m gpu`: per family two seeds of drawn patch
sizes, image shapes, paddings, cameras, depth scales, sensors, counts, masks and output subsets, device against restatement byte
for byte.  What each slice reaches, and that it separates named mutants of the restatements, is asserted on the restatements
alone, over the same draws, in tests/test_fuzz_back_end_host.py."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_back_end as Z  # noqa: E402


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_patches_slice(ctx, seed):
    """Positions, status, iterations and every model array of ps_patch_align -- fused with and without the model written, and on
    the model ps_patch_models left -- over patch sizes of every class of waves per work-group, capacities of every remainder
    against them and images down to one that holds no patch.  The same draws: tests/test_fuzz_back_end_host.py::test_patches_slice."""
    assert Z.run_patches(Z.SLICE_DRAWS["patches"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_uncertainty_slice(ctx, seed):
    """The normal, the gradient and the information matrix of every row of ps_feature_uncertainty over drawn scenes, cameras, depth
    scales, sensors, paddings, counts and output subsets.  The same draws: tests/test_fuzz_back_end_host.py::test_uncertainty_slice."""
    assert Z.run_uncertainty(Z.SLICE_DRAWS["uncertainty"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_edges_slice(ctx, seed):
    """count, mapRow, curRow, uv, position and the three members of ps_measurement_edges over list lengths on both sides of the
    scan's tiles, masks empty to full, pairs and trainIdx outside their sets, and output subsets down to none.  The same draws:
    tests/test_fuzz_back_end_host.py::test_edges_slice."""
    assert Z.run_edges(Z.SLICE_DRAWS["edges"], seed, ctx=ctx, verbose=False) == 0


@pytest.mark.parametrize("seed", Z.SLICE_SEEDS)
def test_fuzz_assemble_slice(ctx, oracle, seed):
    """ps_gather_keypoints against numpy's gather and ps_assemble_frames on its blocks against the oracle, over drawn cameras,
    distortions, depth scales, paddings, counts and index lists.  The same draws: tests/test_fuzz_back_end_host.py::test_assemble_slice."""
    assert Z.run_assemble(Z.SLICE_DRAWS["assemble"], seed, ctx=ctx, verbose=False, oracle=oracle) == 0
