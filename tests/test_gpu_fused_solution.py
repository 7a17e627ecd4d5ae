"""The fused residual update + restriction for solves that carry the solution (csgpu_opts.fused_restrict = 1), on the device:
see helpers_fused_solution.py. (700, 333): many strips and column segments, the XCD-aware tile walk."""
import numpy as np
import pytest

import helpers_fused_solution as hf

SHAPES = ((31, 200), (64, 57), (101, 130), (700, 333))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_voltages_and_current_maps_gpu(gpu_lib, shape, batch):
    """blocks 1 and 2: direct launches everywhere, captured chunks on the first shape, branch currents on the smallest"""
    for ce in ((1, 4) if shape == SHAPES[0] else (1,)):
        hf.check_pairs_voltages(gpu_lib, shape, batch, ce)
        hf.check_pairs_currents(gpu_lib, shape, batch, ce, branch=(shape == SHAPES[1] and batch == 16))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_right_hand_sides_gpu(gpu_lib, shape, batch):
    """block 3"""
    hf.check_rhs(gpu_lib, shape, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_finite_grounds_with_and_without_dirichlet_sets_gpu(gpu_lib, shape, batch):
    """block 4"""
    hf.check_finite_grounds(gpu_lib, shape, batch)


@pytest.mark.gpu
def test_single_precision_gpu(gpu_lib):
    """block 5"""
    hf.check_pairs_voltages(gpu_lib, (101, 130), 32, dtype=np.float32)
    hf.check_pairs_currents(gpu_lib, (101, 130), 32, dtype=np.float32)


@pytest.mark.gpu
def test_mixed_precision_stays_two_pass_gpu(gpu_lib):
    """block 6"""
    hf.check_mixed_precision_stays_two_pass(gpu_lib, (101, 130), 16)
    hf.check_mixed_precision_stays_two_pass(gpu_lib, (64, 57), 32)


@pytest.mark.gpu
def test_polishing_with_the_solution_carried_gpu(gpu_lib):
    """block 7"""
    hf.check_polishing(gpu_lib)


@pytest.mark.gpu
def test_true_residual_criterion_gpu(gpu_lib):
    """block 8"""
    hf.check_true_residual_criterion(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (16, 32))
def test_enriched_level_gpu(gpu_lib, batch):
    """block 9"""
    hf.check_enriched_level(gpu_lib, batch=batch)


@pytest.mark.gpu
def test_default_is_unchanged_gpu(gpu_lib):
    """block 10"""
    hf.check_default_unchanged(gpu_lib)
