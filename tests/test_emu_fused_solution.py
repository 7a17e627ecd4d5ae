"""The fused residual update + restriction for solves that carry the solution (csgpu_opts.fused_restrict = 1), on the CPU
emulator build of the kernel sources: see helpers_fused_solution.py."""
import numpy as np
import pytest

import helpers_fused_solution as hf

SHAPES = ((31, 200), (64, 57))


@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape,check_every", ((SHAPES[0], 1), (SHAPES[0], 4), (SHAPES[1], 1)))
def test_pair_voltages_and_current_maps(emu_lib, shape, check_every, batch):
    """blocks 1 and 2: direct launches and captured chunks on the first shape; branch currents on the smallest"""
    hf.check_pairs_voltages(emu_lib, shape, batch, check_every)
    hf.check_pairs_currents(emu_lib, shape, batch, check_every, branch=(shape == SHAPES[1] and batch == 16))


@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_right_hand_sides(emu_lib, shape, batch):
    """block 3"""
    hf.check_rhs(emu_lib, shape, batch)


@pytest.mark.parametrize("batch", (16, 32))
@pytest.mark.parametrize("shape", SHAPES)
def test_finite_grounds_with_and_without_dirichlet_sets(emu_lib, shape, batch):
    """block 4"""
    hf.check_finite_grounds(emu_lib, shape, batch)


def test_single_precision(emu_lib):
    """block 5"""
    hf.check_pairs_voltages(emu_lib, (64, 57), 32, dtype=np.float32)
    hf.check_pairs_currents(emu_lib, (64, 57), 32, dtype=np.float32)


def test_mixed_precision_stays_two_pass(emu_lib):
    """block 6"""
    hf.check_mixed_precision_stays_two_pass(emu_lib, (64, 57), 16)


def test_polishing_with_the_solution_carried(emu_lib):
    """block 7"""
    hf.check_polishing(emu_lib)


def test_true_residual_criterion(emu_lib):
    """block 8"""
    hf.check_true_residual_criterion(emu_lib)


def test_enriched_level(emu_lib):
    """block 9"""
    hf.check_enriched_level(emu_lib)


def test_default_is_unchanged(emu_lib):
    """block 10"""
    hf.check_default_unchanged(emu_lib)
