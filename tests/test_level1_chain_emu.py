"""The chained level-1 pass (csgpu_opts.fused_level1 = 2) and the first CG product of a batch without the old search
direction, on the emulator build of the kernel sources: the checks of level1_chain_checks.py; the device twin is
test_level1_chain_gpu.py."""
import numpy as np
import pytest

import level1_chain_checks as lc


@pytest.mark.parametrize("batch", [16, 32])
@pytest.mark.parametrize("name", ["one_tile", "residue0", "thin_wide", "thin_tall"])
def test_chained_level1_equals_two_launches(emu_lib, name, batch):
    lc.check_chain_equals_two_launches(emu_lib, name, batch, modes=(1, -1) if name == "one_tile" else (1,))


def test_chained_level1_many_tiles(emu_lib):
    lc.check_chain_equals_two_launches(emu_lib, "many_tiles", 32)


def test_chained_level1_other_precisions(emu_lib):
    lc.check_chain_equals_two_launches(emu_lib, "residue0", 32, precond_bytes=4)
    lc.check_chain_equals_two_launches(emu_lib, "residue0", 32, dtype=np.float32)


def test_chained_level1_default_by_precision(emu_lib):
    lc.check_default(emu_lib)


@pytest.mark.parametrize("batch", [16, 32])
def test_a_handle_that_has_solved_before(emu_lib, batch):
    lc.check_second_solve_on_a_handle(emu_lib, batch)
