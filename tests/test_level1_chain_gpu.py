"""The chained level-1 pass (csgpu_opts.fused_level1 = 2) and the first CG product of a batch without the old search
direction, on the device: the checks of level1_chain_checks.py at every shape and both batch widths."""
import numpy as np
import pytest

import level1_chain_checks as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", [16, 32])
@pytest.mark.parametrize("name", sorted(lc.SHAPES))
def test_chained_level1_equals_two_launches_gpu(gpu_lib, name, batch):
    lc.check_chain_equals_two_launches(gpu_lib, name, batch, modes=(1, -1) if name == "many_tiles" else (1,))


@pytest.mark.parametrize("batch", [16, 32])
def test_chained_level1_other_precisions_gpu(gpu_lib, batch):
    lc.check_chain_equals_two_launches(gpu_lib, "many_tiles", batch, precond_bytes=4)
    lc.check_chain_equals_two_launches(gpu_lib, "many_tiles", batch, dtype=np.float32)


def test_chained_level1_default_by_precision_gpu(gpu_lib):
    lc.check_default(gpu_lib)


@pytest.mark.parametrize("batch", [16, 32])
def test_a_handle_that_has_solved_before_gpu(gpu_lib, batch):
    lc.check_second_solve_on_a_handle(gpu_lib, batch)
    lc.check_second_solve_on_a_handle(gpu_lib, batch, name="many_tiles")
