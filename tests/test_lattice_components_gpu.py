"""csgpu_components and csgpu_solve_rhs from the lattice form on the device, without a CSR matrix
(csrc/lattice_components.h; csgpu_opts.lattice_maps = 1). The checks of lattice_components_checks.py; the emulator twin is
test_lattice_components_emu.py."""
import numpy as np
import pytest

import lattice_components_checks as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("four", [False, True], ids=["eight", "four"])
@pytest.mark.parametrize("name", list(lc.CASES))
def test_components_equal_csr_path(gpu_lib, name, four, dtype):
    lc.check_equals_csr_path(gpu_lib, name, four, dtype=dtype)


@pytest.mark.parametrize("name", ["rand45", "diagonals"])
def test_components_equal_csr_path_avg_resistances(gpu_lib, name):
    lc.check_equals_csr_path(gpu_lib, name, False, avg=True)


@pytest.mark.parametrize("four", [False, True], ids=["eight", "four"])
@pytest.mark.parametrize("name", list(lc.CASES))
def test_components_against_scipy(gpu_lib, name, four):
    lc.check_against_scipy(gpu_lib, name, four)


def test_streamed_host_matrix_without_csr_form(gpu_lib):
    lc.check_streamed_host_matrix(gpu_lib)


@pytest.mark.parametrize("batch", [1, 4, 16, 32])
@pytest.mark.parametrize("prec", list(lc.PRECISIONS))
@pytest.mark.parametrize("case", list(lc.RHS_CASES))
def test_solve_rhs_equals_csr_path(gpu_lib, case, prec, batch):
    lc.check_solve_rhs(gpu_lib, case, prec, batch)


def test_product_path_without_csr_form(gpu_lib):
    lc.check_product_path(gpu_lib)


def test_default_takes_the_csr_path(gpu_lib):
    lc.check_default_unchanged(gpu_lib)


def test_multi_handle_components(gpu_lib):
    lc.check_multi(gpu_lib)
