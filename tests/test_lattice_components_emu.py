"""csgpu_components and csgpu_solve_rhs from the lattice form on the emulator build of the kernel sources: the checks of
lattice_components_checks.py on a subset of the cases (the device twin, test_lattice_components_gpu.py, runs the whole grid)."""
import numpy as np
import pytest

import lattice_components_checks as lc


@pytest.mark.parametrize("four", [False, True], ids=["eight", "four"])
@pytest.mark.parametrize("name", ["serpentine", "diagonals", "hwall", "rand45", "rand45_small", "allvalid_small"])
def test_components_equal_csr_path(emu_lib, name, four):
    lc.check_equals_csr_path(emu_lib, name, four)


def test_components_equal_csr_path_other_settings(emu_lib):
    lc.check_equals_csr_path(emu_lib, "rand45_small", False, dtype=np.float32)
    lc.check_equals_csr_path(emu_lib, "diagonals", True, dtype=np.float32)
    lc.check_equals_csr_path(emu_lib, "rand45_small", False, avg=True)


@pytest.mark.parametrize("four", [False, True], ids=["eight", "four"])
@pytest.mark.parametrize("name", ["serpentine", "diagonals", "hwall", "rand45", "rand45_small", "allvalid_small"])
def test_components_against_scipy(emu_lib, name, four):
    lc.check_against_scipy(emu_lib, name, four)


def test_streamed_host_matrix_without_csr_form(emu_lib):
    lc.check_streamed_host_matrix(emu_lib)


@pytest.mark.parametrize("case,prec,batch", [("small", "fp64", 4), ("tall", "fp64", 1), ("rand45", "mixed", 4),
                                             ("small", "fp32", 4)])
def test_solve_rhs_equals_csr_path(emu_lib, case, prec, batch):
    lc.check_solve_rhs(emu_lib, case, prec, batch)


def test_product_path_without_csr_form(emu_lib):
    lc.check_product_path(emu_lib)


def test_default_takes_the_csr_path(emu_lib):
    lc.check_default_unchanged(emu_lib)
