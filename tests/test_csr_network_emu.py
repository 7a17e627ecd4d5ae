"""The general-CSR kernels (csrc/spmv.h, the SpGEMM and transpose of csrc/amg_setup.h) on network-shaped matrices, on the
emulator build of the kernel sources: the checks of csr_network_checks.py with the matrices, K values, bounds and options of
the device twin, test_csr_network_gpu.py. A set-up of these graphs takes 2 - 20 s in the emulator and is nearly all of a
test's time, so the hierarchy checks run on four of the device twin's thirty (graph, precision) cases -- still every merge
width, hubs and both precisions -- and the solves on one of its eight: batches of 32 (the K = 32 two-halves path of the
epilogues) with a ragged last batch of 3, on an fp32 hierarchy."""
import numpy as np
import pytest

import csr_network_checks as cn

# merge brackets: geo2 <=24; geo20_hub <=24, >48; pa <=6, <=48, >48; tree_hub <=3, <=12, >48
CASES = [("geo2", 0), ("geo20_hub", 4), ("pa", 4), ("tree_hub", 0)]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    cn.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(cn.FINE_MATRICES))
def test_fine_product_on_ragged_and_dense_rows(emu_lib, name, dtype):
    cn.check_fine_products(emu_lib, name, dtype)


@pytest.mark.parametrize("graph,precond_bytes", CASES)
def test_every_operator_of_every_level(emu_lib, graph, precond_bytes):
    cn.check_level_operators(emu_lib, graph, precond_bytes)


@pytest.mark.parametrize("graph,precond_bytes", CASES)
def test_setup_kernels_on_every_level(emu_lib, graph, precond_bytes):
    cn.check_setup_kernels(emu_lib, graph, precond_bytes)


def test_fp32_handle_hierarchy(emu_lib):
    cn.check_setup_kernels(emu_lib, "geo4_hub", 0, dtype=np.float32)
    cn.check_level_operators(emu_lib, "geo4_hub", 0, dtype=np.float32)


def test_every_merge_width_is_reached(emu_lib):
    cn.check_coverage(emu_lib, CASES)


@pytest.mark.parametrize("d,precond_bytes,batch", [(20, 4, 32)])
def test_solves_run_the_epilogues_on_long_rows(emu_lib, d, precond_bytes, batch):
    cn.check_epilogue_solves(emu_lib, d, precond_bytes, batch)
