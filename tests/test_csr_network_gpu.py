"""The general-CSR kernels (csrc/spmv.h, the SpGEMM and transpose of csrc/amg_setup.h) on network-shaped matrices, on the
device: the checks of csr_network_checks.py against scipy within the per-row forward bound. The emulator twin is
test_csr_network_emu.py."""
import numpy as np
import pytest

import csr_network_checks as cn

pytestmark = pytest.mark.gpu

CASES = [(g, pb) for g in cn.HIERARCHY_GRAPHS for pb in (0, 4)]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    cn.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(cn.FINE_MATRICES))
def test_fine_product_on_ragged_and_dense_rows_gpu(gpu_lib, name, dtype):
    cn.check_fine_products(gpu_lib, name, dtype)


@pytest.mark.parametrize("graph,precond_bytes", CASES)
def test_every_operator_of_every_level_gpu(gpu_lib, graph, precond_bytes):
    cn.check_level_operators(gpu_lib, graph, precond_bytes)


@pytest.mark.parametrize("graph,precond_bytes", CASES)
def test_setup_kernels_on_every_level_gpu(gpu_lib, graph, precond_bytes):
    cn.check_setup_kernels(gpu_lib, graph, precond_bytes)


def test_fp32_handle_hierarchy_gpu(gpu_lib):
    cn.check_setup_kernels(gpu_lib, "geo4_hub", 0, dtype=np.float32)
    cn.check_level_operators(gpu_lib, "geo4_hub", 0, dtype=np.float32)


def test_every_merge_width_is_reached_gpu(gpu_lib):
    cn.check_coverage(gpu_lib, CASES)


@pytest.mark.parametrize("precond_bytes,batch", [(0, 32), (4, 32), (0, 1), (4, 8)])
@pytest.mark.parametrize("d", [4, 20])
def test_solves_run_the_epilogues_on_long_rows_gpu(gpu_lib, d, precond_bytes, batch):
    cn.check_epilogue_solves(gpu_lib, d, precond_bytes, batch)
