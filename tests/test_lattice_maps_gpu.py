"""csgpu_opts.lattice_maps on the device: voltage / current maps and the explicit residual check of pair solves from the
lattice form, without a CSR matrix (csrc/lattice_currents.h). The checks of lattice_maps_checks.py; the emulator twin is
test_lattice_maps_emu.py."""
import numpy as np
import pytest

import lattice_maps_checks as lm

pytestmark = pytest.mark.gpu

PRECISIONS = {"fp64": (np.float64, 0), "fp32": (np.float32, 0), "mixed": (np.float64, 4)}


@pytest.mark.parametrize("batch", [1, 4, 16, 32])
@pytest.mark.parametrize("prec", ["fp64", "fp32", "mixed"])
@pytest.mark.parametrize("name", ["tall", "small", "wide"])
def test_lattice_maps_equal_csr_path(gpu_lib, name, prec, batch):
    dtype, pb = PRECISIONS[prec]
    lm.check_equals_csr_path(gpu_lib, name, batch, dtype=dtype, precond_bytes=pb)


@pytest.mark.parametrize("batch", [1, 4, 16, 32])
@pytest.mark.parametrize("kw", [dict(four_neighbors=True), dict(avg_resistances=True)], ids=["four", "avgres"])
def test_lattice_maps_equal_csr_path_connection_rules(gpu_lib, kw, batch):
    lm.check_equals_csr_path(gpu_lib, "tall", batch, **kw)


@pytest.mark.parametrize("batch", [1, 4, 16, 32])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_lattice_maps_equal_csr_path_nodata(gpu_lib, prec, batch):
    dtype, pb = PRECISIONS[prec]
    lm.check_equals_csr_path(gpu_lib, "tall", batch, dtype=dtype, precond_bytes=pb, nodata=True)


@pytest.mark.parametrize("batch", [1, 4, 16, 32])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_maps_accumulated_in_the_kernel(gpu_lib, prec, batch):
    dtype, pb = PRECISIONS[prec]
    lm.check_equals_csr_path(gpu_lib, "wide", batch, dtype=dtype, precond_bytes=pb, nodata=(batch == 16), maps_only_too=True)


def test_no_csr_form_appears(gpu_lib):
    lm.check_no_csr_form(gpu_lib)


def test_node_currents_against_numpy_and_kirchhoff(gpu_lib):
    lm.check_against_numpy(gpu_lib)


def test_golden_maps_through_product_path(gpu_lib):
    from circuitscape_jl_amd import solver as ps
    from conftest import load_case
    from helpers import run_fixture
    from test_emu_solver import _check_maps
    case = load_case("sgVerify1")
    st = {}
    run_fixture(case, ps.HIPAMGSolver(bs=4, opts={"rtol": 1e-10, "atol": 0.0, "criterion": 1, "lattice_maps": 1}), stats=st)
    assert _check_maps(case, st) > 0


def test_multi_handle_maps(gpu_lib):
    lm.check_multi(gpu_lib)


def test_default_takes_the_csr_path(gpu_lib):
    lm.check_default_unchanged(gpu_lib)
