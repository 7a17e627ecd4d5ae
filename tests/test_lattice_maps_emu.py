"""csgpu_opts.lattice_maps on the emulator build of the kernel sources: the checks of lattice_maps_checks.py on a subset of
the shapes and batch widths, chosen to stay within a minute or so (the device twin, test_lattice_maps_gpu.py, runs the whole
grid)."""
import numpy as np
import pytest

import lattice_maps_checks as lm


# (strips: 256 + 5 rows and five column segments at batch 1; 16 + 16 + 8 rows at batch 32)
@pytest.mark.parametrize("name,batch", [("tall", 1), ("small", 32)])
def test_lattice_maps_equal_csr_path(emu_lib, name, batch):
    lm.check_equals_csr_path(emu_lib, name, batch)


def test_lattice_maps_equal_csr_path_other_precisions(emu_lib):
    lm.check_equals_csr_path(emu_lib, "small", 4, dtype=np.float32)
    lm.check_equals_csr_path(emu_lib, "small", 4, precond_bytes=4)


@pytest.mark.parametrize("kw", [dict(four_neighbors=True), dict(avg_resistances=True)], ids=["four", "avgres"])
def test_lattice_maps_equal_csr_path_connection_rules(emu_lib, kw):
    lm.check_equals_csr_path(emu_lib, "small", 4, **kw)


# (batch 4 on a raster with NODATA cells: cell space, pairs inside one component)
@pytest.mark.parametrize("batch", [4, 16])
def test_maps_accumulated_in_the_kernel(emu_lib, batch):
    lm.check_equals_csr_path(emu_lib, "small", batch, nodata=(batch == 4), maps_only_too=True)


def test_no_csr_form_appears(emu_lib):
    lm.check_no_csr_form(emu_lib, name="small")


def test_node_currents_against_numpy_and_kirchhoff(emu_lib):
    lm.check_against_numpy(emu_lib)


def test_golden_maps_through_product_path(emu_lib):
    from circuitscape_jl_amd import solver as ps
    from conftest import load_case
    from helpers import run_fixture
    from test_emu_solver import _check_maps
    case = load_case("sgVerify1")
    st = {}
    run_fixture(case, ps.HIPAMGSolver(bs=4, opts={"rtol": 1e-10, "atol": 0.0, "criterion": 1, "lattice_maps": 1}), stats=st)
    assert _check_maps(case, st) > 0


def test_default_takes_the_csr_path(emu_lib):
    lm.check_default_unchanged(emu_lib, name="small")
