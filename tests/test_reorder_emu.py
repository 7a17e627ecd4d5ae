"""Device-side locality reordering (csgpu_opts.reorder) on the emulator build of the kernel sources: the checks of
reorder_checks.py at n = 3000 and on the multi-component graph; the device twin is test_reorder_gpu.py."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import reorder_checks as rc

NETWORK_GOLDENS = ["sgNetworkVerify1", "sgNetworkVerify2", "sgNetworkVerify3"]


def test_permutation_is_a_deterministic_bijection(emu_lib):
    rc.check_permutation(emu_lib, rc.geometric(3000))
    rc.check_permutation(emu_lib, rc.multi_component_graph())


def test_reorder_is_ignored_where_there_is_locality(emu_lib, oracle):
    rc.check_not_applied(emu_lib, oracle)


def test_an_expander_is_not_reordered(emu_lib):
    rc.check_expander_not_reordered(emu_lib)


@pytest.mark.parametrize("graph", ["geometric", "components"])
def test_device_matrix_is_the_permuted_matrix(emu_lib, graph):
    rc.check_permuted_matrix(emu_lib, rc.geometric(3000) if graph == "geometric" else rc.multi_component_graph())


def test_quality_against_reverse_cuthill_mckee(emu_lib):
    rc.check_quality(emu_lib, rc.geometric(3000))


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("precond_bytes", [0, 4])
@pytest.mark.parametrize("graph", ["geometric", "components"])
def test_every_entry_point_keeps_the_callers_numbering(emu_lib, graph, precond_bytes, batch):
    G = rc.geometric(3000) if graph == "geometric" else rc.multi_component_graph()
    rc.check_entry_points(emu_lib, G, precond_bytes, batch)


@pytest.mark.parametrize("name", NETWORK_GOLDENS)
def test_network_goldens_with_reorder(emu_lib, name):
    rc.check_network_golden(emu_lib, name)


@pytest.mark.parametrize("name", __import__("conftest").advanced_cases())
def test_network_advanced_goldens_with_reorder(emu_lib, name):
    rc.check_network_advanced_golden(emu_lib, name)


def test_three_emulated_devices_reorder_alike():
    """csgpu_multi_setup with reorder=1 on three emulated devices: every replica has the same permutation, the multi-device
    calls equal the single reordered handle (a process of its own: the number of emulated devices is fixed at start-up)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import sys, json
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import circuitscape_jl_amd
        from circuitscape_jl_amd import lib
        import reorder_checks as rc
        lib.load(%r)
        assert lib.device_count() == 3
        G = rc.geometric(3000)
        rc.check_multi_same_permutation(lib, G, [0, 1, 2])
        rc.check_multi(lib, G, [0, 1, 2], npts=11)
        print(json.dumps({"ok": True}))
    ''') % (root, os.path.join(root, "tests"), os.path.join(root, "tests", "emu", "libcsgpu_emu.so"))
    env = dict(os.environ, HIPEMU_DEVICES="3", HIPEMU_THREADS="2")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800, cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    assert json.loads(res.stdout.strip().splitlines()[-1])["ok"]
