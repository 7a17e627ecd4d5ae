"""The stats merge of the multi-device calls on the emulator build: the checks of multi_stats_checks.py (the device twin is
test_multi_stats_gpu.py), plus the precedence of a hard error over the other devices' results, which needs three (emulated)
devices and therefore a process of its own."""
import os
import subprocess
import sys

import multi_stats_checks as ms


def test_chunk_merge_on_one_device(emu_lib):
    ms.check_chunk_merge(emu_lib)


def test_map_calls_pass_one_device_through(emu_lib):
    ms.check_pass_through(emu_lib)


def test_stream_slots_of_a_call_without_maps_are_carried(emu_lib):
    ms.check_stream_slots_are_carried(emu_lib)


def test_hard_error_of_one_device_wins(emu_lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import circuitscape_jl_amd\n"
            "from circuitscape_jl_amd import lib\n"
            "import multi_stats_checks as ms\n"
            "lib.load(%r)\n"
            "ms.check_error_precedence(lib)\n"
            "print('ok')\n") % (root, os.path.join(root, "tests"), os.path.join(root, "tests", "emu", "libcsgpu_emu.so"))
    env = dict(os.environ, HIPEMU_DEVICES="3", HIPEMU_THREADS="2")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stderr[-2000:]
