"""The stats merge of the multi-device calls on the device: the checks of multi_stats_checks.py on one device (the emulator
twin, test_multi_stats_emu.py, also covers the error precedence across three emulated devices)."""
import pytest

import multi_stats_checks as ms

pytestmark = pytest.mark.gpu


def test_chunk_merge_on_one_device(gpu_lib):
    ms.check_chunk_merge(gpu_lib)


def test_map_calls_pass_one_device_through(gpu_lib):
    ms.check_pass_through(gpu_lib)


def test_stream_slots_of_a_call_without_maps_are_carried(gpu_lib):
    ms.check_stream_slots_are_carried(gpu_lib)
