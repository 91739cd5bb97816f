"""A masked reset whose clip, clip time and yaw the caller may give (deepmimic_amd/kin_query.py, `dm_reset_where_at` / k_env_reset_where_at of dm_device.h) on the
CPU emulator; tests/test_reset_where_at_gpu.py runs the same checks on the device.  The checks and their bounds are in tests/reset_where_at_common.py: nothing given
against `reset_where`, a given time against `dm_reset` on a twin context, a given start against the oracle's reset, the draws of what is not given, invalid values
(here only: the same source runs on the device, which is handed valid values only) and the refusals by name."""
import pytest

import reset_where_at_common as rc


@pytest.mark.parametrize("case", list(rc.CASES))
def test_nothing_given_equals_reset_where(emu_lib, case):
    rc.nothing_given_equals_reset_where(case, emu_lib, 64, 4 if case == "amp_heading_clips4" else 3)


def test_nothing_given_equals_reset_where_f32(emu_lib):
    rc.nothing_given_equals_reset_where("plain", emu_lib, 32, 3)


def test_nothing_given_equals_reset_where_physics2(emu_lib):
    rc.nothing_given_equals_reset_where("plain", emu_lib, 64, 3, physics=2)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case", ["plain", "amp_heading_clips4"])
def test_given_time_equals_dm_reset(emu_lib, case, precision):
    rc.given_time_equals_dm_reset(case, emu_lib, precision, 4 if case == "amp_heading_clips4" else 3)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4"])
def test_given_start_against_oracle(emu_lib, name, precision):
    rc.given_start_against_oracle(name, emu_lib, precision, "emu")


@pytest.mark.parametrize("precision", [64, 32])
def test_drawn_time_with_given_clip(emu_lib, precision):
    rc.drawn_time_with_given_clip(emu_lib, precision, "emu")


@pytest.mark.parametrize("precision", [64, 32])
def test_invalid_inputs(emu_lib, precision):
    rc.invalid_inputs(emu_lib, precision)


def test_refusals(emu_lib):
    rc.refusals(emu_lib, 64)
