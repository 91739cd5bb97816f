"""`BatchEnv.reset_where` (`dm_reset_where`, k_env_reset_where of dm_device.h) on the CPU emulator: a step without auto-reset followed by the masked reset of the envs
that ended is, byte for byte, the auto-reset step.  The method and the checks are in tests/reset_where_common.py; tests/test_reset_where_gpu.py runs them on the device."""
import pytest

import reset_where_common as rc


@pytest.mark.parametrize("n", [4, 3])
@pytest.mark.parametrize("case", list(rc.CASES))
def test_masked_reset_equals_auto_reset(emu_lib, case, n):
    rc.masked_reset_equals_auto_reset(case, emu_lib, 64, n)


@pytest.mark.parametrize("n", [4, 3])
def test_masked_reset_equals_auto_reset_physics2(emu_lib, n):
    rc.masked_reset_equals_auto_reset("plain", emu_lib, 64, n, physics=2)


@pytest.mark.parametrize("case", ["plain", "amp_heading_clips4"])
def test_zero_mask_and_mask_values(emu_lib, case):
    rc.zero_mask_and_mask_values(case, emu_lib, 64, 4)
