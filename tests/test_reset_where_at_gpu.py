"""tests/test_reset_where_at.py on the device (tests/reset_where_at_common.py): libdm_hip.so, fp32 contexts, and the plain scene in fp64 as well.  Valid values
only: the untouched env and the bad word of invalid ones are checked on the CPU emulator, which compiles the same source."""
import pytest

import reset_where_at_common as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(rc.CASES))
def test_nothing_given_equals_reset_where_gpu(hip_lib, case):
    rc.nothing_given_equals_reset_where(case, hip_lib, 32, 4 if case == "amp_heading_clips4" else 3)


def test_nothing_given_equals_reset_where_f64_gpu(hip_lib):
    rc.nothing_given_equals_reset_where("plain", hip_lib, 64, 3)


def test_nothing_given_equals_reset_where_physics2_gpu(hip_lib):
    rc.nothing_given_equals_reset_where("plain", hip_lib, 32, 3, physics=2)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case", ["plain", "amp_heading_clips4"])
def test_given_time_equals_dm_reset_gpu(hip_lib, case, precision):
    rc.given_time_equals_dm_reset(case, hip_lib, precision, 4 if case == "amp_heading_clips4" else 3)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4"])
def test_given_start_against_oracle_gpu(hip_lib, name, precision):
    rc.given_start_against_oracle(name, hip_lib, precision, "gpu")


@pytest.mark.parametrize("precision", [64, 32])
def test_drawn_time_with_given_clip_gpu(hip_lib, precision):
    rc.drawn_time_with_given_clip(hip_lib, precision, "gpu")


def test_refusals_gpu(hip_lib):
    rc.refusals(hip_lib, 32)
