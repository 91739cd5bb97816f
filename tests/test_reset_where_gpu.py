"""tests/test_reset_where.py on the device (tests/reset_where_common.py): libdm_hip.so, fp32 contexts, and the plain scene in fp64 as well."""
import pytest

import reset_where_common as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [4, 3])
@pytest.mark.parametrize("case", list(rc.CASES))
def test_masked_reset_equals_auto_reset_gpu(hip_lib, case, n):
    rc.masked_reset_equals_auto_reset(case, hip_lib, 32, n)


def test_masked_reset_equals_auto_reset_f64_gpu(hip_lib):
    rc.masked_reset_equals_auto_reset("plain", hip_lib, 64, 4)


@pytest.mark.parametrize("n", [4, 3])
def test_masked_reset_equals_auto_reset_physics2_gpu(hip_lib, n):
    rc.masked_reset_equals_auto_reset("plain", hip_lib, 32, n, physics=2)


@pytest.mark.parametrize("case", ["plain", "amp_heading_clips4"])
def test_zero_mask_and_mask_values_gpu(hip_lib, case):
    rc.zero_mask_and_mask_values(case, hip_lib, 32, 4)
