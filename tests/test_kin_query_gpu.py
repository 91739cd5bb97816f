"""tests/test_kin_query.py on the device: the same checks (tests/kin_query_common.py) on libdm_hip.so, fp32 and fp64 contexts.  Valid inputs only: the NaN rows of
invalid ones are checked on the CPU emulator, which compiles the same source."""
import numpy as np
import pytest

import kin_query_common as kc

pytestmark = pytest.mark.gpu


def device_alloc(a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), lambda: t.cpu().numpy()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4", "dog3d_pace"])
def test_zero_offset_equals_link_state_gpu(hip_lib, name, precision):
    kc.zero_offset_equals_link_state(name, hip_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4"])
def test_frames_and_flags_gpu(hip_lib, name, precision):
    kc.frames_and_flags(name, hip_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_rows_equal_single_env_contexts_gpu(hip_lib, precision):
    kc.rows_equal_single_env_contexts(hip_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_shapes_gpu(hip_lib, precision):
    kc.shapes(hip_lib, precision, device_alloc)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", kc.ORACLE_ASSETS)
def test_against_oracle_gpu(hip_lib, name, precision):
    kc.against_oracle(name, hip_lib, precision, "gpu")


@pytest.mark.parametrize("precision", [64, 32])
def test_other_clip_against_oracle_gpu(hip_lib, precision):
    kc.other_clip_against_oracle(hip_lib, precision, "gpu")


def test_refusals_gpu(hip_lib):
    kc.refusals(hip_lib, 32)
