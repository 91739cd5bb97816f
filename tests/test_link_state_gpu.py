"""tests/test_link_state.py on the device: the same checks (tests/link_state_common.py) on libdm_hip.so, fp32 and fp64 contexts."""
import numpy as np
import pytest

import link_state_common as lc

pytestmark = pytest.mark.gpu


def device_alloc(a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), lambda: t.cpu().numpy()


@pytest.mark.parametrize("precision", [64, 32])
def test_sim_side_vs_reference_gpu(hip_lib, precision):
    lc.sim_side_vs_reference(hip_lib, precision, "gpu")


def test_heading_vs_origin_trans_gpu(hip_lib):
    lc.heading_vs_origin_trans(hip_lib, 32)


@pytest.mark.parametrize("precision", [64, 32])
def test_kin_side_gpu(hip_lib, precision):
    lc.kin_side(hip_lib, precision, "gpu")


@pytest.mark.parametrize("precision", [64, 32])
def test_kin_side_multi_clip_gpu(hip_lib, precision):
    lc.kin_side_multi_clip(hip_lib, precision)


def test_contact_column_gpu(hip_lib):
    lc.contact_column(hip_lib, 32)


def test_free_body_gpu(hip_lib):
    lc.free_body(hip_lib, 32)


@pytest.mark.parametrize("precision", [64, 32])
def test_shapes_gpu(hip_lib, precision):
    lc.shapes(hip_lib, precision, device_alloc)


def test_refusals_gpu(hip_lib):
    lc.refusals(hip_lib, 32)
