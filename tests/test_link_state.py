"""Link states as device tensors (deepmimic_amd/link_state.py, `dm_link_state` / k_link_state of dm_device.h) on the CPU emulator; tests/test_link_state_gpu.py runs
the same checks on the device.  The checks and their bounds are in tests/link_state_common.py:

* simulated side against the reference's golden vectors (tests/golden/ref_vectors.npz: body_world, joint_world, link_vel, com, com_vel) for humanoid3d_walk,
  dog3d_pace and humanoid3d_spinkick, in both precisions; pose / vel are the float32 rounding of the state that was set, exactly
* the heading against the oracle's cKinTree::BuildOriginTrans of the same pose
* kinematic side: pose / vel against the golden kin_pose / kin_vel, the link state against the oracle's forward kinematics; one multi-clip dataset where every env
  samples its own clip
* the contact column against the env's contact mask, the free body against get_obj_state()
* shapes: each output alone, sentinels behind the last row, two runs, row e of N = 3 against an N = 1 context; refusals by name"""
import numpy as np
import pytest

import link_state_common as lc


def host_alloc(a):
    b = np.ascontiguousarray(a).copy()
    return b.ctypes.data, lambda: b


@pytest.mark.parametrize("precision", [64, 32])
def test_sim_side_vs_reference(emu_lib, precision):
    lc.sim_side_vs_reference(emu_lib, precision, "emu")


def test_heading_vs_origin_trans(emu_lib):
    lc.heading_vs_origin_trans(emu_lib, 64)


@pytest.mark.parametrize("precision", [64, 32])
def test_kin_side(emu_lib, precision):
    lc.kin_side(emu_lib, precision, "emu")


def test_kin_side_multi_clip(emu_lib):
    lc.kin_side_multi_clip(emu_lib, 64)


def test_contact_column(emu_lib):
    lc.contact_column(emu_lib, 64)


def test_free_body(emu_lib):
    lc.free_body(emu_lib, 64)


@pytest.mark.parametrize("precision", [64, 32])
def test_shapes(emu_lib, precision):
    lc.shapes(emu_lib, precision, host_alloc)


def test_refusals(emu_lib):
    lc.refusals(emu_lib, 64)
