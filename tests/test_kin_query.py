"""The kinematic character at caller-given times (deepmimic_amd/kin_query.py, `dm_kin_query` / k_kin_query of dm_device.h) on the CPU emulator;
tests/test_kin_query_gpu.py runs the same checks on the device.  The checks and their bounds are in tests/kin_query_common.py:

* byte-exact: an offset of 0 against dm_link_state(which = 1); frame k of K = 3 against K = 1; TIMES_PER_ENV and TIMES_ABSOLUTE against the shared relative form;
  rows of N = 3 against N = 1 contexts; each output alone between sentinels, two runs
* against the oracle (Oracle.kin_eval, Skel) for a looping clip, the large class, a clip that does not loop, a multi-clip dataset (own clip and another one) and
  the class with a ball, about the env's origin and the identity origin
* invalid inputs (here only: the same source runs on the device, which is handed valid values only) and the refusals by name"""
import numpy as np
import pytest

import kin_query_common as kc


def host_alloc(a):
    b = np.ascontiguousarray(a).copy()
    return b.ctypes.data, lambda: b


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4", "dog3d_pace"])
def test_zero_offset_equals_link_state(emu_lib, name, precision):
    kc.zero_offset_equals_link_state(name, emu_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4"])
def test_frames_and_flags(emu_lib, name, precision):
    kc.frames_and_flags(name, emu_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_rows_equal_single_env_contexts(emu_lib, precision):
    kc.rows_equal_single_env_contexts(emu_lib, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_shapes(emu_lib, precision):
    kc.shapes(emu_lib, precision, host_alloc)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", kc.ORACLE_ASSETS)
def test_against_oracle(emu_lib, name, precision):
    kc.against_oracle(name, emu_lib, precision, "emu")


@pytest.mark.parametrize("precision", [64, 32])
def test_other_clip_against_oracle(emu_lib, precision):
    kc.other_clip_against_oracle(emu_lib, precision, "emu")


@pytest.mark.parametrize("precision", [64, 32])
def test_invalid_inputs(emu_lib, precision):
    kc.invalid_inputs(emu_lib, precision)


def test_refusals(emu_lib):
    kc.refusals(emu_lib, 64)
