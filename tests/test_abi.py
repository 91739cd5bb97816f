"""The C-ABI library loads and exports every symbol include/dm_hip.h declares (no compute calls: runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dm_[a-z_]+)\s*\(", src)))


def declared_parameter_counts():
    """{function: number of parameters} of every prototype in include/dm_hip.h (`(void)` is none)"""
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = re.findall(r"\b(dm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)
    return {name: 0 if args.strip() in ("", "void") else args.count(",") + 1 for name, args in protos}


def test_header_declares_the_boundary():
    names = declared_functions()
    for must in ("dm_create", "dm_destroy", "dm_reset", "dm_set_action", "dm_update", "dm_query", "dm_step_batch",
                 "dm_build_offsets_scales", "dm_set_time_limits", "dm_last_error"):
        assert must in names


def test_hip_library_exports_every_declared_symbol(hip_lib):
    lib = ctypes.CDLL(hip_lib)
    for name in declared_functions():
        assert hasattr(lib, name), "libdm_hip.so does not export %s" % name


def test_create_without_gpu_fails_loudly(hip_lib):
    """No CPU fallback: on a box without a HIP device dm_create must return an error, not compute on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    try:
        BatchEnv(model.load_asset("humanoid3d_walk"), 1, lib_path=hip_lib)
    except RuntimeError as ex:
        assert "no HIP device" in str(ex) or "hip" in str(ex).lower()
    else:
        raise AssertionError("BatchEnv was created without a GPU")


def test_binding_mirrors_the_header_structs(emu_lib, tmp_path):
    """the ctypes structs of deepmimic_amd/core.py are written by hand: their sizes and a field-offset sample must be what a C compiler makes of
    include/dm_hip.h, and binding, header and library must agree on DM_ABI_VERSION"""
    import ctypes as C
    import re
    import subprocess
    from deepmimic_amd import core
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm_hip.h"\nint main(void){ printf("%d %zu %zu %zu %zu %zu\\n", DM_ABI_VERSION, '
                   'sizeof(dm_create_info), sizeof(dm_scene_tables), offsetof(dm_scene_tables, scene_goal), offsetof(dm_scene_tables, ball_radius), '
                   'offsetof(dm_scene_tables, perturb_part_mask)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    ver, s_info, s_tab, o_goal, o_ball, o_mask = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert ver == core.ABI_VERSION == int(re.search(r"#define DM_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "dm_hip.h")).read()).group(1))
    assert (s_info, s_tab) == (C.sizeof(core._CreateInfo), C.sizeof(core._SceneTables))
    assert (o_goal, o_ball, o_mask) == (core._SceneTables.scene_goal.offset, core._SceneTables.ball_radius.offset, core._SceneTables.perturb_part_mask.offset)
    lib = core.load_library(emu_lib)
    sizes = (C.c_int32 * 2)()
    assert lib.dm_abi_version() == ver and lib.dm_struct_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (s_info, s_tab)


def test_binding_signatures_match_the_header(emu_lib):
    """deepmimic_amd/binding.py SIGNATURES is written by hand: every name is a prototype of include/dm_hip.h with as many parameters, and load_library has declared
    it on the library before any Policy / DeviceNormalizer / store exists (a 64-bit address passed as a Python int needs its argtypes from the first call on)"""
    from deepmimic_amd import binding, core
    counts = declared_parameter_counts()
    assert counts["dm_last_error"] == 0 and counts["dm_motion_duration"] == 1 and counts["dm_td_lambda_returns"] == 16        # (the parser)
    lib = core.load_library(emu_lib)
    for name, (argtypes, restype) in binding.SIGNATURES.items():
        assert name in counts, "%s is not declared in include/dm_hip.h" % name
        assert len(argtypes) == counts[name], "%s: %d argtypes, the header declares %d parameters" % (name, len(argtypes), counts[name])
        f = getattr(lib, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes), "%s has no argtypes after load_library" % name
        if restype is not None:
            assert f.restype is restype, name


@pytest.mark.gpu
def test_invalid_device_id_is_refused_by_name_gpu(hip_lib):
    """every learner-side entry point that takes a device_id refuses one that names no device, under its own name and before anything is launched: the output
    buffers keep their bytes.  One row of width 2 (T = N = 1)."""
    import numpy as np
    import torch
    from deepmimic_amd import math_probe as mpr
    from deepmimic_amd import wave_probe as wpr
    from deepmimic_amd import ppo_batch as pb
    from deepmimic_amd import returns as rt
    from deepmimic_amd.normalizer import DeviceNormalizer
    from deepmimic_amd.policy import Policy, random_weights
    f32 = lambda *shape: torch.zeros(shape, device="cuda")
    i32 = lambda *shape: torch.ones(shape, dtype=torch.int32, device="cuda")
    sent_f = lambda *shape: torch.full(shape, -77.0, device="cuda")
    sent_i = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device="cuda")
    rewards, values, term_values, terminate, done = f32(1, 1), f32(2, 1), f32(1, 1), i32(1, 1), i32(1, 1)
    returns, mask = sent_f(1, 1), sent_i(1, 1)
    adv, targets, valid_idx, exp_idx, counts = sent_f(1, 1), sent_f(1, 1), sent_i(1), sent_i(1), sent_i(2)
    stats = torch.full((2,), -77.0, dtype=torch.float64, device="cuda")
    nbytes = pb.workspace_bytes(1, 1, hip_lib)
    work = torch.full(((nbytes + 7) // 8,), -77.0, dtype=torch.float64, device="cuda")
    idx, count, src, dst = torch.zeros(1, dtype=torch.int32, device="cuda"), i32(1), f32(1, 2), sent_f(1, 2)
    weights = random_weights(2, 1, H1=64, H2=64)
    probe_in = torch.zeros((1, mpr.IN), dtype=torch.float64, device="cuda")
    probe_out = torch.full((1, mpr.OUT), -77.0, dtype=torch.float64, device="cuda")
    wave_in = torch.zeros((wpr.WAVE, wpr.IN), dtype=torch.float64, device="cuda")
    wave_out = torch.full((wpr.WAVE, wpr.OUT), -77.0, dtype=torch.float64, device="cuda")
    for dev in (-1, torch.cuda.device_count()):
        with pytest.raises(RuntimeError, match="dm_td_lambda_returns: invalid device_id"):
            rt.td_lambda_returns(1, 1, rewards.data_ptr(), values.data_ptr(), term_values.data_ptr(), terminate.data_ptr(), done.data_ptr(), 0, 0.95, 0.95, 0.0, 1.0,
                                 returns.data_ptr(), mask.data_ptr(), device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_ppo_advantages: invalid device_id"):
            pb.advantages_device(1, 1, rewards.data_ptr(), values.data_ptr(), 0, 0, 1e-5, 5.0, -np.inf, np.inf, adv.data_ptr(), targets.data_ptr(), valid_idx.data_ptr(),
                                 exp_idx.data_ptr(), counts.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes, device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_ppo_gather: invalid device_id"):
            pb.gather_device(idx.data_ptr(), count.data_ptr(), 0, 1, 1, 0, [(src.data_ptr(), dst.data_ptr(), 2)], device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_norm_create: invalid device_id"):
            DeviceNormalizer(2, device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_policy_create: invalid device_id"):
            Policy(weights, device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_math_probe: invalid device_id"):
            mpr.math_probe("SINCOS", 0, 1, probe_in.data_ptr(), probe_out.data_ptr(), device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_wave_probe: invalid device_id"):
            wpr.wave_probe("WAVE_SUM", 0, 1, wave_in.data_ptr(), wave_out.data_ptr(), device_id=dev, lib_path=hip_lib)
    for name, t in dict(returns=returns, mask=mask, adv=adv, targets=targets, valid_idx=valid_idx, exp_idx=exp_idx, counts=counts, stats=stats, work=work, dst=dst, probe_out=probe_out, wave_out=wave_out).items():
        assert (t == -77).all(), name
