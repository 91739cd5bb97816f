"""Expert AMP observations whose clips and clip times are drawn on the device (include/dm_hip.h dm_amp_expert_draw, k_amp_expert_draw in deepmimic_amd/csrc/dm_replay.h):
for call = 0, 1, 2 bit-identical to what a fresh twin context of the same seed returns from three consecutive host-route calls -- `amp_expert(n)` on a single-clip
imitate_amp scene, `amp_expert_clips(n)` on the four-clip amp_heading_clips4 -- and the clip ids and times equal to the Python statement of the draws
(streams.reset_rand01 over `clip_table()`).  On the emulator build through host addresses and, marked `gpu`, through torch tensors."""
import numpy as np
import pytest

from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv
from deepmimic_amd.streams import reset_rand01
from test_amp import amp_tables

SENT = -77
SCENES = ["imitate_amp", "amp_heading_clips4"]
SEED, ENV_OFF = 12345, 6


def tables_of(scene):
    return amp_tables("humanoid3d_walk") if scene == "imitate_amp" else model.load_asset("amp_heading_clips4")


def make_env(scene, lib):
    return BatchEnv(tables_of(scene), 2, seed=SEED, env_id_offset=ENV_OFF, lib_path=lib)


def reference_draws(env, n, call):
    """the draws of dm_amp_expert / dm_amp_expert_clips at their call `call` (dm_host.cpp)"""
    dur, cdf = env.clip_table()
    clips, times = np.zeros(n, np.int32), np.zeros(n)
    for i in range(n):
        k = 0
        if env.num_clips > 1:
            u = reset_rand01(SEED, ENV_OFF + 0x434C50, call, i)
            while k < env.num_clips - 1 and not u < cdf[k]:
                k += 1
        clips[i], times[i] = k, dur[k] * reset_rand01(SEED, ENV_OFF + 0x414D50, call, i)
    return clips, times


class Host:
    """emulator: device pointers are host addresses"""
    def __init__(self, env):
        pass

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return h.copy()


class Torch:
    """GPU: torch tensors; the context launches on torch's current stream, so that a read through torch is ordered behind it"""
    def __init__(self, env):
        import torch
        self.torch = torch
        env.set_stream(int(torch.cuda.current_stream().cuda_stream))

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        return h.cpu().numpy()


def check_draw(scene, lib, backend):
    for n in (1, 5, 64, 65):
        env, twin = make_env(scene, lib), make_env(scene, lib)
        be = backend(env)
        A = env.amp_size
        assert A > 0 and env.num_clips == (1 if scene == "imitate_amp" else 4)
        gh = np.linspace(-0.05, 0.08, n)
        d_gh = be.put(gh)
        seen = []
        for call in range(3):
            with_gh = call != 1                 # call 1 without ground heights (NULL: 0)
            d_out, d_clips, d_times = be.put(np.full((n + 1, A), SENT, np.float32)), be.put(np.full(n + 1, SENT, np.int32)), be.put(np.full(n + 1, float(SENT)))
            env.amp_expert_draw_device(n, call, be.ptr(d_out), ground_h_ptr=be.ptr(d_gh) if with_gh else 0, clips_out_ptr=be.ptr(d_clips), times_out_ptr=be.ptr(d_times))
            out, clips, times = be.get(d_out), be.get(d_clips), be.get(d_times)
            host = (twin.amp_expert if scene == "imitate_amp" else twin.amp_expert_clips)(n, ground_h=gh if with_gh else None)
            assert out[:n].tobytes() == host.tobytes(), (scene, n, call)
            assert (out[n] == SENT).all() and clips[n] == SENT and times[n] == SENT, "guards"
            want_clips, want_times = reference_draws(env, n, call)
            assert (clips[:n] == want_clips).all() and times[:n].tobytes() == want_times.tobytes(), (scene, n, call)
            dur, _ = env.clip_table()
            assert (times[:n] >= 0).all() and (times[:n] < np.asarray(dur)[clips[:n]]).all() and np.isfinite(out[:n]).all()
            seen.append(out[:n].copy())
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
        if scene != "imitate_amp" and n >= 64:
            assert len(set(clips[:n].tolist())) > 1           # the four clips are drawn by weight
        # the outputs for the draws are optional, and the same call gives the same rows
        d_out = be.put(np.full((n, A), SENT, np.float32))
        env.amp_expert_draw_device(n, 2, be.ptr(d_out), ground_h_ptr=be.ptr(d_gh))
        assert be.get(d_out).tobytes() == seen[2].tobytes()
        # the context's own counter was neither read nor advanced: its host route now returns what call 0 returns
        host0 = (env.amp_expert if scene == "imitate_amp" else env.amp_expert_clips)(n, ground_h=gh)
        assert host0.tobytes() == seen[0].tobytes(), (scene, n)
        env.close(); twin.close()


def check_refusals(lib, backend):
    env = make_env("imitate_amp", lib)
    be = backend(env)
    d_out = be.put(np.full((4, env.amp_size), SENT, np.float32))
    with pytest.raises(RuntimeError, match="dm_amp_expert_draw: n must be >= 1"):
        env.amp_expert_draw_device(0, 0, be.ptr(d_out))
    with pytest.raises(RuntimeError, match="dm_amp_expert_draw: n must be >= 1"):
        env.amp_expert_draw_device(-3, 0, be.ptr(d_out))
    with pytest.raises(RuntimeError, match="dm_amp_expert_draw: out_dev is NULL"):
        env.amp_expert_draw_device(4, 0, 0)
    assert (be.get(d_out) == SENT).all()
    # the existing entry point keeps its refusal
    import ctypes as C
    from deepmimic_amd.core import DM_DEVICE_PTRS
    env.lib.dm_amp_expert.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    assert env.lib.dm_amp_expert(env.h, 4, None, None, C.c_void_p(be.ptr(d_out)), DM_DEVICE_PTRS) != 0 and b"needs explicit sample times" in env.lib.dm_last_error()
    env.close()
    plain = BatchEnv(model.load_asset("humanoid3d_walk"), 1, lib_path=lib)
    be = backend(plain)
    d_out = be.put(np.zeros((4, 8), np.float32))
    with pytest.raises(RuntimeError, match="imitate_amp"):
        plain.amp_expert_draw_device(4, 0, be.ptr(d_out))
    plain.close()


@pytest.mark.parametrize("scene", SCENES)
def test_expert_draw_emulator(emu_lib, scene):
    check_draw(scene, emu_lib, Host)


def test_expert_draw_refusals_emulator(emu_lib):
    check_refusals(emu_lib, Host)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_expert_draw_gpu(hip_lib, scene):
    check_draw(scene, hip_lib, Torch)


@pytest.mark.gpu
def test_expert_draw_refusals_gpu(hip_lib):
    check_refusals(hip_lib, Torch)


@pytest.mark.gpu
def test_vec_env_expert_draw_keeps_its_own_counter_gpu(hip_lib):
    """TorchVecEnv.amp_expert_draw: call k equals call k of the host route on a twin context; the scratch grows (n = 70 then 3000) without changing a row"""
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    t = model.load_asset("amp_heading_clips4")
    env = TorchVecEnv(t, 4, seed=SEED, lib_path=hip_lib, amp_obs=True)
    twin = BatchEnv(t, 4, seed=SEED, lib_path=hip_lib)
    a = env.amp_expert_draw(70)
    b, clips, times = env.amp_expert_draw(3000, return_draws=True)
    mine = torch.empty((5, env.env.amp_size), device="cuda")
    assert env.amp_expert_draw(5, out=mine) is mine and env.expert_draw_calls == 3
    assert a.cpu().numpy().tobytes() == twin.amp_expert_clips(70).tobytes()
    assert b.cpu().numpy().tobytes() == twin.amp_expert_clips(3000).tobytes()
    assert mine.cpu().numpy().tobytes() == twin.amp_expert_clips(5).tobytes()
    assert clips.dtype == torch.int32 and times.dtype == torch.float64 and sorted(set(clips.cpu().numpy().tolist())) == [0, 1, 2, 3]
    for bad in (dict(n=0), dict(n=4, out=mine), dict(n=5, out=mine.double())):
        with pytest.raises(ValueError):
            env.amp_expert_draw(**bad)
    env.close(); twin.close()
