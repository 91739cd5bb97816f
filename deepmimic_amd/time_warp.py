"""The test-mode time-warp return of `--scene imitate_amp` for a batch of envs (libdm_hip.so `dm_time_warp_*`, deepmimic_amd/csrc/dm_time_warp.h and
k_time_warp_sample of dm_device.h): cSceneImitateAMP::CalcRewardTimeWarp (scenes/SceneImitateAMP.cpp:174-207, 417-480; util/DynamicTimeWarper.cpp:114-140), the
dynamic-time-warping alignment cost between the joint positions of the simulated and of the kinematic character, sampled at every action boundary and paid once,
at the episode end, plus 1 per sample the episode fell short of the buffer -- the Test_Return the reference's learner logs for an AMP imitation policy.

Per env the caller keeps `capacity` rows of 3J values for each of the two characters, a row count and, for the batch, one overflow word:

    samples [N, 2, capacity, 3J] in the context's precision (0 sim, 1 kin); count int32 [N]; overflow int32 [1]

`sample` appends the state at ENTRY of a control step (in front of the step launch, on the context's stream); an env marked `restart` starts over with two identical
rows, as the reference does behind a reset.  `align` pays the envs of `select`: reward = cost + (capacity - n) * term_step_cost.  The one-env drop-in
(compat/DeepMimicCore) computes the same number on the host; `model.time_warp_cost` is the recurrence in numpy.

Memory: N * 2 * capacity * 3J * sizeof(Real) -- 4096 humanoids (3J = 45) with 20 s test episodes (capacity 602) in fp32: 0.89 GB."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

from .binding import check, vp
from .core import load_library

TERM_STEP_COST = 1.0          # cSceneImitateAMP::CalcRewardTimeWarp: 1 per sample the episode fell short of the buffer


def buffer_size(cfg, query_rate: float) -> Optional[int]:
    """cSceneImitateAMP::BuildTimeWarper: ceil(query rate * max(time_lim_max, time_end_lim_max)) + 2 rows, or None where the reference builds no warper -- a
    scene other than imitate_amp, `enable_test_time_warp` off, or no finite episode length"""
    if cfg.scene != "imitate_amp" or not getattr(cfg, "enable_test_time_warp", True):
        return None
    ends = [x for x in (cfg.time_lim_max, cfg.time_end_lim_max) if x is not None]
    max_time = max(ends) if ends else math.inf
    if not math.isfinite(max_time):
        return None
    return int(math.ceil(query_rate * max_time)) + 2


def why_no_warper(cfg) -> str:
    """the reason `buffer_size` is None, for an error message"""
    if cfg.scene != "imitate_amp":
        return "the scene is `%s`, and only `--scene imitate_amp` has a time-warp return" % cfg.scene
    if not getattr(cfg, "enable_test_time_warp", True):
        return "enable_test_time_warp is off"
    return "the scene has no finite episode length (time_lim_max / time_end_lim_max)"


def dims(env) -> tuple:
    """(bytes per sample element, 3J) of a BatchEnv's context"""
    out = (C.c_int32 * 2)()
    check(env.lib, env.lib.dm_time_warp_dims(env.h, out))
    return int(out[0]), int(out[1])


def buffer_nbytes(num_envs: int, capacity: int, dim: int, elem_bytes: int) -> int:
    return int(num_envs) * 2 * int(capacity) * int(dim) * int(elem_bytes)


def sample_device(env, samples_ptr: int, count_ptr: int, restart_ptr: int, capacity: int, overflow_ptr: int):
    """raw device pointers (restart 0: every env restarts), asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_time_warp_sample(env.h, vp(samples_ptr), vp(count_ptr), vp(restart_ptr), int(capacity), vp(overflow_ptr)))


def align_device(n_envs: int, capacity: int, dim: int, f64: bool, samples_ptr: int, count_ptr: int, select_ptr: int, reward_ptr: int, cost_ptr: int = 0,
                 term_step_cost: float = TERM_STEP_COST, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None, lib=None):
    """raw device pointers (select 0: every env; cost 0: not wanted), asynchronous on the HIP stream `stream` (0 = the null stream) of `device_id`.
    `lib`: an already loaded library (a BatchEnv's) instead of `lib_path`."""
    lib = lib if lib is not None else load_library(lib_path)
    check(lib, lib.dm_time_warp_align(int(device_id), int(n_envs), int(capacity), int(dim), int(bool(f64)), vp(samples_ptr), vp(count_ptr), vp(select_ptr),
                                      float(term_step_cost), vp(reward_ptr), vp(cost_ptr), vp(stream)))


class TimeWarp:
    """The sample buffers, counts and overflow word of a BatchEnv's envs as torch tensors on its GPU, and the two calls on them.  Both are asynchronous on the
    env's current stream (`BatchEnv.set_stream`) and read nothing back; `check_overflow` is the one host read.  `buffers`: (samples, count) views to work on
    instead of tensors of its own -- an env group's rows of whole-batch buffers.  capacity None: `buffer_size` of the scene (ValueError where there is none)."""

    def __init__(self, env, tables=None, capacity: Optional[int] = None, device="cuda:0", buffers=None, term_step_cost: float = TERM_STEP_COST):
        import torch
        self.torch = torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("TimeWarp needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if capacity is None:
            capacity = buffer_size(tables.cfg, tables.query_rate)
            if capacity is None:
                raise ValueError("no time-warp return for this scene: " + why_no_warper(tables.cfg))
        self.env, self.device, self.n, self.capacity, self.term_step_cost = env, dev, int(env.N), int(capacity), float(term_step_cost)
        elem, self.dim = dims(env)
        self.f64 = elem == 8
        dt = torch.float64 if self.f64 else torch.float32
        if buffers is None:
            buffers = (torch.zeros((self.n, 2, self.capacity, self.dim), dtype=dt, device=dev), torch.zeros(self.n, dtype=torch.int32, device=dev))
        self.samples, self.count = buffers
        if tuple(self.samples.shape) != (self.n, 2, self.capacity, self.dim) or self.samples.dtype != dt or not self.samples.is_contiguous() or \
                tuple(self.count.shape) != (self.n,) or self.count.dtype != torch.int32 or not self.count.is_contiguous():
            raise ValueError("buffers must be contiguous (samples %s [%d, 2, %d, %d], count int32 [%d])" % (dt, self.n, self.capacity, self.dim, self.n))
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)

    def sample(self, restart=None):
        """append the envs' current state; `restart`: int32 [n] on this device, != 0 where the env was reset since its last sample (None: every env)"""
        if restart is not None and (restart.dtype != self.torch.int32 or tuple(restart.shape) != (self.n,) or not restart.is_contiguous()):
            raise ValueError("restart must be a contiguous int32 [%d] tensor" % self.n)
        sample_device(self.env, self.samples.data_ptr(), self.count.data_ptr(), restart.data_ptr() if restart is not None else 0, self.capacity, self.overflow.data_ptr())

    def align(self, select=None, out=None, stream: int = 0):
        """(reward float32 [n], cost float64 [n]) of the envs with select != 0 (int32 [n]; None: all), zeros elsewhere; written into `out` if given.
        `stream`: the HIP stream handle to run on -- the one `sample` ran on (0: the null stream)."""
        t = self.torch
        if select is not None and (select.dtype != t.int32 or tuple(select.shape) != (self.n,) or not select.is_contiguous()):
            raise ValueError("select must be a contiguous int32 [%d] tensor" % self.n)
        reward, cost = out if out is not None else (t.empty(self.n, dtype=t.float32, device=self.device), t.empty(self.n, dtype=t.float64, device=self.device))
        align_device(self.n, self.capacity, self.dim, self.f64, self.samples.data_ptr(), self.count.data_ptr(), select.data_ptr() if select is not None else 0,
                     reward.data_ptr(), cost.data_ptr() if cost is not None else 0, self.term_step_cost, stream=stream, device_id=self.device.index,
                     lib=self.env.lib)
        return reward, cost

    def check_overflow(self):
        """one device-to-host copy: RuntimeError if an append found its env's buffer full (cDynamicTimeWarper::AddSample0 throws there)"""
        if int(self.overflow.item()) != 0:
            raise RuntimeError("Time warper buffer overflow, capacity: %d" % self.capacity)
