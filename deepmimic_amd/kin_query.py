"""The reference motion as device tensors at times the caller chooses, and episode starts the caller chooses (libdm_hip.so `dm_kin_query` / `dm_reset_where_at`,
deepmimic_amd/csrc/dm_kin_query.h, k_kin_query and k_env_reset_where_at of dm_device.h).

`dm_link_state(which = 1)` shows the kinematic character where the env's clock stands.  `dm_kin_query` shows it at K times per env: target frames a few control
steps ahead (what motion trackers feed their policies instead of a phase variable), the pose of a candidate start, or another clip of a multi-clip dataset.  The
outputs are float32 with the columns of deepmimic_amd/link_state.py and one more axis:

    links [N, K, J, 22]    env [N, K, 8]    pose, vel [N, K, P]

`times` is float64, [K] shared by all envs or [N, K] with TIMES_PER_ENV.  A time is an offset added to the env's clip clock (negative offsets are allowed), or a
clip time with TIMES_ABSOLUTE; only then may `clips` (int32 [N]) name another clip of the dataset.  ORIGIN_IDENTITY samples about the identity origin instead of
the env's own: the clip in its own frame, which is what a start candidate looks like.  A looping clip adds cycle x cycle_delta to the root, a clip that does not
loop clamps to its first / last frame and rests from its end on.  The heading / root sync a phase wrap of the env's clock would apply on the way is not
anticipated.  A non-finite time or a clip id outside the dataset gives NaN rows for that (env, k).

`dm_reset_where_at` is `dm_reset_where` with the start handed in: per selected env `clips[i] >= 0`, a finite `times[i]`, a finite `yaw[i]` are taken, -1 / NaN /
a missing array are drawn.  Nothing given is exactly `dm_reset_where` (recovery episodes included); anything given is a full scene reset: the time limit is drawn
as always, a clip that is not given by weight, a time that is not given uniformly over the clip the episode starts on, a yaw that is not given is 0 when the time
is given and the scene's rule otherwise.  An env with an invalid value (clip id outside the dataset, negative or infinite time, infinite yaw) keeps every byte
and `bad[0]` becomes 1.

Both calls are asynchronous on the env's stream and read nothing back."""
from __future__ import annotations

import ctypes as C

from .binding import check, vp
from .link_state import dims

TIMES_PER_ENV, TIMES_ABSOLUTE, ORIGIN_IDENTITY = 1, 2, 4
MAX_K = 64


def flags_of(per_env: bool = False, absolute: bool = False, identity_origin: bool = False) -> int:
    return (TIMES_PER_ENV if per_env else 0) | (TIMES_ABSOLUTE if absolute else 0) | (ORIGIN_IDENTITY if identity_origin else 0)


def kin_query_device(env, K: int, times_ptr: int, clips_ptr: int = 0, flags: int = 0, links_ptr: int = 0, env_ptr: int = 0, pose_ptr: int = 0, vel_ptr: int = 0):
    """raw device pointers (0: output not wanted; clips 0: the env's own clip), asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_kin_query(env.h, int(K), vp(times_ptr), vp(clips_ptr), int(flags), vp(links_ptr), vp(env_ptr), vp(pose_ptr), vp(vel_ptr)))


def reset_where_at_device(env, mask_ptr: int, clips_ptr: int = 0, times_ptr: int = 0, yaw_ptr: int = 0, states_ptr: int = 0, goals_ptr: int = 0, bad_ptr: int = 0):
    """raw device pointers: int32 [N] mask, int32 [N] clips (0 or -1 rows: drawn), float64 [N] times and yaw (0 or NaN rows: drawn), float32 [N, S] states,
    float32 [N, G] goals (0: not wanted), int32 [1] bad (0: not wanted; the caller zeroes it); asynchronous on the stream of `env`"""
    check(env.lib, env.lib.dm_reset_where_at(env.h, vp(mask_ptr), vp(clips_ptr), vp(times_ptr), vp(yaw_ptr), vp(states_ptr), vp(goals_ptr), vp(bad_ptr)))


class KinQuery:
    """The kinematic character of a BatchEnv's envs at K times each, on its GPU: `links` [N, K, J, 22], `env_state` [N, K, 8], `pose`, `vel` [N, K, P].
    `update(times, clips=None, ...)` refreshes them asynchronously on the env's current stream; `times` is a float64 device tensor [K] or [N, K] (the shape
    decides TIMES_PER_ENV), `clips` an int32 device tensor [N] (absolute times only)."""

    def __init__(self, env, K: int, device="cuda:0"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("KinQuery needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= int(K) <= MAX_K:
            raise ValueError("K must be in [1, %d]" % MAX_K)
        self.env, self.K, self.device = env, int(K), dev
        J, lw, ew, P, _ = dims(env)
        f32 = dict(dtype=torch.float32, device=dev)
        self.links = torch.zeros((env.N, self.K, J, lw), **f32); self.env_state = torch.zeros((env.N, self.K, ew), **f32)
        self.pose = torch.zeros((env.N, self.K, P), **f32); self.vel = torch.zeros((env.N, self.K, P), **f32)

    def update(self, times, clips=None, absolute: bool = False, identity_origin: bool = False):
        import torch
        if times.dtype != torch.float64 or not times.is_cuda or not times.is_contiguous():
            raise ValueError("times must be a contiguous float64 tensor on the GPU")
        if tuple(times.shape) not in ((self.K,), (self.env.N, self.K)):
            raise ValueError("times must have shape [K] or [N, K] with K = %d" % self.K)
        if clips is not None and (clips.dtype != torch.int32 or not clips.is_cuda or not clips.is_contiguous() or tuple(clips.shape) != (self.env.N,)):
            raise ValueError("clips must be a contiguous int32 tensor [N] on the GPU")
        # (an [N, K] tensor with N == 1 and a [K] tensor address the same words)
        kin_query_device(self.env, self.K, times.data_ptr(), clips.data_ptr() if clips is not None else 0, flags_of(times.dim() == 2, absolute, identity_origin),
                         self.links.data_ptr(), self.env_state.data_ptr(), self.pose.data_ptr(), self.vel.data_ptr())
        return self

    def info(self, prefix: str = "kin_ahead_") -> dict:
        """the tensors under the keys TorchVecEnv.step hands out"""
        return {prefix + "link_state": self.links, prefix + "link_env": self.env_state, prefix + "pose": self.pose, prefix + "vel": self.vel}
