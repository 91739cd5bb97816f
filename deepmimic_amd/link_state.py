"""Link states as device tensors, and the reset selected by a device mask, for tasks written in torch (libdm_hip.so `dm_link_state*` / `dm_reset_where`,
deepmimic_amd/csrc/dm_link_state.h, k_link_state and k_env_reset_where of dm_device.h).

Link positions, body rotations, link velocities and the centre of mass are what a custom reward or observation in this domain is made of: a hand reaching a target,
a foot height, a heading, a per-link tracking error.  `dm_link_state` runs the forward kinematics of every env's record as it stands -- of the simulated character
(`which` = 0) or of the kinematic one (`which` = 1: the env's clip at the env's clip time) -- and writes float32 rows, whatever the context's precision:

    links [N, J, 22]   LINK_COM 0:3 link COM world position; LINK_ROT 3:12 body world rotation, row-major; LINK_VEL 12:15 COM linear velocity; LINK_ANG_VEL 15:18
                       angular velocity; LINK_JOINT_POS 18:21 joint world position; LINK_CONTACT 21: 1.0 where the link touched something in the last substep
                       (bit j of flags[:, 1] of BatchEnv.get_state; 0 for the kinematic character)
    env   [N, 8]       ENV_COM 0:3 character COM, ENV_COM_VEL 3:6 its velocity, ENV_HEADING 6 the root heading (the origin frame of the observation is
                       rot_y(-heading)), 7 unused (0)
    pose, vel [N, P]   the pose and velocity the link state was computed from (which = 1: the sampled clip pose)
    obj   [N, 13]      dribble_amp's ball: position, rotation w x y z, linear and angular velocity

`dm_reset_where` starts a new episode for the envs a device mask selects, exactly as an auto-reset launch does for an env whose episode ended.  A control step then
becomes: step launch without auto-reset, link state, masked reset -- the link state describes the true end of the step for every env, finished ones included, and
the step still returns what the auto-reset step returns (`TorchVecEnv(..., deferred_reset=True)`).

Both calls are asynchronous on the env's stream and read nothing back."""
from __future__ import annotations

import ctypes as C

from .binding import check, vp

LINK_W, ENV_W, OBJ_W = 22, 8, 13
LINK_COM, LINK_ROT, LINK_VEL, LINK_ANG_VEL, LINK_JOINT_POS, LINK_CONTACT = slice(0, 3), slice(3, 12), slice(12, 15), slice(15, 18), slice(18, 21), 21
ENV_COM, ENV_COM_VEL, ENV_HEADING = slice(0, 3), slice(3, 6), 6
SIM, KIN = 0, 1


def dims(env) -> tuple:
    """(J, 22, 8, P, 13 or 0) of a BatchEnv's context: the row widths of links, env, pose / vel and obj (0: no free body)"""
    out = (C.c_int32 * 5)()
    check(env.lib, env.lib.dm_link_state_dims(env.h, out))
    return tuple(int(x) for x in out)


def link_state_device(env, which: int, links_ptr: int = 0, env_ptr: int = 0, pose_ptr: int = 0, vel_ptr: int = 0, obj_ptr: int = 0):
    """raw device pointers (0: output not wanted), asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_link_state(env.h, int(which), vp(links_ptr), vp(env_ptr), vp(pose_ptr), vp(vel_ptr), vp(obj_ptr)))


def reset_where_device(env, mask_ptr: int, states_ptr: int, goals_ptr: int = 0):
    """raw device pointers: int32 [N] mask, float32 [N, S] states, float32 [N, G] goals (0: not wanted); asynchronous on the stream of `env`"""
    check(env.lib, env.lib.dm_reset_where(env.h, vp(mask_ptr), vp(states_ptr), vp(goals_ptr)))


class LinkState:
    """The link-state tensors of one character (`which`: SIM or KIN) of a BatchEnv's envs on its GPU: `links`, `env`, `pose`, `vel` and, where the scene has a ball
    and which == SIM, `obj` (None otherwise).  `update()` refreshes them from the context's current state, asynchronously on the env's current stream."""

    def __init__(self, env, which: int = SIM, device="cuda:0"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("LinkState needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if which not in (SIM, KIN):
            raise ValueError("which must be SIM (0) or KIN (1)")
        self.env, self.which, self.device = env, int(which), dev
        J, lw, ew, P, ow = dims(env)
        f32 = dict(dtype=torch.float32, device=dev)
        self.links = torch.zeros((env.N, J, lw), **f32); self.env_state = torch.zeros((env.N, ew), **f32)
        self.pose = torch.zeros((env.N, P), **f32); self.vel = torch.zeros((env.N, P), **f32)
        self.obj = torch.zeros((env.N, ow), **f32) if (ow and self.which == SIM) else None

    def update(self):
        link_state_device(self.env, self.which, self.links.data_ptr(), self.env_state.data_ptr(), self.pose.data_ptr(), self.vel.data_ptr(),
                          self.obj.data_ptr() if self.obj is not None else 0)
        return self

    def info(self, prefix: str = "") -> dict:
        """the tensors under the keys TorchVecEnv.step hands out"""
        d = {prefix + "link_state": self.links, prefix + "link_env": self.env_state, prefix + "pose": self.pose, prefix + "vel": self.vel}
        if self.obj is not None:
            d[prefix + "obj_state"] = self.obj
        return d
