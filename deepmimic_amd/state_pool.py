"""A pool of whole env records in device memory (libdm_hip.so `dm_state_pool_*` / `dm_state_save` / `dm_state_restore`, deepmimic_amd/csrc/dm_state_pool.h,
k_state_save and k_state_restore of dm_device.h).

`BatchEnv.snapshot()` / `restore()` hold a simulator state on the host, for all N envs at once.  A pool holds M records on the device; the envs a device mask
selects write their record into, or take it from, the slot a per-env index names.  Nothing is read back and everything runs on the env's stream, so a task written
in torch can start episodes from states the policy has visited (deepmimic_amd/state_init.py), rewind selected envs to a checkpoint, or branch one state into many
envs.

A slot is one env's record in the context's precision -- pose, vel, tar, tau, kin, clock, flag and, where the context has them, hist, obj, goal, pert, manif --
with every segment on a 16-byte boundary (`dims`).  It holds no pointer and no env id: the pool is data, `clone()` and `state_dict()` carry it.  Three things belong
to the env and not to its state and are left alone by a restore: the diagnostic counters, and the env's own draw key in the goal and perturbation rows.

`restore(..., new_episode=False)` (REWIND) puts back the record as stored, the AMP pose history included: the same actions reproduce the stored rollout bit for bit
on the env that saved it.  `new_episode=True` (NEW_EPISODE) starts a new episode at the stored state: the destination keeps its episode counter (advanced by one)
and its goal / perturbation draw counters, the episode timer starts over with a freshly drawn limit, the pose history is re-initialised.  Either way the restored
envs' rows of `states` / `goals` receive the observation and goal a zero-update step would hand back.

A slot index outside [0, slots) leaves that env as it is and sets `bad[0]`.  Two envs that save into one slot in one call break the contract (the slot's content is
then unspecified); many envs may restore from one slot."""
from __future__ import annotations

import copy
import ctypes as C

from .binding import check, vp

REWIND, NEW_EPISODE = 0, 1
SEGMENTS = ("pose", "vel", "tar", "tau", "kin", "clock", "flag", "hist", "obj", "goal", "pert", "manif")


def dims(env) -> dict:
    """{"slot_bytes": the size of one record, "offsets": {segment: byte offset inside a slot}} of a BatchEnv's context; a row the context lacks has no offset"""
    out = (C.c_int32 * (1 + len(SEGMENTS)))()
    check(env.lib, env.lib.dm_state_pool_dims(env.h, out))
    return {"slot_bytes": int(out[0]), "offsets": {name: int(out[1 + k]) for k, name in enumerate(SEGMENTS) if out[1 + k] >= 0}}


def pool_bytes(env, slots: int) -> int:
    """the size of a pool of `slots` records of a BatchEnv's context"""
    n = int(env.lib.dm_state_pool_bytes(env.h, int(slots)))
    if n < 0:
        check(env.lib, -1)
    return n


def save_device(env, pool_ptr: int, slots: int, mask_ptr: int, slots_ptr: int, bad_ptr: int = 0):
    """raw device pointers: the pool (16-byte aligned, pool_bytes(env, slots)), int32 [N] mask, int32 [N] slot per env, int32 [1] bad (0: not wanted; the caller
    zeroes it); asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_state_save(env.h, vp(pool_ptr), int(slots), vp(mask_ptr), vp(slots_ptr), vp(bad_ptr)))


def restore_device(env, pool_ptr: int, slots: int, mask_ptr: int, slots_ptr: int, flags: int = REWIND, states_ptr: int = 0, goals_ptr: int = 0, bad_ptr: int = 0):
    """raw device pointers as save_device; float32 [N, S] states and [N, G] goals (0: not wanted) receive the rows of the restored envs; flags: REWIND or NEW_EPISODE"""
    check(env.lib, env.lib.dm_state_restore(env.h, vp(pool_ptr), int(slots), vp(mask_ptr), vp(slots_ptr), int(flags), vp(states_ptr), vp(goals_ptr), vp(bad_ptr)))


class StatePool:
    """`slots` records of a BatchEnv's envs on its GPU: `data` (uint8 [slots, slot_bytes]) and `bad` (int32 [1], becomes 1 when a call named a slot outside the
    pool; nobody reads it on the way).  `save` / `restore` take int32 device tensors [N] (a bool mask is converted) and run asynchronously on the env's current
    stream.  `states` / `goals`: float32 [N, S] / [N, G] tensors whose rows of restored envs are overwritten."""

    def __init__(self, env, slots: int, device="cuda:0"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("StatePool needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if int(slots) < 1:
            raise ValueError("slots must be positive")
        self.env, self.slots, self.device = env, int(slots), dev
        self.slot_bytes = pool_bytes(env, 1)
        self.data = torch.zeros((self.slots, self.slot_bytes), dtype=torch.uint8, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def _i32(self, name, x):
        import torch
        if isinstance(x, torch.Tensor) and x.dtype == torch.bool:
            x = x.to(torch.int32)
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.device != self.device or tuple(x.shape) != (self.env.N,) or not x.is_contiguous():
            raise ValueError("%s must be a contiguous int32 (or bool) tensor [N] on %s" % (name, self.device))
        return x

    def _f32(self, name, x, width):
        import torch
        if x is None:
            return 0
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.device or tuple(x.shape) != (self.env.N, width) or not x.is_contiguous():
            raise ValueError("%s must be a contiguous float32 tensor [N, %d] on %s" % (name, width, self.device))
        return x.data_ptr()

    def save(self, mask, slots):
        mask, slots = self._i32("mask", mask), self._i32("slots", slots)
        save_device(self.env, self.data.data_ptr(), self.slots, mask.data_ptr(), slots.data_ptr(), self.bad.data_ptr())
        return self

    def restore(self, mask, slots, new_episode: bool = False, states=None, goals=None):
        mask, slots = self._i32("mask", mask), self._i32("slots", slots)
        if goals is not None and not self.env.G:
            raise ValueError("goals on a scene without a goal")
        restore_device(self.env, self.data.data_ptr(), self.slots, mask.data_ptr(), slots.data_ptr(), NEW_EPISODE if new_episode else REWIND,
                       self._f32("states", states, self.env.S), self._f32("goals", goals, self.env.G), self.bad.data_ptr())
        return self

    def clone(self):
        """a second pool with the same bytes (a copy on torch's current stream)"""
        other = copy.copy(self)
        other.data, other.bad = self.data.clone(), self.bad.clone()
        return other

    def state_dict(self) -> dict:
        return {"data": self.data, "slot_bytes": self.slot_bytes, "slots": self.slots}

    def load_state_dict(self, sd: dict):
        """takes the records of a pool of the same slot size and slot count (a context of the same scene and precision); anything else is refused"""
        if int(sd["slot_bytes"]) != self.slot_bytes:
            raise ValueError("the pool's slot size is %d bytes, this context's is %d: not a pool of this scene and precision" % (int(sd["slot_bytes"]), self.slot_bytes))
        if int(sd["slots"]) != self.slots or tuple(sd["data"].shape) != (self.slots, self.slot_bytes):
            raise ValueError("the pool holds %d slots, this one %d" % (int(sd["slots"]), self.slots))
        self.data.copy_(sd["data"])
        return self
