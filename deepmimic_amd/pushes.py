"""Task-chosen pushes: forces on body parts from device tensors, and the forces that are acting, for tasks written in torch (libdm_hip.so `dm_push_where` /
`dm_push_state`, deepmimic_amd/csrc/dm_push.h, k_push_where and k_push_state of dm_device.h).

The step kernels apply up to two forces per env at a body part's centre of mass, for whole scene updates: the machinery of `--enable_rand_perturbs`.  `dm_push_where`
writes a force the TASK chose into one of the two slots of the envs a device mask selects -- a push curriculum, per-env magnitudes, a push when a task event
happens, a push "from the character's left" (frame="heading"), an adversary's pushes -- and `dm_push_state` hands out what is acting as float32 rows:

    pushes [N, 2, 6]   PUSH_LINK 0: the body part (-1: a free slot, the other columns are 0); PUSH_FORCE 1:4 the force in world coordinates (N);
                       PUSH_DURATION 4 and PUSH_ELAPSED 5 in seconds.  A push acts while elapsed < duration, for whole scene updates: ceil(duration / dt) of them.

The context needs the perturbation rows: `SceneConfig.task_pushes = True` (`TorchVecEnv(..., pushes=True)` sets it on its own copy of the config), or
`enable_rand_perturbs` with a finite interval, in which case the random schedule and the task share the two slots.  Every scene reset clears both slots; a state-pool
slot carries the pushes stored in it.  Both calls are asynchronous on the env's stream and read nothing back."""
from __future__ import annotations

import numpy as np

from .binding import check, vp

PUSH_SLOTS, PUSH_W = 2, 6
PUSH_LINK, PUSH_FORCE, PUSH_DURATION, PUSH_ELAPSED = 0, slice(1, 4), 4, 5
WORLD, HEADING = 0, 1                                   # DM_PUSH_WORLD, DM_PUSH_HEADING
FRAMES = {"world": WORLD, "heading": HEADING}


def frame_flag(frame) -> int:
    if frame not in FRAMES:
        raise ValueError("frame must be 'world' or 'heading' (got %r)" % (frame,))
    return FRAMES[frame]


def push_where_device(env, mask_ptr: int, links_ptr: int, forces_ptr: int, durations_ptr: int, slots_ptr: int = 0, flags: int = WORLD, bad_ptr: int = 0):
    """raw device pointers: int32 [N] mask, int32 [N] links (-1: clear), float64 [N, 3] forces, float64 [N] durations, int32 [N] slots (0: the rule of a drawn force),
    int32 [1] bad (0: not wanted; the caller zeroes it); asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_push_where(env.h, vp(mask_ptr), vp(links_ptr), vp(forces_ptr), vp(durations_ptr), vp(slots_ptr), int(flags), vp(bad_ptr)))


def push_state_device(env, out_ptr: int):
    """raw device pointer: float32 [N, 2, 6]; asynchronous on the stream of `env` (a BatchEnv)"""
    check(env.lib, env.lib.dm_push_state(env.h, vp(out_ptr)))


# ---- host arrays (BatchEnv.push / clear_pushes / push_state): these run on the CPU emulator too
def _mask(env, mask):
    m = np.asarray(mask)
    return (m.reshape(env.N) != 0).astype(np.int32) if m.dtype == bool else np.ascontiguousarray(m, dtype=np.int32).reshape(env.N)


def push_host(env, mask, links, forces, durations, slots=None, frame="world") -> int:
    """BatchEnv.push: dm_push_where from host arrays (scalars and single rows are broadcast over the envs); returns bad"""
    specs = {"mask": ((env.N,), np.int32), "links": ((env.N,), np.int32), "forces": ((env.N, 3), np.float64), "durations": ((env.N,), np.float64), "bad": ((1,), np.int32)}
    over = lambda x, dtype, shape: np.array(np.broadcast_to(np.asarray(x, dtype=dtype), shape))      # (a copy: a broadcast view is read-only)
    init = {"mask": _mask(env, mask), "links": over(links, np.int32, (env.N,)), "forces": over(forces, np.float64, (env.N, 3)), "durations": over(durations, np.float64, (env.N,))}
    if slots is not None:
        specs["slots"] = ((env.N,), np.int32); init["slots"] = over(slots, np.int32, (env.N,))
    ptr, fetch = env._dev_arrays(specs, init)
    push_where_device(env, ptr["mask"], ptr["links"], ptr["forces"], ptr["durations"], ptr.get("slots", 0), frame_flag(frame), ptr["bad"])
    return int(fetch()["bad"][0])


def push_state_host(env):
    ptr, fetch = env._dev_arrays({"pushes": ((env.N, PUSH_SLOTS, PUSH_W), np.float32)})
    push_state_device(env, ptr["pushes"])
    return fetch()["pushes"]


class RandomPushes:
    """A ready-made push sampler for `make_agent(..., push_fn=)` (or a loop of one's own: `env.push(**sampler(info, t))` before `env.step`), in the style of
    state_init.VisitedStateStarts: a seeded generator on the env's device and a countdown per env, in control steps.  When an env's countdown runs out it is pushed
    -- a uniformly drawn direction, a magnitude drawn from U[magnitude], a duration from U[duration] seconds, on a body part drawn from `links` (None: any) -- and
    its next countdown is drawn from the integers of `interval` = (lo, hi), both included.  `magnitude` is a pair (lo, hi) in newtons, or a float32 / float64 tensor
    [N, 2] on the env's device that the task may update between calls: per-env ranges, i.e. the curriculum.  Everything stays on the device: no host read per call
    (the dict asks `env.push` not to check), and two samplers of one seed on two envs of one seed hand out the same tensors.  The tensors of the last call stay
    readable as `mask`, `links`, `forces`, `durations`."""

    def __init__(self, env, interval=(30, 90), magnitude=(50.0, 200.0), duration=(0.1, 0.3), links=None, seed: int = 0, frame: str = "world"):
        import torch
        if not getattr(env, "has_pushes", False):
            raise ValueError("RandomPushes needs a TorchVecEnv with pushes=True (or a scene with enable_rand_perturbs)")
        lo, hi = int(interval[0]), int(interval[1])
        if not 1 <= lo <= hi:
            raise ValueError("interval must be 1 <= lo <= hi control steps")
        if not 0.0 <= float(duration[0]) <= float(duration[1]):
            raise ValueError("duration must be 0 <= lo <= hi seconds")
        self.env, self.interval, self.duration, self.frame = env, (lo, hi), (float(duration[0]), float(duration[1])), frame
        frame_flag(frame)
        dev, n = env.device, env.n
        if isinstance(magnitude, torch.Tensor):
            if magnitude.device != dev or tuple(magnitude.shape) != (n, 2) or magnitude.dtype not in (torch.float32, torch.float64):
                raise ValueError("magnitude must be a pair or a float tensor [N, 2] on %s" % dev)
            self.magnitude = magnitude                                # the task's tensor, read at every call
        else:
            if not 0.0 <= float(magnitude[0]) <= float(magnitude[1]):
                raise ValueError("magnitude must be 0 <= lo <= hi newtons")
            self.magnitude = torch.tensor([float(magnitude[0]), float(magnitude[1])], dtype=torch.float64, device=dev).expand(n, 2)
        ids = list(range(env.env.J)) if links is None else [int(b) for b in links]
        if not ids or any(b < 0 or b >= env.env.J for b in ids):
            raise ValueError("links must name body parts of the character: [0, %d)" % env.env.J)
        self._links = torch.tensor(ids, dtype=torch.int32, device=dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(int(seed))
        self.countdown = torch.randint(lo, hi + 1, (n,), generator=self.gen, device=dev, dtype=torch.int32)
        self.mask = torch.zeros(n, dtype=torch.int32, device=dev)
        self.links = torch.zeros(n, dtype=torch.int32, device=dev)
        self.forces = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.durations = torch.zeros(n, dtype=torch.float64, device=dev)

    def __call__(self, info=None, t=None) -> dict:
        import torch
        n, dev, g = self.env.n, self.env.device, self.gen
        lo, hi = self.interval
        self.countdown -= 1
        fire = self.countdown <= 0
        nxt = torch.randint(lo, hi + 1, (n,), generator=g, device=dev, dtype=torch.int32)
        d = torch.randn((n, 3), generator=g, device=dev, dtype=torch.float64)
        u = torch.rand((n, 2), generator=g, device=dev, dtype=torch.float64)
        pick = torch.randint(0, self._links.numel(), (n,), generator=g, device=dev)
        self.countdown.copy_(torch.where(fire, nxt, self.countdown))
        self.mask.copy_(fire)
        mag = self.magnitude.to(torch.float64)
        mag = mag[:, 0] + (mag[:, 1] - mag[:, 0]) * u[:, 0]
        norm = d.norm(dim=1, keepdim=True).clamp_min(1e-300)
        torch.mul(d / norm, mag.unsqueeze(1), out=self.forces)
        self.durations.copy_(self.duration[0] + (self.duration[1] - self.duration[0]) * u[:, 1])
        self.links.copy_(self._links[pick])
        return {"mask": self.mask, "links": self.links, "forces": self.forces, "durations": self.durations, "frame": self.frame, "check": False}
