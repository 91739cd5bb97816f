"""Episode starts from states the policy has visited: a ready-made start sampler for `TorchVecEnv.set_start_sampler` on top of the device state pool
(deepmimic_amd/state_pool.py).

    env = TorchVecEnv(tables, n, deferred_reset=True); env.reset()
    env.set_start_sampler(VisitedStateStarts(env, slots=1024, saves_per_step=8, start_fraction=0.3, seed=1))

The pool is a ring of `slots` records.  At construction every slot is filled from the envs' current states (in chunks of at most N envs, so that the slots of one
call are distinct).  At every step `saves_per_step` distinct envs, drawn from a seeded generator on the device, write their end-of-step state into the next ring
positions -- a position is skipped where the drawn env's episode has just ended, its state is the end of an episode, not a place to start one -- and every done env
starts its next episode from a uniformly drawn slot with probability `start_fraction`, else where the device draws it on the reference motion.  Everything stays on
the device: no host read per step, and two samplers of one seed on two envs of one seed hand out the same tensors.  The agents need no change: they take the env as
it is."""
from __future__ import annotations


class VisitedStateStarts:
    def __init__(self, env, slots: int, saves_per_step: int = 1, start_fraction: float = 0.5, seed: int = 0):
        import torch
        if not env.deferred_reset:
            raise ValueError("VisitedStateStarts needs a TorchVecEnv with deferred_reset=True")
        if not 0 <= int(saves_per_step) <= env.n:
            raise ValueError("saves_per_step must be in [0, N]: the envs of one save are distinct")
        if not 0.0 <= float(start_fraction) <= 1.0:
            raise ValueError("start_fraction must be in [0, 1]")
        self.env, self.slots, self.saves, self.fraction = env, int(slots), int(saves_per_step), float(start_fraction)
        self.pool = env.state_pool(self.slots)
        self.gen = torch.Generator(device=env.device)
        self.gen.manual_seed(int(seed))
        self.cursor = 0                                             # the next ring position (host side: it advances by saves_per_step whatever the device drew)
        i32 = dict(dtype=torch.int32, device=env.device)
        self._arange = torch.arange(env.n, **i32)
        self._mask, self._slots = torch.zeros(env.n, **i32), torch.zeros(env.n, **i32)
        self.start_slots = torch.full((env.n,), -1, **i32)         # what the last call handed to the env
        for first in range(0, self.slots, env.n):
            k = min(env.n, self.slots - first)
            self.pool.save((self._arange < k).to(torch.int32), self._arange + first)

    def __call__(self, done_i32, info):
        import torch
        n = self.env.n
        if self.saves:
            envs = torch.randperm(n, generator=self.gen, device=self.env.device)[:self.saves]
            pos = (torch.arange(self.saves, device=self.env.device) + self.cursor) % self.slots
            self.cursor = (self.cursor + self.saves) % self.slots
            self._mask.zero_()
            self._mask[envs] = 1 - done_i32[envs]                   # (distinct indices: no write meets another)
            self._slots.zero_()
            self._slots[envs] = pos.to(torch.int32)
            self.pool.save(self._mask, self._slots)
        u = torch.rand(n, generator=self.gen, device=self.env.device)
        pick = torch.randint(0, self.slots, (n,), generator=self.gen, device=self.env.device, dtype=torch.int32)
        torch.where((done_i32 != 0) & (u < self.fraction), pick, torch.full_like(pick, -1), out=self.start_slots)
        return {"slots": self.start_slots}
