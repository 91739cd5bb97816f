"""Times of one iteration's discriminator data stage (deepmimic_amd/csrc/dm_replay.h, deepmimic_amd/replay.py) at rollout size against the same stage written with
public torch calls on the same tensors:
  (a) expert rows   TorchVecEnv.amp_expert_draw(n_valid) (draw kernel + expert kernel, no host copy)   vs   BatchEnv.amp_expert_clips(n_valid) (host draws, staged copies)
  (b) two appends   agent rows over the valid list with the packed rows, expert rows dense               vs   torch_append below (nonzero, randperm victims, index_copy_)
  (c) sample pair   one sample of the discriminator batch from each store                                vs   torch_sample below (randint + index_select)
  (d) the stage     (a) + (b) + (c) in one timed window, kernels only
The pairs run interleaved in one process, each call timed with HIP events on the current stream (the host route of (a), which synchronises, with a host clock);
medians over the timed repetitions after a warm-up, with the quartiles next to them.  The torch side stands for what a learner writes without the kernels; its
nonzero() waits for the device, which the event timing includes.  Both sides start every repetition from a full store (the steady state of training).
Writes one JSON object (default profiles/replay_bench.json).
usage: python tools/replay_bench.py [--T 32] [--N 4096] [--capacity 100000] [--batch 256] [--reps 100] [--warmup 10] [--scene amp_heading_clips4] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import model, ppo_batch, replay  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


class TorchStore:
    """learning/replay_buffer_rand_storage.py in public torch ops"""
    def __init__(self, capacity, width):
        self.buf, self.size, self.cap = torch.zeros((capacity, width), device="cuda"), 0, capacity

    def append(self, rows):
        n = rows.shape[0]
        if n > self.cap:                   # (the reference asserts n < buffer_size: keep a random subset, as the kernels do)
            rows = rows[torch.randperm(n, device="cuda")[:self.cap]]; n = self.cap
        fresh = min(n, self.cap - self.size)
        if fresh:
            self.buf[self.size:self.size + fresh] = rows[:fresh]
        if n > fresh:
            victims = torch.randperm(self.size, device="cuda")[:n - fresh]
            self.buf.index_copy_(0, victims, rows[fresh:])
        self.size = min(self.size + n, self.cap)

    def sample(self, rows):
        return self.buf.index_select(0, torch.randint(0, self.size, (rows,), device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32); ap.add_argument("--N", type=int, default=4096); ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--reps", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scene", default="amp_heading_clips4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_bench.json"))
    a = ap.parse_args()
    T, N, B, CAP = a.T, a.N, a.batch, a.capacity
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench needs a GPU (deepmimic_amd has no CPU path)")
    env = TorchVecEnv(model.load_asset(a.scene), 64, seed=1, amp_obs=True)          # the scene's clips serve the expert rows; the agent rows are synthetic
    W = env.env.amp_size
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    amp = torch.randn((T, N, W), generator=g, device="cuda")
    mask = (torch.rand((T, N), generator=g, device="cuda") >= 0.2).int()
    zeros = torch.zeros((T, N), device="cuda")
    kb = ppo_batch.advantages_torch(zeros, zeros, mask, None)
    n_valid, _ = kb.counts_host()
    agent, expert = replay.DeviceReplayStore(CAP, W, seed=2), replay.DeviceReplayStore(CAP, W, seed=3)
    t_agent, t_expert = TorchStore(CAP, W), TorchStore(CAP, W)
    packed, expert_rows = torch.zeros((T * N, W), device="cuda"), torch.zeros((n_valid, W), device="cuda")

    def k_expert():
        env.amp_expert_draw(n_valid, out=expert_rows)

    def k_append():
        agent.append_batch(amp, kb, packed=packed); expert.append(expert_rows)

    def k_sample():
        return agent.sample(B), expert.sample(B)

    def t_append():
        idx = (mask.reshape(-1) != 0).nonzero().squeeze(1)
        rows = amp.reshape(T * N, W).index_select(0, idx)          # (the packed rows the normaliser records)
        t_agent.append(rows); t_expert.append(expert_rows)
        return rows

    def t_sample():
        return t_agent.sample(B), t_expert.sample(B)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3          # us

    def host_clock(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    # agreement: the kernels' stores against the numpy statement, from a cleared store
    k_expert(); k_append()
    slots = replay.reference_append_slots(0, CAP, n_valid, 2, 0)
    valid = (mask.reshape(-1) != 0).nonzero().squeeze(1)
    want = torch.zeros((CAP, W), device="cuda"); s = torch.from_numpy(slots).cuda().long()
    want[s[s >= 0]] = amp.reshape(T * N, W)[valid][s >= 0]
    picked = agent.sample(B, picked=True)
    agree = dict(agent_store_equals_reference=bool((agent.buf == want).all()), packed_rows_equal_valid_rows=bool((packed[:n_valid] == amp.reshape(T * N, W)[valid]).all()),
                 state=list(agent.state_host()), sample_slots_equal_reference=bool((picked[1].cpu().numpy() == replay.reference_sample_slots(min(n_valid, CAP), B, 2, 0)).all()),
                 sample_rows_equal_store_rows=bool((picked[0] == agent.buf[picked[1].long()]).all()))
    runs = dict(expert_rows_kernels=k_expert, expert_rows_host_route=lambda: env.env.amp_expert_clips(n_valid), appends_kernels=k_append, appends_torch_ops=t_append,
                sample_pair_kernels=k_sample, sample_pair_torch_ops=t_sample, stage_kernels=lambda: (k_expert(), k_append(), k_sample()),
                stage_torch_ops_without_expert=lambda: (t_append(), t_sample()))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            times[k].append(host_clock(fn) if k == "expert_rows_host_route" else timed(fn))
    q = lambda x: [float(np.percentile(x, p)) for p in (25, 50, 75)]
    med = {k: float(np.median(v)) for k, v in times.items()}
    append_bytes = 4 * W * (3 * n_valid + 2 * n_valid)          # agent rows read once and written twice (store, packed); expert rows read and written once
    out = dict(what="AMP discriminator data stage: hand-written kernels vs the same stage in public torch ops, interleaved in one process, HIP events, microseconds (every "
                    "time includes the Python / ctypes launch path; the torch appends include the host wait of nonzero(); the expert host route is a host clock "
                    "around a call that synchronises); both kinds of store are full from the second repetition on",
               T=T, N=N, width=W, capacity=CAP, batch=B, n_valid=n_valid, scene=a.scene, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               append_tile="one wavefront per workgroup, 16 list rows per wavefront: lanes 0..15 settle the slots, 64 lanes copy the tile, 8 loads in flight per lane",
               us_q25_median_q75={k: q(v) for k, v in times.items()},
               torch_over_kernels=dict(appends=med["appends_torch_ops"] / med["appends_kernels"], sample_pair=med["sample_pair_torch_ops"] / med["sample_pair_kernels"],
                                       expert_rows_host_route=med["expert_rows_host_route"] / med["expert_rows_kernels"]),
               append_bytes_moved=append_bytes, appends_kernels_bytes_per_s=append_bytes / (med["appends_kernels"] * 1e-6), agreement=agree)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
