"""Times of the AMP batch-reward stage (deepmimic_amd/csrc/dm_amp_rewards.h, deepmimic_amd/amp_rewards.py), one process, the two arms alternating, whole calls
bracketed by HIP events on the current stream, every repetition kept:
  device   AmpRewards.update_torch on a [T, N] rollout (four launches, no host read) + AmpRewards.clip_torch of [T + 1, N] values (one launch)
  torch    the same result in public torch ops on the same tensors: the mask by a backward pass over the T rows, the style reward and its blend, mean / std
           over the counted rows, min / max into running bounds on the host -- the two `.item()` reads a learner needs to rebuild `Critic(lo, hi)` -- and the clip.
No ratio is the point: the device arm ends without a synchronisation, the torch arm cannot.  Writes one JSON object (default profiles/amp_rewards_bench.json).
usage: python tools/amp_rewards_bench.py [--T 32] [--N 4096] [--reps 50] [--warmup 10] [--out profiles/amp_rewards_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import amp_rewards  # noqa: E402


class TorchArm:
    """the stage in torch ops; reward_min / reward_max are host floats, as in a learner that hands them to heads.Critic"""

    def __init__(self, scale, lerp, discount):
        self.scale, self.lerp, self.discount = scale, lerp, discount
        self.reward_min, self.reward_max = float("inf"), float("-inf")
        self.mean = self.std = None

    def update(self, logits, task, done, valid, values):
        T = logits.shape[0]
        mask = torch.empty_like(done)
        inv = torch.zeros_like(done[0], dtype=torch.bool)
        for t in range(T - 1, -1, -1):
            inv = torch.where(done[t] != 0, valid[t] == 0, inv)
            mask[t] = (~inv).int()
        d = 1.0 - logits
        s = torch.clamp_min(1.0 - 0.25 * d * d, 0.0) * self.scale
        r = (1.0 - self.lerp) * s + self.lerp * task
        counted = mask != 0
        sc = s[counted].double()
        self.mean, self.std = sc.mean(), sc.std(unbiased=False)
        inf = torch.tensor(float("inf"), device=r.device)
        self.reward_min = min(self.reward_min, torch.where(counted, r, inf).min().item())          # (a host read each: the bounds become the critic's lo / hi)
        self.reward_max = max(self.reward_max, torch.where(counted, r, -inf).max().item())
        lo, hi = self.reward_min / (1.0 - self.discount), self.reward_max / (1.0 - self.discount)
        return r, mask, torch.clamp(values, lo, hi)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32); ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amp_rewards_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amp_rewards_bench needs a GPU (deepmimic_amd has no CPU path)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    T, N, scale, lerp, discount = a.T, a.N, 2.0, 0.3, 0.95
    logits = 1.0 + 1.6 * torch.randn((T, N), generator=g, device=dev)
    task = torch.rand((T, N), generator=g, device=dev)
    done = (torch.rand((T, N), generator=g, device=dev) < 1.0 / 30).int()          # episodes of about a second
    valid = (torch.rand((T, N), generator=g, device=dev) >= 0.01).int()
    values = 40.0 * torch.randn((T + 1, N), generator=g, device=dev)
    trk = amp_rewards.AmpRewards(dev, reward_scale=scale, task_reward_lerp=lerp, discount=discount)
    arm = TorchArm(scale, lerp, discount)

    def device_arm():
        r, m = trk.update_torch(logits, task, done, valid)
        return r, m, trk.clip_torch(values)
    kd, td = device_arm(), arm.update(logits, task, done, valid, values)
    st = trk.state_host()
    agree = dict(mask_equal=bool((kd[1] == td[1]).all()), rewards_max_abs_diff=float((kd[0] - td[0]).abs().max()), clipped_max_abs_diff=float((kd[2] - td[2]).abs().max()),
                 bounds_equal=bool(st["reward_min"] == arm.reward_min and st["reward_max"] == arm.reward_max),
                 mean_rel_diff=float(abs(st["disc_reward_mean"] - arm.mean.item()) / abs(st["disc_reward_mean"])),
                 std_rel_diff=float(abs(st["disc_reward_std"] - arm.std.item()) / abs(st["disc_reward_std"])), n=st["n"],
                 clipped_share=float(((kd[2] == st["val_min"]) | (kd[2] == st["val_max"])).float().mean()))
    runs = dict(device=device_arm, torch_ops=lambda: arm.update(logits, task, done, valid, values))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    out = dict(what="AMP batch rewards: AmpRewards.update_torch + clip_torch of [T + 1, N] values (five launches, no host read) vs the same result in public torch "
                    "ops with the two .item() reads of the running bounds (microseconds per call, HIP events around whole calls, arms alternating; every time includes "
                    "the allocation of the outputs and the Python / ctypes launch path)",
               device=torch.cuda.get_device_name(0), T=T, N=N, reps=a.reps, warmup=a.warmup, bytes_in=T * N * 16 + (T + 1) * N * 4, bytes_out=T * N * 8 + (T + 1) * N * 4,
               us_q25_median_q75={k: quartiles(v) for k, v in times.items()}, host_reads_per_call=dict(device=0, torch_ops=2), agreement=agree,
               us_every_repetition=times)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("us_every_repetition", "what")}))


if __name__ == "__main__":
    main()
