"""Times of the episode statistics stage (deepmimic_amd/csrc/dm_episode.h, deepmimic_amd/episodes.py), one process, the arms interleaved, whole calls bracketed by HIP
events on the current stream, every repetition kept:
  (a) update   EpisodeStats.update (two launches, no host read) at (T, N) = (1, 4096) and (32, 4096)   vs   TorchStats.update below: the same stage -- carry, per-step
               rows, per-class counts / steps / longest / return sum, squares, min, max -- in public torch ops on the same tensors, no host read either.  That
               baseline is the yardstick: what a learner writes without the kernel.
  (b) walk     TorchVecEnv, humanoid3d_walk, 4096 envs, one fixed action tensor, env-steps per second with episode_stats on against off (two contexts of one
               seed, stepped in alternating blocks).
Writes one JSON object (default profiles/episode_stats_bench.json).
usage: python tools/episode_stats_bench.py [--N 4096] [--reps 200] [--warmup 20] [--walk-steps 100] [--walk-reps 10] [--out profiles/episode_stats_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import episodes, model  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


class TorchStats:
    """the stage of dm_episode_stats in torch ops: fp64 carry, one-hot class masks [4, N], reductions along the env axis; nothing is read back"""

    def __init__(self, n, dev):
        f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
        self.acc, self.len = torch.zeros(n, **f64), torch.zeros(n, dtype=torch.int32, device=dev)
        self.episodes, self.steps, self.len_max = torch.zeros(4, **i64), torch.zeros(4, **i64), torch.zeros(4, **i64)
        self.sum, self.sq = torch.zeros(3, **f64), torch.zeros(3, **f64)
        self.min, self.max = torch.full((3,), float("inf"), **f64), torch.full((3,), float("-inf"), **f64)
        self.classes = torch.arange(4, device=dev).unsqueeze(1)
        self.inf = torch.tensor(float("inf"), **f64)
        self.zero_acc, self.zero_len = torch.zeros_like(self.acc), torch.zeros_like(self.len)

    def update(self, rewards, terminate, done, valid):
        T = rewards.shape[0]
        ep_return, ep_len = torch.empty_like(rewards), torch.empty_like(terminate)
        for t in range(T):
            self.acc += rewards[t].double(); self.len += 1
            ep_return[t] = self.acc.float(); ep_len[t] = self.len
            d = done[t] != 0
            cls = torch.where((valid[t] == 0) | ~torch.isfinite(self.acc), 3, torch.where((terminate[t] == 1) | (terminate[t] == 2), terminate[t], 0))
            hot = (cls.unsqueeze(0) == self.classes) & d                   # [4, N]
            lens = hot * self.len.long()
            self.episodes += hot.sum(1); self.steps += lens.sum(1); self.len_max = torch.maximum(self.len_max, lens.amax(1))
            ret = torch.where(hot[:3], self.acc, 0.0)
            self.sum += ret.sum(1); self.sq += (ret * ret).sum(1)
            self.min = torch.minimum(self.min, torch.where(hot[:3], self.acc, self.inf).amin(1))
            self.max = torch.maximum(self.max, torch.where(hot[:3], self.acc, -self.inf).amax(1))
            self.acc = torch.where(d, self.zero_acc, self.acc); self.len = torch.where(d, self.zero_len, self.len)
        return ep_return, ep_len


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench_update(T, N, reps, warmup, g):
    dev = torch.device("cuda:0")
    rewards = torch.rand((T, N), generator=g, dtype=torch.float32, device=dev)
    terminate = torch.randint(0, 3, (T, N), generator=g, device=dev).int()
    done = (torch.rand((T, N), generator=g, device=dev) < 1.0 / 30).int()          # episodes of about a second
    valid = (torch.rand((T, N), generator=g, device=dev) >= 0.01).int()
    ks, ts = episodes.EpisodeStats(N, dev), TorchStats(N, dev)
    k_out, t_out = ks.update(rewards, terminate, done, valid), ts.update(rewards, terminate, done, valid)
    kb = ks.raw(); kf = kb.view(np.float64)
    agree = dict(rows_equal=bool((k_out[0] == t_out[0]).all() and (k_out[1] == t_out[1]).all()),
                 counts_equal=bool((kb[0:4] == ts.episodes.cpu().numpy()).all() and (kb[4:8] == ts.steps.cpu().numpy()).all() and (kb[8:12] == ts.len_max.cpu().numpy()).all()),
                 ret_sum_max_rel_diff=float(np.max(np.abs(kf[12:15] - ts.sum.cpu().numpy()) / np.maximum(np.abs(kf[12:15]), 1e-300))),
                 ret_min_max_equal=bool((kf[18:21] == ts.min.cpu().numpy()).all() and (kf[21:24] == ts.max.cpu().numpy()).all()))
    runs = dict(kernels=lambda: ks.update(rewards, terminate, done, valid), torch_ops=lambda: ts.update(rewards, terminate, done, valid))
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(T=T, N=N, bytes_in=T * N * 16, bytes_out=T * N * 8, us_q25_median_q75={k: quartiles(v) for k, v in times.items()},
                torch_over_kernels=med["torch_ops"] / med["kernels"], agreement=agree, us_every_repetition=times)


def bench_walk(N, steps, reps, warmup_steps):
    t = model.load_asset("humanoid3d_walk")
    envs = {"off": TorchVecEnv(t, N, seed=1), "on": TorchVecEnv(t, N, seed=1, episode_stats=True)}
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    acts = 0.3 * torch.randn((N, envs["off"].act_dim), generator=g, dtype=torch.float32, device="cuda")

    def block(env, n):
        for _ in range(n):
            env.step(acts)
    for env in envs.values():
        env.reset(); block(env, warmup_steps)
    torch.cuda.synchronize()
    rates = {k: [] for k in envs}
    for _ in range(reps):
        for k, env in envs.items():
            us = timed(lambda: block(env, steps))
            rates[k].append(N * steps / (us * 1e-6))
    tot = envs["on"].episode_totals()
    for env in envs.values():
        env.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    off = np.array(rates["off"])
    return dict(N=N, steps_per_block=steps, blocks=reps, env_steps_per_s_q25_median_q75={k: quartiles(v) for k, v in rates.items()},
                on_over_off=med["on"] / med["off"], off_spread_rel=float((off.max() - off.min()) / med["off"]),
                episodes_seen=dict(episodes=tot["episodes"], fall_share=tot["fall_share"], invalid=tot["invalid"]["episodes"], mean_length=tot["mean_length"],
                                   mean_return=tot["mean_return"]),
                env_steps_per_s_every_block=rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096); ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--walk-steps", type=int, default=100); ap.add_argument("--walk-reps", type=int, default=10); ap.add_argument("--walk-warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_stats_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_stats_bench needs a GPU (deepmimic_amd has no CPU path)")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    out = dict(what="episode statistics: EpisodeStats.update vs the same stage in public torch ops (microseconds per call, HIP events, interleaved; every time includes "
                    "the allocation of the per-step rows and the Python / ctypes launch path), and TorchVecEnv env-steps/s with episode_stats on vs off",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               update=[bench_update(T, a.N, a.reps, a.warmup, g) for T in (1, 32)],
               walk=bench_walk(a.N, a.walk_steps, a.walk_reps, a.walk_warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    for u in out["update"]:
        print("update T=%d N=%d us q25/median/q75:" % (u["T"], u["N"]), u["us_q25_median_q75"], "torch/kernels = %.2f" % u["torch_over_kernels"], u["agreement"])
    w = out["walk"]
    print("walk env-steps/s q25/median/q75:", w["env_steps_per_s_q25_median_q75"], "on/off = %.4f" % w["on_over_off"], "off spread = %.4f" % w["off_spread_rel"], w["episodes_seen"])


if __name__ == "__main__":
    main()
