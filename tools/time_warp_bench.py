"""Times of the batched time-warp return (deepmimic_amd/csrc/dm_time_warp.h, deepmimic_amd/time_warp.py), one process, the arms interleaved, whole calls bracketed by
HIP events on the current stream, every repetition kept:
  (a) align    dm_time_warp_align at N = 4096 envs of a 20 s test episode (capacity 602, 3J = 45, fp32): every env with n = 601 samples, and n drawn ragged (uniform
               in [2, 601]: falls end episodes early).  Beside it `model.time_warp_cost` on the host for a handful of envs -- the only route to this number before
               the kernel, so the ratio is against what the project could do, not against another kernel -- and the two routes' agreement on those envs.
  (b) walk     TorchVecEnv, humanoid3d_walk as `--scene imitate_amp` with 20 s episodes, 4096 envs, one fixed action tensor, env-steps per second with time_warp on
               against off (two contexts of one seed, stepped in alternating blocks).
Writes one JSON object (default profiles/time_warp_bench.json).
usage: python tools/time_warp_bench.py [--N 4096] [--reps 10] [--warmup 2] [--host-envs 3] [--walk-steps 100] [--walk-reps 10] [--out profiles/time_warp_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import model, time_warp  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench_align(N, capacity, dim, reps, warmup, host_envs, g):
    dev = torch.device("cuda:0")
    # a random walk per env and coordinate, and the same walk with a slower second walk on top for the kinematic side: distances grow along the episode as they do
    # when a character drifts off its clip.  (The kernel's work does not depend on the values.)
    samples = torch.empty((N, 2, capacity, dim), dtype=torch.float32, device=dev)
    samples[:, 0] = torch.cumsum(0.02 * torch.randn((N, capacity, dim), generator=g, device=dev), dim=1)
    samples[:, 1] = samples[:, 0] + torch.cumsum(0.005 * torch.randn((N, capacity, dim), generator=g, device=dev), dim=1)
    n_full = capacity - 1
    counts = dict(full=torch.full((N,), n_full, dtype=torch.int32, device=dev),
                  ragged=torch.randint(2, n_full + 1, (N,), generator=g, device=dev).int())
    reward, cost = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(count):
        time_warp.align_device(N, capacity, dim, False, samples.data_ptr(), count.data_ptr(), 0, reward.data_ptr(), cost.data_ptr(), stream=stream)
    runs = {k: (lambda c=c: run(c)) for k, c in counts.items()}
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    # the host route on a handful of envs of the full arm, and what the two routes make of them
    run(counts["full"]); torch.cuda.synchronize()
    dev_cost = cost[:host_envs].cpu().numpy()
    host_s, host_cost = [], []
    for e in range(host_envs):
        s = samples[e, :, :n_full].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter(); host_cost.append(model.time_warp_cost(s[0], s[1])); host_s.append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    cells = {k: int(((c.long() - 1) ** 2).sum().item()) for k, c in counts.items()}
    return dict(N=N, capacity=capacity, dim=dim, n_full=n_full, ragged_mean_n=float(counts["ragged"].float().mean().item()), cells=cells,
                sample_bytes=N * 2 * capacity * dim * 4, us_q25_median_q75={k: quartiles(v) for k, v in times.items()},
                cells_per_s={k: cells[k] / (med[k] * 1e-6) for k in med},
                host_seconds_per_env=host_s, host_envs=host_envs,
                host_time_for_N_over_device_time=float(np.median(host_s)) * N / (med["full"] * 1e-6),
                agreement_max_rel_diff=float(np.max(np.abs(dev_cost - np.array(host_cost)) / np.maximum(np.array(host_cost), 1e-300))),
                us_every_repetition=times)


def bench_walk(N, steps, reps, warmup_steps):
    t = model.load_asset("humanoid3d_walk")
    t.cfg.scene = "imitate_amp"
    t.cfg.time_lim_min = t.cfg.time_lim_max = t.cfg.time_end_lim_min = t.cfg.time_end_lim_max = 20.0
    envs = {"off": TorchVecEnv(t, N, seed=1, test_mode=True), "on": TorchVecEnv(t, N, seed=1, test_mode=True, time_warp=True, episode_stats=True)}
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
    envs["on"].tw.check_overflow()
    tot = envs["on"].episode_totals()
    cap = envs["on"].tw.capacity
    for env in envs.values():
        env.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    off = np.array(rates["off"])
    return dict(N=N, capacity=cap, steps_per_block=steps, blocks=reps, env_steps_per_s_q25_median_q75={k: quartiles(v) for k, v in rates.items()},
                on_over_off=med["on"] / med["off"], off_spread_rel=float((off.max() - off.min()) / med["off"]),
                episodes_seen=dict(episodes=tot["episodes"], fall_share=tot["fall_share"], mean_length=tot["mean_length"], mean_time_warp_return=tot["mean_return"]),
                env_steps_per_s_every_block=rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=602); ap.add_argument("--dim", type=int, default=45); ap.add_argument("--host-envs", type=int, default=3)
    ap.add_argument("--walk-steps", type=int, default=100); ap.add_argument("--walk-reps", type=int, default=10); ap.add_argument("--walk-warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_warp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_warp_bench needs a GPU (deepmimic_amd has no CPU path)")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    out = dict(what="time-warp return: dm_time_warp_align (microseconds per call, HIP events, arms interleaved; every time includes the Python / ctypes launch path) "
                    "beside model.time_warp_cost on the host, and TorchVecEnv env-steps/s with time_warp on vs off",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               align=bench_align(a.N, a.capacity, a.dim, a.reps, a.warmup, a.host_envs, g),
               walk=bench_walk(a.N, a.walk_steps, a.walk_reps, a.walk_warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    al, w = out["align"], out["walk"]
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    print("align N=%d n=%d us q25/median/q75:" % (al["N"], al["n_full"]), al["us_q25_median_q75"], "cells/s", al["cells_per_s"],
          "host s/env", al["host_seconds_per_env"], "host(N)/device = %.0f" % al["host_time_for_N_over_device_time"], "max rel diff %.2e" % al["agreement_max_rel_diff"])
    print("walk env-steps/s q25/median/q75:", w["env_steps_per_s_q25_median_q75"], "on/off = %.4f" % w["on_over_off"], "off spread = %.4f" % w["off_spread_rel"], w["episodes_seen"])


if __name__ == "__main__":
    main()
