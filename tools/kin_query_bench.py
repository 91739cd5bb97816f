"""Times of the kinematic-query and start-at launches (k_kin_query / k_env_reset_where_at of deepmimic_amd/csrc/dm_device.h, deepmimic_amd/kin_query.py), in the manner
of tools/link_state_bench.py: one process, the arms alternating, whole calls bracketed by HIP events on the current stream, every repetition kept.  Per scene (4096
humanoid3d_walk and 4096 dog3d_pace by default):
  (a) launches  dm_kin_query with K = 1, 4 and 8 (every output) beside FOUR dm_link_state(which = 1) calls in one bracket -- the yardstick: one K = 4 query loads the
                env record and the model tables once where four link-state launches load them four times, so it must take less (`gate_k4_below_4x_link_state`,
                on the medians) --, and dm_reset_where_at (a clip time given for every selected env) beside dm_reset_where, with a mask of 1 % and of 100 % of the
                envs.  Microseconds per bracket, the ctypes launch path included, next to the bytes each launch writes, computed from the shapes.
  (b) step      TorchVecEnv.step, one fixed action tensor, env-steps per second, default against kin_lookahead of K = 4, in alternating blocks.  A report.
Writes one JSON object (default profiles/kin_query_bench.json); the exit status is 1 if the gate of (a) fails for a scene.
usage: python tools/kin_query_bench.py [--N 4096] [--reps 100] [--warmup 10] [--steps 100] [--blocks 6] [--scenes humanoid3d_walk dog3d_pace] [--out ...]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import kin_query as kq, link_state as ls, model  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402

KS = (1, 4, 8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench_launches(scene, N, reps, warmup):
    env = TorchVecEnv(model.load_asset(scene), N, seed=1, kin_link_state=True)
    env.reset(); env._enter()
    J, lw, ew, P, _ = ls.dims(env.env)
    S, G = env.obs_dim, env.goal_dim
    dev = env.device
    queries = {K: kq.KinQuery(env.env, K, device=dev) for K in KS}
    offsets = {K: torch.arange(1, K + 1, dtype=torch.float64, device=dev) / 30.0 for K in KS}        # the next K control steps
    few = torch.zeros(N, dtype=torch.int32, device=dev); few[::100] = 1               # 1 % of the envs
    every = torch.ones(N, dtype=torch.int32, device=dev)
    start = torch.full((N,), 0.25, dtype=torch.float64, device=dev)                   # a clip time for every env
    goal_ptr = env.goal.data_ptr() if G else 0

    def four_link_states():
        for _ in range(4):
            env.kin_ls.update()
    runs = {"link_state_kin_x4": four_link_states, "link_state_kin": lambda: env.kin_ls.update()}
    for K in KS:
        runs["kin_query_K%d" % K] = lambda K=K: queries[K].update(offsets[K])
    for name, mask in (("1pct", few), ("100pct", every)):
        runs["reset_where_" + name] = lambda mask=mask: ls.reset_where_device(env.env, mask.data_ptr(), env.obs.data_ptr(), goal_ptr)
        runs["reset_where_at_" + name] = lambda mask=mask: kq.reset_where_at_device(env.env, mask.data_ptr(), 0, start.data_ptr(), 0, env.obs.data_ptr(), goal_ptr, 0)
    frame_bytes = 4 * N * (J * lw + ew + 2 * P)
    elem = 8 if env.env.precision == 64 else 4
    per_reset = elem * (3 * P + env.env.D + 8) + 6 * 8 + 4 * 4 + 4 * (S + G)          # (tools/link_state_bench.py)
    written = {"link_state_kin_x4": 4 * frame_bytes, "link_state_kin": frame_bytes}
    written.update({"kin_query_K%d" % K: K * frame_bytes for K in KS})
    for name, mask in (("1pct", few), ("100pct", every)):
        written["reset_where_" + name] = written["reset_where_at_" + name] = int(mask.sum()) * per_reset
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    env.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(scene=scene, N=N, J=J, P=P, S=S, bytes_written=written, us_q25_median_q75={k: quartiles(v) for k, v in times.items()},
                k4_over_4x_link_state=med["kin_query_K4"] / med["link_state_kin_x4"], gate_k4_below_4x_link_state=bool(med["kin_query_K4"] < med["link_state_kin_x4"]),
                us_per_frame={"kin_query_K%d" % K: med["kin_query_K%d" % K] / K for K in KS}, us_every_repetition=times)


def bench_step(scene, N, steps, blocks, warmup_steps):
    t = model.load_asset(scene)
    configs = {"default": {}, "kin_lookahead_K4": dict(kin_lookahead=(1 / 30, 2 / 30, 3 / 30, 4 / 30))}
    envs = {k: TorchVecEnv(t, N, seed=1, **kw) for k, kw in configs.items()}
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    acts = 0.3 * torch.randn((N, envs["default"].act_dim), generator=g, dtype=torch.float32, device="cuda")

    def block(env, n):
        for _ in range(n):
            env.step(acts)
    for env in envs.values():
        env.reset(); block(env, warmup_steps)
    torch.cuda.synchronize()
    rates = {k: [] for k in envs}
    for _ in range(blocks):
        for k, env in envs.items():
            us = timed(lambda: block(env, steps))
            rates[k].append(N * steps / (us * 1e-6))
    for env in envs.values():
        env.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    base = np.array(rates["default"])
    return dict(scene=scene, N=N, steps_per_block=steps, blocks=blocks, env_steps_per_s_q25_median_q75={k: quartiles(v) for k, v in rates.items()},
                over_default={k: med[k] / med["default"] for k in med}, default_spread_rel=float((base.max() - base.min()) / med["default"]),
                env_steps_per_s_every_block=rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096); ap.add_argument("--reps", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--blocks", type=int, default=6); ap.add_argument("--step-warmup", type=int, default=30)
    ap.add_argument("--scenes", nargs="+", default=["humanoid3d_walk", "dog3d_pace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kin_query_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kin_query_bench needs a GPU (deepmimic_amd has no CPU path)")
    out = dict(what="the kinematic query and the reset at a given start: microseconds per dm_kin_query (K = 1, 4, 8) / dm_reset_where_at call beside four dm_link_state(1) "
                    "calls / dm_reset_where (HIP events, alternating, the ctypes launch path included), the bytes each launch writes (from the shapes), and TorchVecEnv "
                    "env-steps/s with kin_lookahead of K = 4 against the default (alternating blocks).  Gate: one K = 4 query below four link-state calls, on the medians",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               launches=[bench_launches(s, a.N, a.reps, a.warmup) for s in a.scenes],
               step=[bench_step(s, a.N, a.steps, a.blocks, a.step_warmup) for s in a.scenes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    for u in out["launches"]:
        print("launches %s N=%d us q25/median/q75:" % (u["scene"], u["N"]), u["us_q25_median_q75"], "K4 / 4 x link_state = %.3f" % u["k4_over_4x_link_state"])
    for w in out["step"]:
        print("step %s env-steps/s q25/median/q75:" % w["scene"], w["env_steps_per_s_q25_median_q75"], "over default:", w["over_default"], "default spread = %.4f" % w["default_spread_rel"])
    return 0 if all(u["gate_k4_below_4x_link_state"] for u in out["launches"]) else 1


if __name__ == "__main__":
    sys.exit(main())
