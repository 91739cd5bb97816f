"""Times of the link-state and masked-reset launches (k_link_state / k_env_reset_where of deepmimic_amd/csrc/dm_device.h, deepmimic_amd/link_state.py), one process,
the arms alternating, whole calls bracketed by HIP events on the current stream, every repetition kept.  A report, no gate.  Per scene (4096 humanoid3d_walk and
4096 dog3d_pace by default):
  (a) launches  dm_link_state alone (the simulated character, every output; the kinematic character) and dm_reset_where alone with a mask of 1 % and of 100 % of the
                envs, microseconds per call (the ctypes launch path included), next to the bytes each launch writes, computed from the shapes
  (b) step      TorchVecEnv.step, one fixed action tensor, env-steps per second in four configurations stepped in alternating blocks: default, link_state,
                link_state + kin_link_state, link_state + deferred_reset
Writes one JSON object (default profiles/link_state_bench.json).
usage: python tools/link_state_bench.py [--N 4096] [--reps 100] [--warmup 10] [--steps 100] [--blocks 6] [--scenes humanoid3d_walk dog3d_pace] [--out ...]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import link_state as ls, model  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench_launches(scene, N, reps, warmup):
    env = TorchVecEnv(model.load_asset(scene), N, seed=1, link_state=True, kin_link_state=True)
    env.reset(); env._enter()
    J, lw, ew, P, ow = ls.dims(env.env)
    S, G = env.obs_dim, env.goal_dim
    dev = env.device
    few = torch.zeros(N, dtype=torch.int32, device=dev); few[::100] = 1               # 1 % of the envs
    every = torch.ones(N, dtype=torch.int32, device=dev)
    runs = dict(link_state_sim=lambda: env.ls.update(), link_state_kin=lambda: env.kin_ls.update(),
                reset_where_1pct=lambda: ls.reset_where_device(env.env, few.data_ptr(), env.obs.data_ptr(), env.goal.data_ptr() if G else 0),
                reset_where_100pct=lambda: ls.reset_where_device(env.env, every.data_ptr(), env.obs.data_ptr(), env.goal.data_ptr() if G else 0))
    link_bytes = 4 * N * (J * lw + ew + 2 * P)
    # a reset writes the env record (pose, vel, PD targets: 3 P; torques D; kin row 8 elements; clocks 6 doubles; flags 4 ints) and one observation row
    elem = 8 if env.env.precision == 64 else 4
    per_reset = elem * (3 * P + env.env.D + 8) + 6 * 8 + 4 * 4 + 4 * (S + G)
    written = dict(link_state_sim=link_bytes + 4 * N * ow, link_state_kin=link_bytes, reset_where_1pct=int(few.sum()) * per_reset, reset_where_100pct=N * per_reset)
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    env.close()
    return dict(scene=scene, N=N, J=J, P=P, S=S, bytes_written=written, us_q25_median_q75={k: quartiles(v) for k, v in times.items()}, us_every_repetition=times)


def bench_step(scene, N, steps, blocks, warmup_steps):
    t = model.load_asset(scene)
    configs = {"default": {}, "link_state": dict(link_state=True), "link_state+kin": dict(link_state=True, kin_link_state=True),
               "link_state+deferred_reset": dict(link_state=True, deferred_reset=True)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_state_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("link_state_bench needs a GPU (deepmimic_amd has no CPU path)")
    out = dict(what="link states and the masked reset: microseconds per dm_link_state / dm_reset_where call (HIP events, alternating, the ctypes launch path included) "
                    "beside the bytes each launch writes (from the shapes), and TorchVecEnv env-steps/s in four configurations (alternating blocks); a report, no gate",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               launches=[bench_launches(s, a.N, a.reps, a.warmup) for s in a.scenes],
               step=[bench_step(s, a.N, a.steps, a.blocks, a.step_warmup) for s in a.scenes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    for u in out["launches"]:
        print("launches %s N=%d us q25/median/q75:" % (u["scene"], u["N"]), u["us_q25_median_q75"], "bytes written:", u["bytes_written"])
    for w in out["step"]:
        print("step %s env-steps/s q25/median/q75:" % w["scene"], w["env_steps_per_s_q25_median_q75"], "over default:", w["over_default"], "default spread = %.4f" % w["default_spread_rel"])


if __name__ == "__main__":
    main()
