"""Times of the task-push launches (k_push_where / k_push_state of deepmimic_amd/csrc/dm_device.h, deepmimic_amd/pushes.py), one process, the arms alternating, whole
calls bracketed by HIP events on the current stream, every repetition kept.  A report, no gate.  Per scene (4096 humanoid3d_walk and 4096 dog3d_pace by default):
  (a) launches  dm_push_where with a mask of 1 % and of 100 % of the envs (world and heading frame) and dm_push_state, microseconds per call (the ctypes launch path
                included); the pushed rows are cleared again outside the bracket, so that every repetition finds free slots
  (b) step      TorchVecEnv.step, one fixed action tensor, env-steps per second in two configurations stepped in alternating blocks: `rows` -- enable_rand_perturbs
                with an interval of 1e9 s, i.e. the AMP kernel family with perturbation rows and nothing else -- and `pushes` -- pushes=True, which adds the
                dm_push_state launch behind every step; nobody is pushed in either arm, so the difference is the feature's standing cost
Writes one JSON object (default profiles/push_bench.json).
usage: python tools/push_bench.py [--N 4096] [--reps 100] [--warmup 10] [--steps 100] [--blocks 6] [--scenes humanoid3d_walk dog3d_pace] [--out ...]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import model, pushes as pu  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench_launches(scene, N, reps, warmup):
    env = TorchVecEnv(model.load_asset(scene), N, seed=1, pushes=True)
    env.reset(); env._enter()
    dev, J = env.device, env.env.J
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    few = torch.zeros(N, **i32); few[::100] = 1                                          # 1 % of the envs
    every = torch.ones(N, **i32)
    g = torch.Generator(device=dev); g.manual_seed(2)
    links = torch.randint(0, J, (N,), generator=g, device=dev, dtype=torch.int32)
    forces = 100.0 * torch.randn((N, 3), generator=g, **f64)
    durs = torch.full((N,), 0.2, **f64)
    bad = torch.zeros(1, **i32)
    push = lambda mask, flags: pu.push_where_device(env.env, mask.data_ptr(), links.data_ptr(), forces.data_ptr(), durs.data_ptr(), 0, flags, bad.data_ptr())
    runs = dict(push_where_1pct=lambda: push(few, pu.WORLD), push_where_1pct_heading=lambda: push(few, pu.HEADING), push_where_100pct=lambda: push(every, pu.WORLD),
                push_where_100pct_heading=lambda: push(every, pu.HEADING), push_state=lambda: pu.push_state_device(env.env, env.pushes.data_ptr()))
    # bytes from the shapes: a push reads mask, link, force, duration and the row's two slots and writes one slot; push_state reads two slots and writes 12 floats
    per_push = 6 * 8
    moved = dict(push_where_1pct=int(few.sum()) * per_push, push_where_1pct_heading=int(few.sum()) * per_push, push_where_100pct=N * per_push,
                 push_where_100pct_heading=N * per_push, push_state=N * 12 * 4)
    for _ in range(warmup):
        for fn in runs.values():
            fn()
        env.clear_pushes()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
            env.clear_pushes()
    assert int(bad.item()) == 0
    env.close()
    return dict(scene=scene, N=N, J=J, bytes_written=moved, us_q25_median_q75={k: quartiles(v) for k, v in times.items()}, us_every_repetition=times)


def bench_step(scene, N, steps, blocks, warmup_steps):
    rows = model.load_asset(scene)
    rows.cfg.enable_rand_perturbs = True; rows.cfg.perturb_time_min = rows.cfg.perturb_time_max = 1e9
    envs = {"rows": TorchVecEnv(rows, N, seed=1), "pushes": TorchVecEnv(model.load_asset(scene), N, seed=1, pushes=True)}
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    acts = 0.3 * torch.randn((N, envs["rows"].act_dim), generator=g, dtype=torch.float32, device="cuda")

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
    base = np.array(rates["rows"])
    return dict(scene=scene, N=N, steps_per_block=steps, blocks=blocks, env_steps_per_s_q25_median_q75={k: quartiles(v) for k, v in rates.items()},
                pushes_over_rows=med["pushes"] / med["rows"], rows_spread_rel=float((base.max() - base.min()) / med["rows"]), env_steps_per_s_every_block=rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096); ap.add_argument("--reps", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--blocks", type=int, default=6); ap.add_argument("--step-warmup", type=int, default=30)
    ap.add_argument("--scenes", nargs="+", default=["humanoid3d_walk", "dog3d_pace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("push_bench needs a GPU (deepmimic_amd has no CPU path)")
    out = dict(what="task-chosen pushes: microseconds per dm_push_where / dm_push_state call (HIP events, alternating, the ctypes launch path included) beside the bytes "
                    "each launch writes (from the shapes), and TorchVecEnv env-steps/s with pushes=True against enable_rand_perturbs with an interval of 1e9 s "
                    "(alternating blocks); a report, no gate",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               launches=[bench_launches(s, a.N, a.reps, a.warmup) for s in a.scenes],
               step=[bench_step(s, a.N, a.steps, a.blocks, a.step_warmup) for s in a.scenes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    for u in out["launches"]:
        print("launches %s N=%d us q25/median/q75:" % (u["scene"], u["N"]), u["us_q25_median_q75"])
    for w in out["step"]:
        print("step %s env-steps/s q25/median/q75:" % w["scene"], w["env_steps_per_s_q25_median_q75"], "pushes over rows: %.4f" % w["pushes_over_rows"],
              "rows spread = %.4f" % w["rows_spread_rel"])


if __name__ == "__main__":
    main()
