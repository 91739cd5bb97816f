"""A PPO run on humanoid3d_walk with the reference's agent file values (data/agents/ct_agent_humanoid_ppo.txt) at 4096 envs, for a wall-clock budget: Train_Return,
Samples and wall time of every iteration, and whether the return rose over its value at iteration 0 of the same run.  Nothing is tuned here: a flat curve is a
finding.  Train_Return is the mean return of the episodes that finished in the iteration's rollout.  The packaged humanoid3d_walk scene has no episode timer
(it is the reference's run scene): an episode ends when the character falls, so the return is the reward collected until the fall and has no upper bound.

Writes one JSON object (default profiles/agent_learning_walk.json).
usage: python tools/agent_learning_run.py [--minutes 2] [--envs 4096] [--T 32] [--mini_batch_size 256] [--out profiles/agent_learning_walk.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import agent, model  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402
from agent_iteration_bench import PPO  # noqa: E402


COLUMNS = ("Samples", "Train_Return", "wall_s")


def write(out: dict, path: str):
    """the run's figures, then one line per column of the per-iteration record (row i: iteration i), five significant digits"""
    rows = out.pop("rows")
    cols = {k: [r[k] if isinstance(r[k], int) else float("%.5g" % r[k]) for r in rows] for k in COLUMNS}
    with open(path, "w") as f:
        f.write(json.dumps(out)[:-1] + ',\n "per_iteration": {\n' + ",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cols.items()) + "\n }}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=2.0); ap.add_argument("--envs", type=int, default=4096); ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--mini_batch_size", type=int, default=256); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agent_learning_walk.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agent_learning_run needs the GPU: no HIP device is visible")
    if a.minutes > 10:
        raise SystemExit("--minutes: at most ten")
    cfg = agent.AgentConfig.from_dict(PPO)
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), a.envs, seed=a.seed)
    ag = agent.make_agent(env, cfg, rollout_steps=a.T, seed=a.seed, mini_batch_size=a.mini_batch_size)
    rows, t0 = [], time.time()
    while time.time() - t0 < 60.0 * a.minutes:
        r = ag.iterate()
        rows.append({k: r[k] for k in ("Samples", "Train_Return")})
        rows[-1]["wall_s"] = time.time() - t0
        if len(rows) % 20 == 1:
            print("iteration %4d  samples %9d  Train_Return %8.4f  %6.1f s" % (r["Iteration"], r["Samples"], r["Train_Return"], rows[-1]["wall_s"]), flush=True)
    ret = np.array([r["Train_Return"] for r in rows])
    tenth = max(1, len(rows) // 10)
    first, last = float(ret[0]), float(ret[-tenth:].mean())
    out = dict(tool="tools/agent_learning_run.py", device=torch.cuda.get_device_name(0), asset="humanoid3d_walk", agent_file_values="data/agents/ct_agent_humanoid_ppo.txt", envs=a.envs, T=a.T,
               mini_batch_size=a.mini_batch_size, seed=a.seed, iterations=len(rows), samples=rows[-1]["Samples"], wall_s=rows[-1]["wall_s"],
               train_return_iteration_0=first, train_return_first_tenth_mean=float(ret[:tenth].mean()), train_return_last_tenth_mean=last,
               train_return_max=float(ret.max()), return_rose_over_iteration_0=bool(last > first), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write(out, a.out)
    print("iterations %d, samples %d: Train_Return %.4f at iteration 0, %.4f over the last tenth -> rose: %s" % (len(rows), out["samples"], first, last,
                                                                                                            out["return_rose_over_iteration_0"]))
    env.close()


if __name__ == "__main__":
    main()
