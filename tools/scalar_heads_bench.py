#!/usr/bin/env python
"""Scalar heads against what the library offered before them, interleaved in ONE process, HIP-event times.

Arms, at the humanoid critic (S = 197, and gated 197 + 3) and discriminator (226) widths, at 4096 and 32 x 4096 rows:
  scalar   one dm_policy_eval_scalar call (deepmimic_amd/heads.py): net + clip / terminate override, or net + style reward
  actor1   a Policy with A = 1 asked for its mode action, plus the torch ops that finish the value (clamp, two torch.where) or the reward
and for the critic on terminal observations: the scalar call with row_mask at the done rate of a random actor against the same call without a mask.
Every repetition goes to profiles/scalar_heads_bench.json.  Usage: python tools/scalar_heads_bench.py [--reps 30] [--out profiles/scalar_heads_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--done-rate", type=float, default=0.02, help="fraction of rows with done set (a random actor's humanoid falls every ~50 steps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_heads_bench.json"))
    a = ap.parse_args()
    import torch
    from deepmimic_amd.heads import Critic, Discriminator
    from deepmimic_amd.policy import Policy, random_weights
    torch.zeros(1, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3          # microseconds

    results = []
    for name, S, G, kind in (("critic", 197, 0, "value"), ("gated_critic", 200, 3, "value"), ("discriminator", 226, 0, "style")):
        w = random_weights(S, 1, seed=3, init_output_scale=0.5, gated_goal_dim=G)
        for k in ("a_mean", "a_std"):
            w.pop(k, None)
        head = Critic(w, lo=-1.0, hi=1.0, val_fail=0.0, val_succ=20.0) if kind == "value" else \
            Discriminator({k: v for k, v in w.items() if k != "logstd"}, reward_scale=2.0, task_reward_lerp=0.5)
        actor = Policy(w)
        for n in (4096, 32 * 4096):
            gen = torch.Generator(device="cuda"); gen.manual_seed(n + S)
            x = torch.randn((n, S), generator=gen, **f32)
            term = torch.randint(0, 3, (n,), generator=gen, device="cuda", dtype=torch.int32)
            task = torch.rand((n,), generator=gen, **f32)
            done = (torch.rand((n,), generator=gen, **f32) < a.done_rate).to(torch.int32)
            out = torch.empty(n, **f32); act = torch.empty((n, 1), **f32)
            fail, succ = torch.tensor(0.0, **f32), torch.tensor(20.0, **f32)

            def scalar():
                if kind == "value":
                    head.eval_device(x.data_ptr(), n, out.data_ptr(), stream=stream, terminate_ptr=term.data_ptr())
                else:
                    head.eval_device(x.data_ptr(), n, out.data_ptr(), stream=stream, task_reward_ptr=task.data_ptr())

            def actor1():
                actor.forward_device(x.data_ptr(), n, act.data_ptr(), stream=stream)
                y = act[:, 0]
                if kind == "value":
                    v = torch.clamp(y, -1.0, 1.0)
                    return torch.where(term == 1, fail, torch.where(term == 2, succ, v))
                d = 1.0 - y
                r = 2.0 * torch.clamp(1.0 - 0.25 * d * d, min=0.0)
                return 0.5 * r + 0.5 * task

            arms = [("scalar", scalar), ("actor1", actor1)]
            if kind == "value":
                arms += [("scalar_masked", lambda: head.eval_device(x.data_ptr(), n, out.data_ptr(), stream=stream, row_mask_ptr=done.data_ptr())),
                         ("scalar_unmasked", lambda: head.eval_device(x.data_ptr(), n, out.data_ptr(), stream=stream))]
            for _ in range(a.warmup):
                for _, fn in arms:
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k, _ in arms}
            for _ in range(a.reps):                      # interleaved: one repetition of every arm per round
                for k, fn in arms:
                    times[k].append(timed(fn))
            row = dict(net=name, S=S, goal_dim=G, head=kind, rows=n, done_rate=a.done_rate, path=head.info()["path"], us=times,
                       median_us={k: float(np.median(v)) for k, v in times.items()}, min_us={k: float(np.min(v)) for k, v in times.items()})
            results.append(row)
            print("SCALAR_HEADS_BENCH %s rows %d median us %s" % (name, n, {k: round(v, 1) for k, v in row["median_us"].items()}), flush=True)
        head.close(); actor.close()
    dev = torch.cuda.get_device_properties(0)
    doc = dict(tool="tools/scalar_heads_bench.py", device=dev.name, reps=a.reps, warmup=a.warmup, timing="HIP events around each arm, arms interleaved per repetition, one process",
               results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
