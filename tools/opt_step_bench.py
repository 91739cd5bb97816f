"""Times of the optimiser step that ends a minibatch (deepmimic_amd/csrc/dm_optim.h, deepmimic_amd/train.py), one MI355X, one process, the arms alternating, whole
calls bracketed by HIP events on the current stream, every repetition kept.  Per net -- the plain actor at the reference's widths, the 226 -> 1024 -> 512 -> 1
discriminator, the gated actor -- on a fixed gradient block:
  sgd_step         dm_train_sgd_step / dm_train_gated_sgd_step: the momentum step and the refresh of the context, unchanged code: the yardstick
  opt_momentum     dm_train_opt_step MOMENTUM with clipping and the guard on (norm pass, decisions, step, refresh)
  opt_adam         the same with ADAM
  torch_adam       clip_grad_norm_ + torch.optim.Adam on one [P] fp32 parameter, then Policy.set_weights_torch on its views (the refresh a torch learner needs)
  torch_adam_item  the same behind the `.item()` finiteness check a host-side guard costs
Bytes per second are the arrays a call must move once (norm 4 P, momentum step 16 P, Adam 28 P, the refresh reads 4 P and writes 2 P), not a measured traffic.
Writes one JSON object (default profiles/opt_step_bench.json).
usage: python tools/opt_step_bench.py [--reps 50] [--warmup 10] [--out profiles/opt_step_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import train as tr  # noqa: E402
from deepmimic_amd.policy import Policy, random_weights  # noqa: E402

NETS = dict(actor=dict(S=197, A=36), disc=dict(S=226, A=1), gated_actor=dict(S=200, A=36, gated_goal_dim=3))
NOTE = ("expectation, not a threshold: at these sizes (P about 0.75 M, 3 to 20 MB per call) every launch is latency-bound, so dm_train_opt_step with clipping and the "
        "guard should cost dm_train_sgd_step plus two small launches (k_opt_sq, k_opt_begin), and Adam a little more for its 28 bytes per element; the torch arms pay "
        "several launches for the norm, the foreach Adam kernels, the refresh, and with the guard one host read")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def arms_of(name, dims, dev):
    gated = "gated_goal_dim" in dims
    w = random_weights(dims["S"], dims["A"], seed=3, **({k: v for k, v in dims.items() if k == "gated_goal_dim"}))
    cls = tr.GatedActorTrainer if gated else (tr.DiscTrainer if name == "disc" else tr.ActorTrainer)
    kw = dict(stepsize=1e-4, weight_decay=1e-4, device=dev)
    old = cls.from_policy(Policy(w), w, momentum=0.9, **kw)
    mom = cls.from_policy(Policy(w), w, momentum=0.9, max_grad_norm=1.0, skip_nonfinite=True, **kw)
    adam = cls.from_policy(Policy(w), w, optimizer="adam", max_grad_norm=1.0, skip_nonfinite=True, **kw)
    P = old.P
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    grads = 0.01 * torch.randn(P, generator=g, device=dev)
    for t in (old, mom, adam):
        t.grads.copy_(grads)
    # the torch route: one flat parameter, the context refreshed from its views
    pol = Policy(w)
    flat = torch.nn.Parameter(old.params.clone())
    flat.grad = grads.clone()
    opt = torch.optim.Adam([flat], lr=1e-4, weight_decay=1e-4)
    views = old._unpack(flat.data, pol)

    def torch_adam(check):
        if check and not bool(torch.isfinite(flat.grad).all().item()):
            return
        torch.nn.utils.clip_grad_norm_([flat], 1.0)
        opt.step()
        pol.set_weights_torch(views)
    runs = dict(sgd_step=old.step, opt_momentum=mom.step, opt_adam=adam.step, torch_adam=lambda: torch_adam(False), torch_adam_item=lambda: torch_adam(True))
    moved = dict(sgd_step=22 * P, opt_momentum=26 * P, opt_adam=38 * P, torch_adam=38 * P, torch_adam_item=42 * P)
    return P, runs, moved, (mom, adam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opt_step_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("opt_step_bench needs a GPU (deepmimic_amd has no CPU path)")
    dev = torch.device("cuda:0")
    nets = {}
    for name, dims in NETS.items():
        P, runs, moved, (mom, adam) = arms_of(name, dims, dev)
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                times[k].append(timed(fn))
        q = {k: quartiles(v) for k, v in times.items()}
        nets[name] = dict(P=P, us_q25_median_q75=q, bytes_moved=moved, gbytes_per_s_at_median={k: moved[k] / q[k][1] * 1e-3 for k in runs},
                          last_norm=dict(opt_momentum=float(mom.grad_norm().cpu()), opt_adam=float(adam.grad_norm().cpu())),
                          skipped=dict(opt_momentum=float(mom.skipped().cpu()), opt_adam=float(adam.skipped().cpu())), us_every_repetition=times)
    out = dict(what="the optimiser step that ends a minibatch, refresh of the context included (microseconds per call, HIP events around whole calls, arms alternating; every "
                    "time includes the Python / ctypes launch path)", note=NOTE, device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               host_reads_per_call=dict(sgd_step=0, opt_momentum=0, opt_adam=0, torch_adam=0, torch_adam_item=1), nets=nets)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({n: {k: v for k, v in d.items() if k != "us_every_repetition"} for n, d in nets.items()}))


if __name__ == "__main__":
    main()
