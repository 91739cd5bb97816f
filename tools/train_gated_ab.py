"""Times of one GATED PPO actor update at the widths of the AMP task agents (200 -> 1024 -> 512 -> 36, the last G = 3 input columns the goal, gate 128 / 64) on the
same box, in one process:
  gated   GatedActorTrainer.grad + GatedActorTrainer.step (deepmimic_amd/train.py, dm_train_gated_*: forward on the context's gated per-layer route, head, backward through
          sigma, beta and the gate on the matrix cores, momentum step over the twenty arrays, refresh of the context with its gate)
  torch   the fp32 route a user had before: the gated net written in torch (parameters in tf.layers.dense layout), the same loss (clipped surrogate + action-bound loss),
          autograd, SGD(momentum), Policy.set_weights_torch of all twenty arrays
  plain   ActorTrainer.grad + step on the plain net at 197 inputs: what the gate costs on top of the update that was on the device already
at n = 256 (the reference's minibatch) and n = 4096.  The arms alternate inside every repetition; a whole call (grad, step, forward + backward, optimiser, refresh) is
bracketed by HIP events on the current stream, after --warmup warm repetitions.  EVERY repetition is written (milliseconds), with medians and quartiles beside them.
usage: python tools/train_gated_ab.py [--rows 256 4096] [--reps 50] [--warmup 10] [--out profiles/train_gated_ab.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, G, H1, H2, A, GC, GH = 200, 3, 1024, 512, 36, 128, 64


def quart(xs):
    q = np.percentile(np.asarray(xs), [25, 50, 75])
    return dict(median_us=round(float(q[1]) * 1e3, 2), q1_us=round(float(q[0]) * 1e3, 2), q3_us=round(float(q[2]) * 1e3, 2))


def measure(n, reps, warmup):
    import torch
    from deepmimic_amd import train as tr
    from deepmimic_amd.policy import Policy, random_weights
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2)
    def with_norm(w, width):
        w["s_mean"] = rng.uniform(-0.5, 0.5, width).astype(np.float32); w["s_std"] = rng.uniform(0.5, 2, width).astype(np.float32)
        w["a_mean"] = np.zeros(A, np.float32); w["a_std"] = np.ones(A, np.float32)
        return w
    w = with_norm(random_weights(S, A, H1=H1, H2=H2, seed=1, gated_goal_dim=G, gate_common=GC, gate_hidden=GH), S)
    wp = with_norm(random_weights(S - G, A, H1=H1, H2=H2, seed=1), S - G)
    pol, pol_t, pol_p = Policy(w), Policy(w), Policy(wp)
    trn = tr.GatedActorTrainer.from_policy(pol, w, stepsize=1e-4, momentum=0.9)
    trn_p = tr.ActorTrainer.from_policy(pol_p, wp, stepsize=1e-4, momentum=0.9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    states = t(rng.standard_normal((n, S)))
    states_p = states[:, :S - G].contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    actions, old = torch.empty((n, A), device=dev), torch.empty(n, device=dev)
    pol.forward_device_ex(states.data_ptr(), n, actions.data_ptr(), logp_ptr=old.data_ptr(), sample=True, seed=3, stream=stream)
    actions_p, old_p = torch.empty((n, A), device=dev), torch.empty(n, device=dev)
    pol_p.forward_device_ex(states_p.data_ptr(), n, actions_p.data_ptr(), logp_ptr=old_p.data_ptr(), sample=True, seed=3, stream=stream)
    adv = t(rng.standard_normal(n))
    lo, hi = np.full(A, -1.0, np.float32), np.full(A, 1.0, np.float32)
    # the torch route: the gated net on a second copy of the parameters
    p = {k: t(w[k]).requires_grad_(True) for k in tr.GATED_KEYS}
    opt = torch.optim.SGD(list(p.values()), lr=1e-4, momentum=0.9)
    s_mean, s_inv, logstd = t(w["s_mean"]), 1.0 / t(w["s_std"]), t(w["logstd"])
    lo_t, hi_t = t(lo), t(hi)

    def torch_fwd_bwd():
        opt.zero_grad(set_to_none=True)
        x = (states - s_mean) * s_inv
        c = torch.relu(x[:, S - G:] @ p["gc_w"] + p["gc_b"])
        h = x
        for i in (0, 1):
            e = torch.relu(c @ p["g%d_w" % i] + p["g%d_b" % i])
            beta = e @ p["g%d_bias_w" % i] + p["g%d_bias_b" % i]
            sigma = 2 * torch.sigmoid(e @ p["g%d_scale_w" % i] + p["g%d_scale_b" % i])
            h = torch.relu(sigma * (h @ p["w%d" % (i + 1)] + p["b%d" % (i + 1)]) + beta)
        mu = h @ p["w3"] + p["b3"]
        u = (actions - mu) * torch.exp(-logstd)
        logp = -0.5 * (u * u).sum(1) - 0.5 * A * float(np.log(2 * np.pi)) - logstd.sum()
        ratio = torch.exp(logp - old)
        loss = -torch.minimum(adv * ratio, adv * ratio.clamp(0.8, 1.2)).mean()
        loss = loss + 10.0 * 0.5 * ((mu - lo_t).clamp(max=0).square().sum(1) + (mu - hi_t).clamp(min=0).square().sum(1)).mean()
        loss.backward()

    kw = dict(ratio_clip=0.2, bound_weight=10.0, a_bound_min=lo, a_bound_max=hi)
    phases = {"gated_grad": lambda: trn.grad(states, actions, old, adv, **kw), "gated_step": trn.step,
              "torch_forward_backward": torch_fwd_bwd, "torch_optimizer": opt.step, "torch_refresh": lambda: pol_t.set_weights_torch({k: v.detach() for k, v in p.items()}),
              "plain_grad": lambda: trn_p.grad(states_p, actions_p, old_p, adv, **kw), "plain_step": trn_p.step}
    times = {k: [] for k in phases}
    for it in range(warmup + reps):
        for k, f in phases.items():                      # the arms alternate inside every repetition
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); e1.synchronize()
            if it >= warmup:
                times[k].append(e0.elapsed_time(e1))
    total = lambda keys: [sum(v) for v in zip(*[times[k] for k in keys])]
    times["gated_update"] = total(["gated_grad", "gated_step"])
    times["torch_update"] = total(["torch_forward_backward", "torch_optimizer", "torch_refresh"])
    times["plain_update"] = total(["plain_grad", "plain_step"])
    out = {k: quart(v) for k, v in times.items()}
    out["repetitions_ms"] = {k: [round(x, 5) for x in v] for k, v in times.items()}
    out.update(n=n, reps=reps, warmup=warmup, stats=[float(x) for x in trn.stats().cpu()])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096]); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_gated_ab.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_gated_ab needs a GPU (deepmimic_amd has no CPU path)")
    res = {"widths": dict(S=S, G=G, H1=H1, H2=H2, A=A, GC=GC, GH=GH, plain_S=S - G),
           "timing": "HIP events around each whole call on the current stream, one process, the arms alternating inside every repetition, warm", "rows": {}}
    for n in a.rows:
        res["rows"][str(n)] = measure(n, a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for n, row in res["rows"].items():
        print("n = %s: " % n + "  ".join("%s %.1f us" % (k, row[k]["median_us"]) for k in ("gated_update", "torch_update", "plain_update")))


if __name__ == "__main__":
    main()
