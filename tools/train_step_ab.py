"""Times of one PPO actor update at the reference's widths (197 -> 1024 -> 512 -> 36) on the device trainer against the torch fp32 route of INTEGRATION.md, same box:
  device   ActorTrainer.grad + ActorTrainer.step (deepmimic_amd/train.py: forward on the context's kernels, head, backward on the matrix cores, momentum step, refresh)
  torch    nn.Linear forward, the same loss (clipped surrogate + action-bound loss), backward, SGD(momentum), Policy.set_weights_torch
at n = 256 (the reference's minibatch) and n = 4096.  Each n runs in a child process of its own under `timeout`; inside it the two arms alternate, every call bracketed by
HIP events on the current stream, warm, medians of --reps repetitions with the quartiles.  The split: device grad / step, torch forward + backward / optimiser / refresh.
The per-kernel split comes from a run of its own, one child under the profiler: `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/train_step_ab.py --worker N`;
`--kernel-stats N=its_kernel_stats.csv ...` then adds the library's kernels (average ns per launch) to the rows of an existing output file instead of timing anything.
Writes one JSON object (default profiles/train_step_ab.json).
usage: python tools/train_step_ab.py [--rows 256 4096] [--reps 50] [--warmup 10] [--timeout 240] [--out profiles/train_step_ab.json] [--kernel-stats 256=a.csv 4096=b.csv]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, H1, H2, A = 197, 1024, 512, 36


def quart(xs):
    q = np.percentile(np.asarray(xs), [25, 50, 75])
    return dict(median_us=round(float(q[1]) * 1e3, 2), q1_us=round(float(q[0]) * 1e3, 2), q3_us=round(float(q[2]) * 1e3, 2))


def worker(n, reps, warmup):
    import torch
    from deepmimic_amd import train as tr
    from deepmimic_amd.policy import Policy, random_weights
    if not torch.cuda.is_available():
        raise SystemExit("train_step_ab needs a GPU (deepmimic_amd has no CPU path)")
    dev = torch.device("cuda", 0)
    w = random_weights(S, A, H1=H1, H2=H2, seed=1)
    rng = np.random.default_rng(2)
    w["s_mean"] = rng.uniform(-0.5, 0.5, S).astype(np.float32); w["s_std"] = rng.uniform(0.5, 2, S).astype(np.float32)
    w["a_mean"] = np.zeros(A, np.float32); w["a_std"] = np.ones(A, np.float32)
    pol, pol_t = Policy(w), Policy(w)
    trn = tr.ActorTrainer.from_policy(pol, w, stepsize=1e-4, momentum=0.9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    states = t(rng.standard_normal((n, S)))
    actions, old = torch.empty((n, A), device=dev), torch.empty(n, device=dev)
    pol.forward_device_ex(states.data_ptr(), n, actions.data_ptr(), logp_ptr=old.data_ptr(), sample=True, seed=3, stream=torch.cuda.current_stream().cuda_stream)
    adv = t(rng.standard_normal(n))
    lo, hi = np.full(A, -1.0, np.float32), np.full(A, 1.0, np.float32)
    # the torch route: a second copy of the net in torch.nn, the loss by hand
    net = torch.nn.Sequential(torch.nn.Linear(S, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU(), torch.nn.Linear(H2, A)).to(dev)
    with torch.no_grad():
        for lin, (wk, bk) in zip((net[0], net[2], net[4]), (("w1", "b1"), ("w2", "b2"), ("w3", "b3"))):
            lin.weight.copy_(t(w[wk]).T); lin.bias.copy_(t(w[bk]))
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)
    s_mean, s_inv, logstd = t(w["s_mean"]), 1.0 / t(w["s_std"]), t(w["logstd"])
    lo_t, hi_t = t(lo), t(hi)

    def torch_fwd_bwd():
        opt.zero_grad(set_to_none=True)
        mu = net((states - s_mean) * s_inv)
        u = (actions - mu) * torch.exp(-logstd)
        logp = -0.5 * (u * u).sum(1) - 0.5 * A * float(np.log(2 * np.pi)) - logstd.sum()
        ratio = torch.exp(logp - old)
        loss = -torch.minimum(adv * ratio, adv * ratio.clamp(0.8, 1.2)).mean()
        loss = loss + 10.0 * 0.5 * ((mu - lo_t).clamp(max=0).square().sum(1) + (mu - hi_t).clamp(min=0).square().sum(1)).mean()
        loss.backward()

    def torch_refresh():
        pol_t.set_weights_torch(dict(w1=net[0].weight, b1=net[0].bias, w2=net[2].weight, b2=net[2].bias, w3=net[4].weight, b3=net[4].bias), layout="out_in")

    phases = {"device_grad": lambda: trn.grad(states, actions, old, adv, ratio_clip=0.2, bound_weight=10.0, a_bound_min=lo, a_bound_max=hi),
              "device_step": trn.step, "torch_forward_backward": torch_fwd_bwd, "torch_optimizer": opt.step, "torch_refresh": torch_refresh}
    times = {k: [] for k in phases}
    for it in range(warmup + reps):
        for k, f in phases.items():                      # the arms alternate inside every repetition
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); e1.synchronize()
            if it >= warmup:
                times[k].append(e0.elapsed_time(e1))
    total = lambda keys: [sum(v) for v in zip(*[times[k] for k in keys])]
    out = {k: quart(v) for k, v in times.items()}
    out["device_update"] = quart(total(["device_grad", "device_step"]))
    out["torch_update"] = quart(total(["torch_forward_backward", "torch_optimizer", "torch_refresh"]))
    out.update(n=n, reps=reps, warmup=warmup, stats=[float(x) for x in trn.stats().cpu()])
    print("TRAIN_STEP_AB " + json.dumps(out))


def merge_kernel_stats(out_path, specs):
    """the dmt:: / dmp:: rows of rocprofv3's kernel_stats.csv files into res["rows"][n]["kernel_split"]: {kernel: {calls, average_us, min_us, max_us}}"""
    import csv
    res = json.load(open(out_path))
    for spec in specs:
        n, path = spec.split("=", 1)
        split = {}
        for row in csv.DictReader(open(path)):
            name = row["Name"]
            if name.startswith(("dmt::", "dmp::", "void dmp::")):
                short = name.replace("void ", "").split("(")[0]
                split[short] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2), min_us=round(float(row["MinNs"]) / 1e3, 2),
                                    max_us=round(float(row["MaxNs"]) / 1e3, 2))
        res["rows"][n]["kernel_split"] = split
    res["kernel_split_source"] = "rocprofv3 --kernel-trace --stats, a run of its own (20 repetitions after 5 warm-up ones, both arms in the process; the profiler slows the host, not the kernels)"
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096]); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240); ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_ab.json"))
    ap.add_argument("--kernel-stats", nargs="+", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.out, a.kernel_stats)
    if a.worker:
        return worker(a.worker, a.reps, a.warmup)
    res = {"widths": [S, H1, H2, A], "timing": "HIP events around each call on the current stream, the phases alternating inside every repetition, warm", "rows": {}}
    for n in a.rows:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                            # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("train_step_ab: the n = %d step ended with status %d" % (n, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("TRAIN_STEP_AB ")][-1]
        res["rows"][str(n)] = json.loads(line[len("TRAIN_STEP_AB "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
