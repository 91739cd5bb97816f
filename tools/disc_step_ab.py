"""Times of one AMP discriminator update at the reference's widths (the humanoid's amp_obs 226 -> 1024 -> 512 -> 1) on the device trainer against the torch fp32 route,
same box:
  device   DiscTrainer.grad + DiscTrainer.step (deepmimic_amd/train.py: forward on the context's kernels, head, least-squares backward, the gradient penalty's chain on
           the expert rows, momentum step with weight decay, refresh of the context)
  torch    nn.Linear forward, the same loss with autograd.grad(create_graph=True) for the penalty, backward, SGD(momentum, weight_decay), Discriminator.set_weights_torch
at n_expert = n_agent = 256 (the reference's DiscBatchSize) and 2048.  Each row count runs in a child process of its own under `timeout`; inside it the two arms alternate,
every call bracketed by HIP events on the current stream, warm, medians of --reps repetitions with the quartiles.
The per-kernel split comes from a run of its own, one child under the profiler: `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/disc_step_ab.py --worker N`;
`--kernel-stats N=its_kernel_stats.csv ...` then adds the library's kernels (average ns per launch) to the rows of an existing output file instead of timing anything.
Writes one JSON object (default profiles/disc_step_ab.json).
usage: python tools/disc_step_ab.py [--rows 256 2048] [--reps 50] [--warmup 10] [--timeout 240] [--out profiles/disc_step_ab.json] [--kernel-stats 256=a.csv 2048=b.csv]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_step_ab import quart  # noqa: E402

S, H1, H2 = 226, 1024, 512
GRAD_PENALTY, LOGIT_REG, WEIGHT_DECAY, STEPSIZE = 10.0, 0.05, 5e-4, 1e-5


def worker(n, reps, warmup):
    import torch
    from deepmimic_amd import heads
    from deepmimic_amd import train as tr
    from deepmimic_amd.policy import random_weights
    if not torch.cuda.is_available():
        raise SystemExit("disc_step_ab needs a GPU (deepmimic_amd has no CPU path)")
    dev = torch.device("cuda", 0)
    w = random_weights(S, 1, H1=H1, H2=H2, seed=1)
    w = {k: v for k, v in w.items() if k not in ("a_mean", "a_std", "logstd")}
    rng = np.random.default_rng(2)
    w["s_mean"] = rng.uniform(-0.5, 0.5, S).astype(np.float32); w["s_std"] = rng.uniform(0.5, 2, S).astype(np.float32)
    disc, disc_t = heads.Discriminator(w), heads.Discriminator(w)
    trn = tr.DiscTrainer.from_policy(disc.net, w, stepsize=STEPSIZE, momentum=0.9, weight_decay=WEIGHT_DECAY)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    expert, agent = t(rng.standard_normal((n, S)) + 0.2), t(rng.standard_normal((n, S)) - 0.2)
    # the torch route: a second copy of the net in torch.nn, the loss by hand, the penalty by a double backward pass
    net = torch.nn.Sequential(torch.nn.Linear(S, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU(), torch.nn.Linear(H2, 1)).to(dev)
    with torch.no_grad():
        for lin, (wk, bk) in zip((net[0], net[2], net[4]), (("w1", "b1"), ("w2", "b2"), ("w3", "b3"))):
            lin.weight.copy_(t(w[wk]).T); lin.bias.copy_(t(w[bk]).reshape(-1))
    mats = [net[0].weight, net[2].weight, net[4].weight]
    opt = torch.optim.SGD([dict(params=mats, weight_decay=WEIGHT_DECAY), dict(params=[net[0].bias, net[2].bias, net[4].bias], weight_decay=0.0)], lr=STEPSIZE, momentum=0.9)
    s_mean, s_inv = t(w["s_mean"]), 1.0 / t(w["s_std"])

    def torch_fwd_bwd():
        opt.zero_grad(set_to_none=True)
        xe = ((expert - s_mean) * s_inv).requires_grad_(True)
        ye, ya = net(xe)[:, 0], net((agent - s_mean) * s_inv)[:, 0]
        loss = 0.5 * ((0.5 * (ye - 1).square()).mean() + (0.5 * (ya + 1).square()).mean())
        gx, = torch.autograd.grad(ye.sum(), xe, create_graph=True)
        loss = loss + GRAD_PENALTY * 0.5 * gx.square().sum(1).mean() + LOGIT_REG * 0.5 * net[4].weight.square().sum()
        loss.backward()

    def torch_refresh():
        disc_t.set_weights_torch(dict(w1=net[0].weight, b1=net[0].bias, w2=net[2].weight, b2=net[2].bias, w3=net[4].weight, b3=net[4].bias), layout="out_in")

    phases = {"device_grad": lambda: trn.grad(expert, agent, grad_penalty=GRAD_PENALTY, logit_reg=LOGIT_REG), "device_step": trn.step,
              "torch_forward_backward": torch_fwd_bwd, "torch_optimizer": opt.step, "torch_refresh": torch_refresh}
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
    out.update(n_expert=n, n_agent=n, reps=reps, warmup=warmup, stats=dict(zip(tr.DISC_STATS, (float(x) for x in trn.stats().cpu()))))
    print("DISC_STEP_AB " + json.dumps(out))


def merge_kernel_stats(out_path, specs):
    """the library's rows (namespaces dmt and dmp, templates included) of rocprofv3's kernel_stats.csv files into res["rows"][n]["kernel_split"]:
    {kernel: {calls, average_us, min_us, max_us}}"""
    import csv
    res = json.load(open(out_path))
    for spec in specs:
        n, path = spec.split("=", 1)
        split = {}
        for row in csv.DictReader(open(path)):
            short = row["Name"].replace("void ", "").split("(")[0]
            if short.startswith(("dmt::", "dmp::")):
                split[short] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2), min_us=round(float(row["MinNs"]) / 1e3, 2),
                                    max_us=round(float(row["MaxNs"]) / 1e3, 2))
        res["rows"][n]["kernel_split"] = split
    res["kernel_split_source"] = "rocprofv3 --kernel-trace --stats, a run of its own (20 repetitions after 5 warm-up ones, both arms in the process; the profiler slows the host, not the kernels)"
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 2048]); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240); ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_step_ab.json"))
    ap.add_argument("--kernel-stats", nargs="+", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.out, a.kernel_stats)
    if a.worker:
        return worker(a.worker, a.reps, a.warmup)
    res = {"widths": [S, H1, H2, 1], "coefficients": dict(grad_penalty=GRAD_PENALTY, logit_reg=LOGIT_REG, weight_decay=WEIGHT_DECAY),
           "timing": "HIP events around each call on the current stream, the phases alternating inside every repetition, warm", "rows": {}}
    for n in a.rows:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                            # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("disc_step_ab: the n = %d step ended with status %d" % (n, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("DISC_STEP_AB ")][-1]
        res["rows"][str(n)] = json.loads(line[len("DISC_STEP_AB "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
