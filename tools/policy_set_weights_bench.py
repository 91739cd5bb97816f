"""What a weight refresh of a device policy costs at the reference widths (S = 197, A = 28, 1024 / 512; plain and gated with goal_dim 3, gate 128 / 64), for
parameters that live in torch tensors on the GPU in torch.nn.Linear layout ([out, in]):

 (a) rebuild: the tensors to the host, dm_policy_destroy + dm_policy_create(_gated) (a dozen allocations, the fp32 arrays staged to the device, one k_policy_pack launch) and the first forward
     afterwards, which regrows the activation buffers behind a stream synchronise -- the only route before dm_policy_set_weights;
 (b) refresh: Policy.set_weights_torch(layout="out_in") and the same forward, enqueued back to back on one stream and timed as ONE event interval, so a host
     synchronisation inside the refresh would show as a gap (host_enqueue_us is the host's time for the two calls; it returns before the work is done).

Also timed alone: the refresh, the forward, and a plain device-to-device copy of the same fp32 parameters (what the refresh reads; it writes half as much).
All in one process on one device, the routes interleaved per repetition, HIP events on the current stream, microseconds, after a warm-up.  Every repetition is
written to the JSON (default profiles/policy_set_weights.json) next to the medians.
usage: python tools/policy_set_weights_bench.py [--rows 4096] [--reps 30] [--warmup 5] [--out profiles/policy_set_weights.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd.policy import Policy, random_weights  # noqa: E402


def measure(gated, rows, reps, warmup):
    S, A, G = (200, 28, 3) if gated else (197, 28, 0)
    w = random_weights(S, A, seed=1, gated_goal_dim=G)
    host = {k: v for k, v in w.items() if k != "goal_dim"}
    # the learner's side: [out, in] tensors on the device
    dev = {k: torch.from_numpy(np.ascontiguousarray(v.T if v.ndim == 2 else v)).cuda() for k, v in host.items()}
    nbytes = int(sum(t.numel() for t in dev.values()) * 4)
    flat_src = torch.empty(nbytes // 4, device="cuda"); flat_dst = torch.empty_like(flat_src)
    ts = torch.randn((rows, S), device="cuda"); ta = torch.zeros((rows, A), device="cuda"); tl = torch.zeros(rows, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    box = dict(pol=Policy(w, lib_path=None))

    def forward():
        box["pol"].forward_device(ts.data_ptr(), rows, ta.data_ptr(), tl.data_ptr(), stream=stream)

    def rebuild():
        hw = {k: (t.cpu().numpy().T if t.dim() == 2 else t.cpu().numpy()) for k, t in dev.items()}
        if gated:
            hw["goal_dim"] = G
        box["pol"].close()
        box["pol"] = Policy(hw, lib_path=None)
        forward()

    def refresh():
        box["pol"].set_weights_torch(dev, layout="out_in")

    def refresh_forward():
        refresh(); forward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); t0 = time.perf_counter(); fn(); t1 = time.perf_counter(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, (t1 - t0) * 1e6
    routes = dict(rebuild_forward=rebuild, refresh_forward=refresh_forward, refresh=refresh, forward=forward, d2d_copy=lambda: flat_dst.copy_(flat_src))
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}; enqueue = []
    for _ in range(reps):
        for k, fn in routes.items():
            dt, host_dt = timed(fn)
            times[k].append(dt)
            if k == "refresh_forward":
                enqueue.append(host_dt)
    torch.cuda.synchronize()
    info = box["pol"].info()
    box["pol"].close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(S=S, A=A, goal_dim=G, rows=rows, gated_fused=info["gated_fused"], fused=info["fused"], parameter_bytes=nbytes, launches_per_refresh=1,
                median_us=med, refresh_forward_host_enqueue_median_us=float(np.median(enqueue)),
                rebuild_over_refresh=med["rebuild_forward"] / med["refresh_forward"],
                refresh_read_bytes_per_s=nbytes / (med["refresh"] * 1e-6), d2d_copy_bytes_per_s=nbytes / (med["d2d_copy"] * 1e-6),
                repetitions_us=times, refresh_forward_host_enqueue_us=enqueue)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096); ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_set_weights.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    torch.zeros(1, device="cuda")
    out = dict(what="weight refresh of a device policy: rebuild (tensors to host, destroy + create, first forward) against set_weights_torch + forward, interleaved in one "
                    "process, HIP event intervals on one stream, microseconds", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               plain=measure(False, a.rows, a.reps, a.warmup), gated=measure(True, a.rows, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: (dict(median_us=v["median_us"], host_enqueue_us=v["refresh_forward_host_enqueue_median_us"], rebuild_over_refresh=v["rebuild_over_refresh"])
                          if isinstance(v, dict) else v) for k, v in out.items()}))
    for k in ("plain", "gated"):
        if not out[k]["median_us"]["refresh_forward"] < out[k]["median_us"]["rebuild_forward"]:
            raise SystemExit("%s: the refresh route (%.0f us) does not beat the rebuild route (%.0f us)" % (k, out[k]["median_us"]["refresh_forward"], out[k]["median_us"]["rebuild_forward"]))


if __name__ == "__main__":
    main()
