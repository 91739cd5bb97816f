"""Time of the TD(lambda) kernel (deepmimic_amd/csrc/dm_returns.h) at rollout size, against the same reverse loop written with torch ops on the same tensors.
The two are run interleaved in one process, each timed with HIP events on the current stream; medians over the timed repetitions after a warm-up, with the
quartiles next to them.  Writes one JSON object (default profiles/td_returns_bench.json).
usage: python tools/returns_bench.py [--T 32] [--N 4096] [--reps 200] [--warmup 20] [--out profiles/td_returns_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import returns  # noqa: E402


def torch_loop(r, v, tv, term, done, valid, gamma, lam, vf, vs):
    """the recursion of include/dm_hip.h dm_td_lambda_returns as a reverse loop of torch ops, float64 inside (what a learner writes without the kernel)"""
    T, N = r.shape
    ret = torch.empty((T, N), dtype=torch.float32, device=r.device); mask = torch.empty((T, N), dtype=torch.int32, device=r.device)
    nxt = torch.zeros(N, dtype=torch.float64, device=r.device); inv = torch.zeros(N, dtype=torch.bool, device=r.device)
    fail, succ = torch.full((N,), vf, dtype=torch.float64, device=r.device), torch.full((N,), vs, dtype=torch.float64, device=r.device)
    for t in range(T - 1, -1, -1):
        d = done[t] != 0
        end_v = torch.where(term[t] == 1, fail, torch.where(term[t] == 2, succ, tv[t].double()))
        v_next = torch.where(d, end_v, v[t + 1].double())
        closes = d if t < T - 1 else torch.ones_like(d)
        cur = torch.where(closes, r[t].double() + gamma * v_next, r[t].double() + gamma * ((1.0 - lam) * v_next + lam * nxt))
        inv = torch.where(d, valid[t] == 0, inv)
        ret[t] = cur.float(); mask[t] = (~inv).int(); nxt = cur
    return ret, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32); ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td_returns_bench.json"))
    a = ap.parse_args()
    T, N = a.T, a.N
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    f = lambda *s: torch.rand(s, generator=g, dtype=torch.float32, device="cuda")
    r, v, tv = f(T, N), f(T + 1, N) * 10, f(T, N) * 10
    done = (f(T, N) < 0.05).int(); term = (torch.randint(0, 3, (T, N), generator=g, device="cuda").int() * done).int()
    valid = (1 - done * (f(T, N) < 0.1).int()).int()
    args = (r, v, tv, term, done, valid, 0.95, 0.95, 0.0, 20.0)
    k_ret, k_mask = returns.td_lambda_returns_torch(*args)
    t_ret, t_mask = torch_loop(*args)
    torch.cuda.synchronize()
    # fp64 with one rounding on both sides; torch may contract a * b + c, so the two need not agree in the last bit
    agree = dict(max_abs_diff=float((k_ret.double() - t_ret.double()).abs().max()), mask_equal=bool((k_mask == t_mask).all()))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3          # us
    kern = lambda: returns.td_lambda_returns_torch(*args)
    loop = lambda: torch_loop(*args)
    for _ in range(a.warmup):
        kern(); loop()
    torch.cuda.synchronize()
    tk, tl = [], []
    for _ in range(a.reps):
        tk.append(timed(kern)); tl.append(timed(loop))
    q = lambda x: [float(np.percentile(x, p)) for p in (25, 50, 75)]
    nbytes = 32 * T * N + 4 * N                    # six input arrays (values has T + 1 rows), returns and mask, 4 bytes each
    out = dict(what="dm_td_lambda_returns vs the same reverse loop in torch ops, interleaved in one process, HIP events, microseconds (the kernel's time includes the "
                    "allocation of its two output tensors and the launch through ctypes)",
               T=T, N=N, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               kernel_us_q25_median_q75=q(tk), torch_loop_us_q25_median_q75=q(tl), bytes_moved=nbytes,
               kernel_bytes_per_s=nbytes / (float(np.median(tk)) * 1e-6), torch_loop_over_kernel=float(np.median(tl) / np.median(tk)), agreement=agree)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
