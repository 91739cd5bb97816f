"""Times of the PPO batch stage (deepmimic_amd/csrc/dm_ppo_batch.h) at rollout size against the same stage written with public torch calls on the same tensors:
  (a) advantages   ppo_batch.advantages_torch (five launches, no host synchronisation)   vs   torch_advantages below (boolean masks, nonzero, index_select, mean / std)
  (b) minibatch    one critic gather from the valid list + one actor gather from the exp list (two launches, the shuffle evaluated per row)
                   vs   torch_minibatch below (six index_selects through a stored permutation), and torch_shuffle (the two randperms an epoch costs before it)
The pairs run interleaved in one process, each call timed with HIP events on the current stream; medians over the timed repetitions after a warm-up, with the
quartiles next to them.  The torch side stands for what a learner writes without the kernels; its nonzero() waits for the device, which the event timing includes.
Writes one JSON object (default profiles/ppo_batch_bench.json).
usage: python tools/ppo_batch_bench.py [--T 32] [--N 4096] [--S 227] [--A 28] [--M 4096] [--reps 200] [--warmup 20] [--out profiles/ppo_batch_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import ppo_batch  # noqa: E402


def torch_advantages(ret, values, mask, flags, eps, clip, vmin, vmax):
    """ppo_agent.py:159-172 on device tensors, float64 inside: the lists by nonzero (a host synchronisation each), the statistics by torch's reductions"""
    T = ret.shape[0]
    valid = mask.reshape(-1) != 0
    exp = valid & (flags.reshape(-1) != 0)
    valid_idx, exp_idx = valid.nonzero().squeeze(1), exp.nonzero().squeeze(1)
    a = (ret.double() - values[:T].double()).reshape(-1)
    ae = a.index_select(0, exp_idx)
    mean, std = ae.mean(), ae.std(unbiased=False)
    adv = torch.zeros_like(a)
    adv[exp_idx] = ((ae - mean) / (std + eps)).clamp(-clip, clip)
    return adv.float().view_as(ret), ret.clamp(vmin, vmax), valid_idx, exp_idx, torch.stack([mean, std])


def torch_shuffle(valid_idx, exp_idx):
    """ppo_agent.py:179-180: a fresh shuffle of both lists, once per epoch"""
    return valid_idx[torch.randperm(valid_idx.numel(), device=valid_idx.device)], exp_idx[torch.randperm(exp_idx.numel(), device=exp_idx.device)]


def torch_minibatch(valid_sh, exp_sh, first, M, critic_cols, actor_cols):
    """ppo_agent.py:186-196 for one minibatch: positions first .. first + M of the two shuffled lists (np.mod wrap), one index_select per column"""
    pos = torch.arange(first, first + M, device=valid_sh.device)
    c_rows, a_rows = valid_sh[pos % valid_sh.numel()], exp_sh[pos % exp_sh.numel()]
    return [x.reshape((-1,) + x.shape[2:]).index_select(0, c_rows) for x in critic_cols], [x.reshape((-1,) + x.shape[2:]).index_select(0, a_rows) for x in actor_cols]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32); ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--S", type=int, default=227); ap.add_argument("--A", type=int, default=28); ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_batch_bench.json"))
    a = ap.parse_args()
    T, N, S, A, M = a.T, a.N, a.S, a.A, a.M
    if not torch.cuda.is_available():
        raise SystemExit("ppo_batch_bench needs a GPU (deepmimic_amd has no CPU path)")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    f = lambda *s: torch.randn(s, generator=g, dtype=torch.float32, device="cuda")
    u = lambda *s: torch.rand(s, generator=g, dtype=torch.float32, device="cuda")
    ret, values, obs, act, logp = f(T, N), f(T + 1, N), f(T, N, S), f(T, N, A), f(T, N)
    mask = (u(T, N) >= 0.2).int(); flags = (u(T, N) >= 0.3).int()
    eps, clip, vmin, vmax = 1e-5, 5.0, -2.0, 2.0

    kb = ppo_batch.advantages_torch(ret, values, mask, flags, eps, clip, vmin, vmax)
    t_adv, t_tar, t_valid, t_exp, t_stats = torch_advantages(ret, values, mask, flags, eps, clip, vmin, vmax)
    n_valid, n_exp = kb.counts_host()
    first = n_valid - M // 2 if n_valid > M else 0           # a minibatch that runs over the end of the pass: both sides wrap
    ks = kb.stats.cpu().numpy(); ts = t_stats.cpu().numpy()
    c_k = kb.gather("valid", first, M, 7, 0, obs, kb.targets, picked=True); a_k = kb.gather("exp", first, M, 7, 0, obs, act, logp, kb.adv, picked=True)
    agree = dict(lists_equal=bool(n_valid == t_valid.numel() and n_exp == t_exp.numel() and (kb.valid_idx[:n_valid] == t_valid).all() and (kb.exp_idx[:n_exp] == t_exp).all()),
                 adv_max_abs_diff=float((kb.adv.double() - t_adv.double()).abs().max()), targets_equal=bool((kb.targets == t_tar).all()),
                 mean_rel_diff=float(abs(ks[0] - ts[0]) / abs(ts[0])), std_rel_diff=float(abs(ks[1] - ts[1]) / ts[1]),
                 gathered_rows_are_the_picked_rows=bool((c_k[0] == obs.reshape(T * N, S)[c_k[2].long()]).all() and (a_k[3] == kb.adv.reshape(-1)[a_k[4].long()]).all()
                                                        and (mask.reshape(-1)[c_k[2].long()] != 0).all() and (flags.reshape(-1)[a_k[4].long()] != 0).all()))
    v_sh, e_sh = torch_shuffle(t_valid, t_exp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3          # us
    runs = dict(
        advantages_kernels=lambda: ppo_batch.advantages_torch(ret, values, mask, flags, eps, clip, vmin, vmax),
        advantages_torch_ops=lambda: torch_advantages(ret, values, mask, flags, eps, clip, vmin, vmax),
        minibatch_kernels=lambda: (kb.gather("valid", first, M, 7, 0, obs, kb.targets), kb.gather("exp", first, M, 7, 0, obs, act, logp, kb.adv)),
        minibatch_torch_ops=lambda: torch_minibatch(v_sh, e_sh, first, M, [obs, t_tar], [obs, act, logp, t_adv]),
        shuffle_torch_ops_per_epoch=lambda: torch_shuffle(t_valid, t_exp))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    q = lambda x: [float(np.percentile(x, p)) for p in (25, 50, 75)]
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = M * 4 * (2 * (2 * S + A + 3) + 2)      # per position: obs twice, actions, logp, adv, targets read and written, and the two index reads
    out = dict(what="PPO batch stage: hand-written kernels vs the same stage in public torch ops, interleaved in one process, HIP events, microseconds (every time includes "
                    "the allocation of the outputs and the Python / ctypes launch path; the torch advantages include the host waits of nonzero())",
               T=T, N=N, S=S, A=A, minibatch=M, n_valid=n_valid, n_exp=n_exp, first=first, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               us_q25_median_q75={k: q(v) for k, v in times.items()},
               torch_over_kernels=dict(advantages=med["advantages_torch_ops"] / med["advantages_kernels"], minibatch=med["minibatch_torch_ops"] / med["minibatch_kernels"]),
               minibatch_bytes_moved=nbytes, minibatch_kernels_bytes_per_s=nbytes / (med["minibatch_kernels"] * 1e-6), agreement=agree)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
