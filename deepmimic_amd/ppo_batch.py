"""PPO training batches from a device-resident rollout (libdm_hip.so `dm_ppo_advantages` / `dm_ppo_gather`, deepmimic_amd/csrc/dm_ppo_batch.h): what the
reference's PPOAgent._train_step (learning/ppo_agent.py:141-232) does between the returns and the first optimiser step, on arrays that never left HBM.
Everything is time-major [T, N] and addressed by the flat index i = t * N + n:

    returns, mask     what `returns.td_lambda_returns_torch` handed out (mask None: every sample valid)
    values            the critic values the returns were computed from ([T + 1, N] is taken as it is: the first T rows are read)
    exp_flags         the EXP flags of `Policy.forward_device_ex` (None: every step explored)

Sample i is VALID where mask[i] != 0 and EXP where it is valid and exp_flags[i] != 0.  `advantages_torch` leaves on the device: the normalised, clipped advantage
(0 off the exp samples), the clipped critic targets, the ascending lists of the valid and the exp samples with their two counts, and the advantage's mean / std
(fp64, two passes, fixed summation order: bit-identical from run to run).  `PPOBatch.gather` then copies the rows of a shuffled pass over one of the lists in one
launch: position p of the pass reads idx[perm(p % count)] with a fresh keyed permutation for every wrap p // count and every epoch, so a list shorter than
the pass over it wraps as `np.mod(batch, num_idx)` does at ppo_agent.py:186-193.  The only host read is `PPOBatch.counts_host()`, once per iteration.
Losses, gradients and optimiser steps stay torch's.

`reference_advantages`, `reference_permutation` and `reference_gather_rows` are the numpy statements the tests hold the kernels to."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, u32, u64, vp
from .core import load_library
from .streams import philox4x32_10

MAX_COLUMNS = 8


class _Column(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int32)]


def workspace_bytes(T: int, N: int, lib_path: Optional[str] = None) -> int:
    """scratch bytes `advantages_device` needs at this shape (the caller allocates them, 8-byte aligned)"""
    lib = load_library(lib_path)
    n = lib.dm_ppo_workspace_bytes(int(T), int(N))
    check(lib, n < 0)
    return int(n)


def advantages_device(T: int, N: int, returns_ptr: int, values_ptr: int, mask_ptr: int, exp_flags_ptr: int, adv_eps: float, norm_adv_clip: float,
                      val_min: float, val_max: float, adv_ptr: int, targets_ptr: int, valid_idx_ptr: int, exp_idx_ptr: int, counts_ptr: int, stats_ptr: int,
                      workspace_ptr: int, workspace_nbytes: int, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints; mask_ptr and exp_flags_ptr may be 0), asynchronous on the HIP stream `stream` (0 = the null stream) of `device_id`."""
    lib = load_library(lib_path)
    check(lib, lib.dm_ppo_advantages(int(device_id), int(T), int(N), vp(returns_ptr), vp(values_ptr), vp(mask_ptr), vp(exp_flags_ptr), float(adv_eps),
                                      float(norm_adv_clip), float(val_min), float(val_max), vp(adv_ptr), vp(targets_ptr), vp(valid_idx_ptr), vp(exp_idx_ptr),
                                      vp(counts_ptr), vp(stats_ptr), vp(workspace_ptr), int(workspace_nbytes), vp(stream)))


def gather_device(idx_ptr: int, count_ptr: int, first: int, rows: int, seed: int, epoch: int, columns, picked_ptr: int = 0, stream: int = 0, device_id: int = 0,
                  lib_path: Optional[str] = None):
    """`columns`: a sequence of (src_ptr, dst_ptr, width) -- src a [T * N, width] array of 4-byte elements, dst [rows, width]; one launch for all of them."""
    lib = load_library(lib_path)
    columns = list(columns)
    cols = (_Column * max(1, len(columns)))()
    for c, (src, dst, width) in zip(cols, columns):
        c.src, c.dst, c.width = (int(src) or None), (int(dst) or None), int(width)
    check(lib, lib.dm_ppo_gather(int(device_id), vp(idx_ptr), vp(count_ptr), int(first), int(rows), u64(seed), u32(epoch), len(columns), C.cast(cols, C.c_void_p),
                                  vp(picked_ptr), vp(stream)))


class PPOBatch:
    """What `advantages_torch` left on the device: adv, targets [T, N] float32; valid_idx, exp_idx [T * N] int32 (meaningful up to their counts);
    counts int32[2] = (n_valid, n_exp); stats float64[2] = (mean, std) of returns - values over the exp samples."""

    def __init__(self, adv, targets, valid_idx, exp_idx, counts, stats, lib_path: Optional[str] = None):
        self.adv, self.targets, self.valid_idx, self.exp_idx, self.counts, self.stats = adv, targets, valid_idx, exp_idx, counts, stats
        self.T, self.N = int(adv.shape[0]), int(adv.shape[1])
        self.lib_path = lib_path
        self._counts_host = None

    def counts_host(self):
        """(n_valid, n_exp) on the host: the one call that synchronises (once; the result is kept)"""
        if self._counts_host is None:
            c = self.counts.cpu()
            self._counts_host = (int(c[0]), int(c[1]))
        return self._counts_host

    def gather(self, which: str, first: int, rows: int, seed: int, epoch: int, *columns, picked: bool = False):
        """Rows `first .. first + rows` of the shuffled pass over the "valid" or the "exp" list from every tensor of `columns` (contiguous float32 / int32, leading
        shape [T, N]) in one launch on torch's current stream: a list of [rows, ...] tensors, and the int32 [rows] source rows behind them if `picked`."""
        import torch
        if which not in ("valid", "exp"):
            raise ValueError('which must be "valid" or "exp"')
        if not 1 <= len(columns) <= MAX_COLUMNS:
            raise ValueError("1 to %d columns per call" % MAX_COLUMNS)
        if int(rows) < 1 or int(first) < 0:
            raise ValueError("rows must be >= 1 and first >= 0")
        dev = self.adv.device
        cols, outs = [], []
        for x in columns:
            if x.device != dev or x.dtype not in (torch.float32, torch.int32) or x.dim() < 2 or tuple(x.shape[:2]) != (self.T, self.N) or not x.is_contiguous():
                raise ValueError("a column must be a contiguous float32 / int32 tensor of leading shape [%d, %d] on %s" % (self.T, self.N, dev))
            width = int(math.prod(x.shape[2:]))
            if width < 1:
                raise ValueError("a column has no elements per row")
            out = torch.empty((int(rows),) + tuple(x.shape[2:]), dtype=x.dtype, device=dev)
            cols.append((x.data_ptr(), out.data_ptr(), width)); outs.append(out)
        src = torch.empty(int(rows), dtype=torch.int32, device=dev) if picked else None
        k = 0 if which == "valid" else 1
        gather_device((self.valid_idx, self.exp_idx)[k].data_ptr(), self.counts.data_ptr() + 4 * k, first, rows, seed, epoch, cols,
                      picked_ptr=src.data_ptr() if picked else 0, stream=stream_handle(dev), device_id=dev.index or 0,
                      lib_path=self.lib_path)
        return outs + [src] if picked else outs

    def minibatches(self, mini_batch_size: int, epochs: int, seed: int, critic_columns, actor_columns, picked: bool = False):
        """The double loop of ppo_agent.py:178-212: for every epoch, ceil(n_valid / mini_batch_size) batches; batch b takes positions b * M .. (b + 1) * M of the
        epoch's pass over the valid list for the critic and of its pass over the exp list for the actor.  Yields (epoch, b, critic tensors, actor tensors), each
        a list as `gather` returns it (`self.targets` / `self.adv` are columns like any other).  Reads the counts once; nothing if there is no valid sample, and
        no actor rows (None) if there is no exp sample."""
        M = int(mini_batch_size)
        if M < 1:
            raise ValueError("mini_batch_size must be >= 1")
        n_valid, n_exp = self.counts_host()
        for e in range(int(epochs)):
            for b in range(-(-n_valid // M)):
                critic = self.gather("valid", b * M, M, seed, e, *critic_columns, picked=picked)
                actor = self.gather("exp", b * M, M, seed, e, *actor_columns, picked=picked) if n_exp > 0 else None
                yield e, b, critic, actor


def advantages_torch(returns, values, mask=None, exp_flags=None, adv_eps: float = 1e-5, norm_adv_clip: float = 5.0, val_min: float = -math.inf,
                     val_max: float = math.inf, lib_path: Optional[str] = None) -> PPOBatch:
    """`dm_ppo_advantages` on torch tensors of one GPU, on torch's current stream.  returns [T, N] float32; values [T, N] or [T + 1, N] float32; mask, exp_flags
    [T, N] int32 or None.  Five short launches, no host synchronisation."""
    import torch
    if returns.dim() != 2:
        raise ValueError("returns must be [T, N]")
    T, N = int(returns.shape[0]), int(returns.shape[1])
    dev = returns.device
    if dev.type != "cuda":
        raise ValueError("advantages_torch needs GPU tensors (deepmimic_amd has no CPU path)")
    tensor_arg("returns", returns, dev, torch.float32, [(T, N)]); tensor_arg("values", values, dev, torch.float32, [(T, N), (T + 1, N)])
    if mask is not None:
        tensor_arg("mask", mask, dev, torch.int32, [(T, N)])
    if exp_flags is not None:
        tensor_arg("exp_flags", exp_flags, dev, torch.int32, [(T, N)])
    adv = torch.empty((T, N), dtype=torch.float32, device=dev); targets = torch.empty((T, N), dtype=torch.float32, device=dev)
    valid_idx = torch.empty(T * N, dtype=torch.int32, device=dev); exp_idx = torch.empty(T * N, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev); stats = torch.empty(2, dtype=torch.float64, device=dev)
    nbytes = workspace_bytes(T, N, lib_path)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    advantages_device(T, N, returns.data_ptr(), values.data_ptr(), mask.data_ptr() if mask is not None else 0,
                      exp_flags.data_ptr() if exp_flags is not None else 0, adv_eps, norm_adv_clip, val_min, val_max, adv.data_ptr(), targets.data_ptr(),
                      valid_idx.data_ptr(), exp_idx.data_ptr(), counts.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes,
                      stream=stream_handle(dev), device_id=dev.index or 0, lib_path=lib_path)
    return PPOBatch(adv, targets, valid_idx, exp_idx, counts, stats, lib_path=lib_path)


# ---- numpy statements of the above (host; the tests hold the kernels to them)

def reference_advantages(returns, values, mask=None, exp_flags=None, adv_eps=1e-5, norm_adv_clip=5.0, val_min=-np.inf, val_max=np.inf):
    """float64 throughout: dict(adv, targets [T, N] float64 -- the kernel stores their float32 roundings --, valid_idx, exp_idx, counts, stats (mean, std))"""
    ret = np.asarray(returns, np.float32); T, N = ret.shape
    r = ret.astype(np.float64).reshape(-1)
    v = np.asarray(values, np.float32)[:T].astype(np.float64).reshape(-1)
    valid = np.ones(T * N, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    exp = valid if exp_flags is None else valid & (np.asarray(exp_flags).reshape(-1) != 0)
    a = r - v
    mean, std = (float(np.mean(a[exp])), float(np.std(a[exp]))) if exp.any() else (0.0, 0.0)
    adv = np.zeros(T * N)
    adv[exp] = np.clip((a[exp] - mean) / (std + adv_eps), -norm_adv_clip, norm_adv_clip)
    return dict(adv=adv.reshape(T, N), targets=np.clip(r, val_min, val_max).reshape(T, N), valid_idx=np.flatnonzero(valid).astype(np.int32),
                exp_idx=np.flatnonzero(exp).astype(np.int32), counts=(int(valid.sum()), int(exp.sum())), stats=(mean, std))


def _feistel_rounds(x, h, m, key, epoch, pass_, rounds):
    L, R = x >> np.uint32(h), x & m
    for r in range(rounds):
        ctr = np.stack([R, np.full_like(R, r), np.full_like(R, epoch), np.full_like(R, pass_)], axis=-1)
        L, R = R, L ^ (philox4x32_10(ctr, key)[..., 0] & m)
    return (L << np.uint32(h)) | R


def reference_permutation(count: int, seed, epoch: int, pass_: int, rounds: int = 6):
    """perm(count, seed, epoch, pass) of include/dm_hip.h as an int64 array p with p[slot] = the permuted slot: a cycle-walking balanced Feistel network on
    Philox4x32-10.  `seed` may be an array of seeds: one row per seed.  (`rounds` is 6 in the kernel; the argument is there for the uniformity test's comparison.)"""
    count = int(count)
    seeds = np.atleast_1d(np.asarray(seed, dtype=np.uint64))
    k = max(1, (count - 1).bit_length()) if count > 0 else 1
    h = (k + 1) // 2
    m = np.uint32((1 << h) - 1)
    key = np.repeat(np.stack([seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)], axis=-1).astype(np.uint32), count, axis=0)      # one key per element
    epoch, pass_ = int(epoch) & 0xFFFFFFFF, int(pass_) & 0xFFFFFFFF
    y = np.tile(np.arange(count, dtype=np.uint32), seeds.size)
    todo = np.arange(y.size)
    while todo.size:
        y[todo] = _feistel_rounds(y[todo], h, m, key[todo], epoch, pass_, rounds)
        todo = todo[y[todo] >= count]
    y = y.astype(np.int64).reshape(seeds.size, count)
    return y if np.ndim(seed) else y[0]


def reference_gather_rows(idx, count: int, first: int, rows: int, seed: int, epoch: int):
    """the source rows `dm_ppo_gather` picks for positions first .. first + rows of the pass over idx[:count] (int32 [rows]; all -1 when count == 0)"""
    count = int(count)
    if count == 0:
        return np.full(int(rows), -1, np.int32)
    idx = np.asarray(idx)
    pos = int(first) + np.arange(int(rows), dtype=np.int64)
    out = np.empty(int(rows), np.int32)
    for p in np.unique(pos // count):
        sel = pos // count == p
        out[sel] = idx[reference_permutation(count, seed, epoch, int(p))[pos[sel] % count]]
    return out
