"""Episode returns, lengths and end-cause totals over a device-resident rollout (libdm_hip.so `dm_episode_stats`, deepmimic_amd/csrc/dm_episode.h): what the
reference's learner logs as Train_Return / Test_Return -- path.calc_return() of the finished, valid paths (learning/path.py:45-46, learning/rl_agent.py:351-365,
456-466; a path with a non-finite value is never stored, learning/replay_buffer.py:102-112) -- together with episode lengths and the share of falls, without a
device-to-host copy per step.  Everything is time-major, row t = step t of the N envs, the way a sampler stacks the outputs of `TorchVecEnv.step`:

    rewards [T, N] float32; terminate, done, valid [T, N] int32 (info["terminate"], the `done` of step t, info["valid"]; valid None: every episode valid)

Per env column, forward in time, on a carry (acc_return float64 [N], acc_len int32 [N]) the caller keeps between calls: the reward is added in fp64 and the length
counted; ep_return[t] / ep_len[t] are the running return (rounded once to fp32) and length of the episode step t belongs to, the finished episode's where done[t]
is set.  A finished episode has class 3 (INVALID: valid == 0, or a non-finite return), else 1 (FAIL) / 2 (SUCC) by `terminate`, else 0 (NULL: episode timer, clip
end), and goes into a totals block of 25 eight-byte words (BLOCK layout below, include/dm_hip.h DM_EP_*) and, for classes 0 .. 2, into a histogram of lengths.
T = 1 is the per-step use (`TorchVecEnv(episode_stats=True)`), T = the rollout length the per-iteration use.

`reference_episode_stats` is the same recursion in numpy float64 with `math.fsum` totals: the statement the tests hold the kernel to."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, vp
from .core import load_library

NULL, FAIL, SUCC, INVALID = 0, 1, 2, 3
CLASS_NAMES = ("null", "fail", "succ", "invalid")
# the totals block: int64 words EPISODES + c, STEPS + c, LEN_MAX + c (c in 0 .. 3) and STEPS_SEEN; float64 words RET_SUM + c, RET_SQ + c, RET_MIN + c, RET_MAX + c (c in 0 .. 2)
EPISODES, STEPS, LEN_MAX, RET_SUM, RET_SQ, RET_MIN, RET_MAX, STEPS_SEEN, TOTALS_WORDS = 0, 4, 8, 12, 15, 18, 21, 24, 25


def initial_block(bins: int = 0) -> np.ndarray:
    """the block a window starts from, as int64[25 + bins] (the histogram behind the totals): zeros, ret_min = +inf, ret_max = -inf"""
    b = np.zeros(TOTALS_WORDS + int(bins), np.int64)
    f = b.view(np.float64)
    f[RET_MIN:RET_MIN + 3], f[RET_MAX:RET_MAX + 3] = np.inf, -np.inf
    return b


def merge_blocks(blocks) -> np.ndarray:
    """raw blocks (int64[25 + bins], of env groups or ranks) added in list order: counts, steps, sums and the histogram add; len_max, ret_min, ret_max fold"""
    blocks = [np.asarray(b, np.int64) for b in blocks]
    if not blocks or any(b.shape != blocks[0].shape or b.ndim != 1 or b.size < TOTALS_WORDS for b in blocks):
        raise ValueError("merge needs a non-empty list of int64 blocks of one length >= %d" % TOTALS_WORDS)
    out = blocks[0].copy()
    of = out.view(np.float64)
    for b in blocks[1:]:
        bf = b.view(np.float64)
        out[EPISODES:LEN_MAX] += b[EPISODES:LEN_MAX]
        out[LEN_MAX:RET_SUM] = np.maximum(out[LEN_MAX:RET_SUM], b[LEN_MAX:RET_SUM])
        of[RET_SUM:RET_MIN] += bf[RET_SUM:RET_MIN]
        of[RET_MIN:RET_MAX] = np.minimum(of[RET_MIN:RET_MAX], bf[RET_MIN:RET_MAX])
        of[RET_MAX:STEPS_SEEN] = np.maximum(of[RET_MAX:STEPS_SEEN], bf[RET_MAX:STEPS_SEEN])
        out[STEPS_SEEN:] += b[STEPS_SEEN:]
    return out


def _figures(n, steps, len_max, s, sq, lo, hi):
    n, steps = int(n), int(steps)
    d = {"episodes": n, "steps": steps, "mean_length": steps / n if n else float("nan"), "max_length": int(len_max)}
    if s is not None:
        s, sq = float(s), float(sq)
        mean = s / n if n else float("nan")
        d.update(mean_return=mean, std_return=math.sqrt(max(sq / n - mean * mean, 0.0)) if n else float("nan"),
                 min_return=float(lo) if n else float("nan"), max_return=float(hi) if n else float("nan"))
    return d


def decode_block(block, bin_steps: int = 1) -> dict:
    """a raw block as figures: per class under its name (invalid: counts and lengths only), the same over the finished valid episodes (classes 0 .. 2) at the top
    level, fall_share = episodes[FAIL] / episodes[0 .. 2], invalid_share = episodes[INVALID] / all, steps_seen, the histogram and the raw block"""
    b = np.asarray(block, np.int64)
    f = b.view(np.float64)
    out = {}
    for c, name in enumerate(CLASS_NAMES):
        ret = (f[RET_SUM + c], f[RET_SQ + c], f[RET_MIN + c], f[RET_MAX + c]) if c < 3 else (None,) * 4
        out[name] = _figures(b[EPISODES + c], b[STEPS + c], b[LEN_MAX + c], *ret)
    n = int(b[EPISODES:EPISODES + 3].sum())
    out.update(_figures(n, b[STEPS:STEPS + 3].sum(), b[LEN_MAX:LEN_MAX + 3].max(), math.fsum(f[RET_SUM:RET_SUM + 3]), math.fsum(f[RET_SQ:RET_SQ + 3]),
                        f[RET_MIN:RET_MIN + 3].min(), f[RET_MAX:RET_MAX + 3].max()))
    total = n + int(b[EPISODES + INVALID])
    out.update(fall_share=int(b[EPISODES + FAIL]) / n if n else float("nan"), invalid_share=int(b[EPISODES + INVALID]) / total if total else float("nan"),
               steps_seen=int(b[STEPS_SEEN]), histogram=b[TOTALS_WORDS:].copy(), bin_steps=int(bin_steps), block=b.copy())
    return out


def workspace_bytes(N: int, lib_path: Optional[str] = None) -> int:
    """scratch bytes `episode_stats_device` needs for N envs when totals or a histogram are asked for (the caller allocates them, 8-byte aligned)"""
    lib = load_library(lib_path)
    n = lib.dm_episode_workspace_bytes(int(N))
    check(lib, n < 0)
    return int(n)


def episode_stats_device(T: int, N: int, rewards_ptr: int, terminate_ptr: int, done_ptr: int, valid_ptr: int, acc_return_ptr: int, acc_len_ptr: int,
                         ep_return_ptr: int = 0, ep_len_ptr: int = 0, totals_ptr: int = 0, hist_ptr: int = 0, bins: int = 0, bin_steps: int = 1,
                         work_ptr: int = 0, work_nbytes: int = 0, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints; valid, ep_return, ep_len, totals, hist and -- without totals and hist -- work may be 0), asynchronous on the HIP stream `stream`
    (0 = the null stream) of `device_id`."""
    lib = load_library(lib_path)
    check(lib, lib.dm_episode_stats(int(device_id), int(T), int(N), vp(rewards_ptr), vp(terminate_ptr), vp(done_ptr), vp(valid_ptr), vp(acc_return_ptr), vp(acc_len_ptr),
                                     vp(ep_return_ptr), vp(ep_len_ptr), vp(totals_ptr), vp(hist_ptr), int(bins), int(bin_steps), vp(work_ptr), int(work_nbytes), vp(stream)))


class EpisodeStats:
    """The carry, totals, histogram and workspace of `n` envs as torch tensors on one GPU.  `update` is asynchronous on torch's current stream and reads nothing
    back; `totals` is the one host read.  bins = 0: no histogram.  `carry`: (acc_return float64 [n], acc_len int32 [n]) views to work on instead of tensors of its
    own -- an env group's rows of whole-batch carries."""

    def __init__(self, n: int, device="cuda:0", bins: int = 0, bin_steps: int = 1, lib_path: Optional[str] = None, carry=None):
        import torch
        self.torch = torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("EpisodeStats needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if int(n) < 1 or int(bins) < 0 or int(bin_steps) < 1:
            raise ValueError("n >= 1, bins >= 0 and bin_steps >= 1")
        self.n, self.device, self.bins, self.bin_steps, self.lib_path = int(n), dev, int(bins), int(bin_steps), lib_path
        if carry is None:
            carry = (torch.zeros(self.n, dtype=torch.float64, device=dev), torch.zeros(self.n, dtype=torch.int32, device=dev))
        self.acc_return = tensor_arg("carry[0]", carry[0], dev, torch.float64, [(self.n,)])
        self.acc_len = tensor_arg("carry[1]", carry[1], dev, torch.int32, [(self.n,)])
        self._initial = torch.from_numpy(initial_block(self.bins)).to(dev)
        self.block = self._initial.clone()                                            # int64[25 + bins]: the totals, the histogram behind them
        self._work_nbytes = workspace_bytes(self.n, lib_path)
        self._work = torch.zeros(self._work_nbytes // 8, dtype=torch.int64, device=dev)

    def update(self, rewards, terminate, done, valid=None, per_step: bool = True, out=None):
        """One window: rewards float32, terminate / valid int32, done bool or int32, all [N] (one step) or [T, N], contiguous, on this device.  Returns
        (ep_return float32, ep_len int32) of the inputs' shape -- written into `out` = (ep_return, ep_len) if given -- or None with per_step off."""
        t = self.torch
        dev = self.device
        one = isinstance(rewards, t.Tensor) and rewards.dim() == 1
        shape = (self.n,) if one else (int(rewards.shape[0]) if isinstance(rewards, t.Tensor) and rewards.dim() == 2 else 0, self.n)
        T = 1 if one else shape[0]
        tensor_arg("rewards", rewards, dev, t.float32, [shape])
        tensor_arg("terminate", terminate, dev, t.int32, [shape])
        if isinstance(done, t.Tensor) and done.dtype == t.bool:
            done = done.to(t.int32)
        tensor_arg("done", done, dev, t.int32, [shape])
        if valid is not None:
            tensor_arg("valid", valid, dev, t.int32, [shape])
        ret = length = None
        if per_step:
            ret, length = out if out is not None else (t.empty(shape, dtype=t.float32, device=dev), t.empty(shape, dtype=t.int32, device=dev))
            tensor_arg("out[0]", ret, dev, t.float32, [shape]); tensor_arg("out[1]", length, dev, t.int32, [shape])
        episode_stats_device(T, self.n, rewards.data_ptr(), terminate.data_ptr(), done.data_ptr(), valid.data_ptr() if valid is not None else 0,
                             self.acc_return.data_ptr(), self.acc_len.data_ptr(), ret.data_ptr() if per_step else 0, length.data_ptr() if per_step else 0,
                             totals_ptr=self.block.data_ptr(), hist_ptr=self.block.data_ptr() + 8 * TOTALS_WORDS if self.bins else 0, bins=self.bins,
                             bin_steps=self.bin_steps, work_ptr=self._work.data_ptr(), work_nbytes=self._work_nbytes, stream=stream_handle(dev),
                             device_id=dev.index, lib_path=self.lib_path)
        return (ret, length) if per_step else None

    def clear_totals(self):
        """start a new window: the initial block over totals and histogram, a device-to-device copy on the current stream"""
        self.block.copy_(self._initial)

    def reset_carry(self, rows=None):
        """drop the episodes in flight (of `rows`: an index tensor or slice; None: all) without counting them"""
        if rows is None:
            self.acc_return.zero_(); self.acc_len.zero_()
        else:
            self.acc_return[rows] = 0; self.acc_len[rows] = 0

    def raw(self) -> np.ndarray:
        """the raw block int64[25 + bins] on the host: one device-to-host copy (synchronises the current stream)"""
        return self.block.cpu().numpy()

    def totals(self) -> dict:
        """`decode_block` of the block: one device-to-host copy"""
        return decode_block(self.raw(), self.bin_steps)

    merge = staticmethod(merge_blocks)


def reference_episode_stats(rewards, terminate, done, valid, acc_return, acc_len, bins: int = 0, bin_steps: int = 1) -> dict:
    """The recursion of include/dm_hip.h dm_episode_stats in numpy float64 on host arrays ([T, N]; valid None: all valid; acc_return / acc_len [N]: the carry on
    entry, not modified).  Returns ep_return float32 [T, N], ep_len int32 [T, N], the carry behind the window (acc_return, acc_len), `block`: the window's raw
    block from the initial one with every fp64 total taken by math.fsum, and `returns` / `squares`: per class 0 .. 2 the lists of terms behind ret_sum / ret_sq."""
    r = np.asarray(rewards, np.float32).astype(np.float64)
    T, N = r.shape
    term, dn = np.asarray(terminate), np.asarray(done)
    vl = np.ones((T, N), np.int32) if valid is None else np.asarray(valid)
    acc, ln = np.array(acc_return, np.float64), np.array(acc_len, np.int32)
    ep_return, ep_len = np.zeros((T, N), np.float32), np.zeros((T, N), np.int32)
    block = initial_block(bins)
    rets, sqs = [[], [], []], [[], [], []]
    with np.errstate(all="ignore"):
        for t in range(T):
            acc = acc + r[t]
            ln = ln + np.int32(1)
            ep_return[t], ep_len[t] = acc.astype(np.float32), ln
            for n in np.flatnonzero(dn[t] != 0):
                a, L = float(acc[n]), int(ln[n])
                c = INVALID if (vl[t, n] == 0 or not math.isfinite(a)) else (int(term[t, n]) if term[t, n] in (FAIL, SUCC) else NULL)
                block[EPISODES + c] += 1; block[STEPS + c] += L; block[LEN_MAX + c] = max(block[LEN_MAX + c], L)
                if c < INVALID:
                    rets[c].append(a); sqs[c].append(a * a)
                    if bins:
                        block[TOTALS_WORDS + min(max((L - 1) // bin_steps, 0), bins - 1)] += 1
                acc[n], ln[n] = 0.0, 0
    f = block.view(np.float64)
    for c in range(3):
        f[RET_SUM + c], f[RET_SQ + c] = math.fsum(rets[c]), math.fsum(sqs[c])
        if rets[c]:
            f[RET_MIN + c], f[RET_MAX + c] = min(rets[c]), max(rets[c])
    block[STEPS_SEEN] = T * N
    return dict(ep_return=ep_return, ep_len=ep_len, acc_return=acc, acc_len=ln, block=block, returns=rets, squares=sqs)
