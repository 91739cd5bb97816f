"""AMP batch rewards, reward statistics and the critic's value bounds over a device-resident rollout (libdm_hip.so `dm_amp_batch_rewards` / `dm_amp_value_clip`,
deepmimic_amd/csrc/dm_amp_rewards.h): what the reference's AMPAgent does between `_update_disc` and the returns -- `_batch_calc_reward` (learning/amp_agent.py:393-421),
`_lerp_reward` (:423-425) and the value clip of `_compute_batch_vals` (:436-443).  At train time the reference scores the WHOLE stored rollout with the discriminator
as it is after its update, logs Disc_Reward_Mean / Disc_Reward_Std over the scaled style reward, blends in the task reward and clips the critic's values to the
RUNNING extrema of the blended reward over 1 - discount.  Here the extrema live in a 2-element tensor on the device and the clip reads them there: no `.item()`, no
rebuilt `Critic(lo, hi)` per iteration.  Everything is time-major, row t = step t of the N envs, the way a sampler stacks the outputs of `TorchVecEnv.step`:

    logits [T, N] float32        the discriminator's y (`Discriminator.eval_torch(..., raw=True)[1]`)
    task_reward [T, N] float32   the env reward of step t, or None (style reward only)
    done, valid [T, N] int32     the `done` of step t, info["valid"] (valid None: every episode valid)

Per row, counted or not: d = 1 - y, s = max(0, 1 - d^2 / 4) * reward_scale, r = (1 - lerp) * s + lerp * task_r -- bit for bit the style head's output.  `mask` is the
mask of `returns.td_lambda_returns`: 0 for the steps of an episode that ended invalid inside the window.  Over the counted rows (mask 1): n, mean and population
standard deviation of s in fp64 (two passes, a fixed order), min and max of r; the running bounds take the min / max in.  A NaN r in a counted row makes the bounds NaN
and stays visible; rows that are not counted reach nothing.

`reference_batch_rewards` / `reference_value_clip` are the same arithmetic in numpy, sums in the kernel's order: the statement the tests hold the kernels to."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, vp
from .core import load_library

STAT_N, STAT_MEAN, STAT_STD, STAT_MIN, STAT_MAX, STATS_WORDS = 0, 1, 2, 3, 4, 5          # include/dm_hip.h DM_AMP_STAT_*
SCAN, FOLD = 64, 256         # dm_amp_rewards.h kScan / kFold: env columns per group partial, threads of the folding workgroup


def initial_bounds() -> np.ndarray:
    """{+inf, -inf}: reward_min / reward_max before the first rollout (learning/amp_agent.py:46-47)"""
    return np.array([np.inf, -np.inf], np.float32)


def workspace_bytes(T: int, N: int, lib_path: Optional[str] = None) -> int:
    """scratch bytes `batch_rewards_device` needs for a [T, N] rollout (the caller allocates them, 8-byte aligned)"""
    lib = load_library(lib_path)
    n = lib.dm_amp_batch_rewards_workspace(int(T), int(N))
    check(lib, n < 0)
    return int(n)


def batch_rewards_device(T: int, N: int, logits_ptr: int, task_reward_ptr: int, done_ptr: int, valid_ptr: int, reward_scale: float, task_reward_lerp: Optional[float],
                         rewards_ptr: int, mask_ptr: int, bounds_ptr: int, stats_ptr: int, work_ptr: int, work_nbytes: int, stream: int = 0, device_id: int = 0,
                         lib_path: Optional[str] = None):
    """Raw device pointers (ints; task_reward, valid -- then done too -- and mask may be 0), asynchronous on the HIP stream `stream` (0 = the null stream) of
    `device_id`.  task_reward_lerp None: the agent has no TaskRewardLerp (a task reward is then refused)."""
    lib = load_library(lib_path)
    lerp = float("nan") if task_reward_lerp is None else float(task_reward_lerp)
    check(lib, lib.dm_amp_batch_rewards(int(device_id), int(T), int(N), vp(logits_ptr), vp(task_reward_ptr), vp(done_ptr), vp(valid_ptr), float(reward_scale), lerp,
                                         vp(rewards_ptr), vp(mask_ptr), vp(bounds_ptr), vp(stats_ptr), vp(work_ptr), int(work_nbytes), vp(stream)))


def value_clip_device(n: int, values_ptr: int, bounds_ptr: int, discount: float, out_ptr: int, row_mask_ptr: int = 0, fill: float = 0.0, stream: int = 0,
                      device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints; row_mask may be 0, out may be values), asynchronous on the HIP stream `stream` of `device_id`."""
    lib = load_library(lib_path)
    check(lib, lib.dm_amp_value_clip(int(device_id), int(n), vp(values_ptr), vp(bounds_ptr), float(discount), vp(row_mask_ptr), float(fill), vp(out_ptr), vp(stream)))


class AmpRewards:
    """The running bounds, the statistics of the last rollout and the workspace as torch tensors on one GPU.  `bounds` (float32 [2] = reward_min, reward_max) is
    the state a checkpoint keeps (`torch.save(tracker.bounds)`, `tracker.bounds.copy_(...)`).  Every method but `state_host` is asynchronous on torch's current
    stream and reads nothing back.  reward_scale / task_reward_lerp: the agent's RewardScale / TaskRewardLerp (None: style reward only; a task reward passed to
    `update_torch` is then refused); discount: the agent's Discount."""

    def __init__(self, device="cuda:0", reward_scale: float = 1.0, task_reward_lerp: Optional[float] = None, discount: float = 0.95, lib_path: Optional[str] = None):
        import torch
        self.torch = torch
        dev = torch.device(device)
        if dev.type != "cuda" and not load_library(lib_path).dm_is_emulator():          # "cpu": the emulator build of the tests, where device memory is host memory
            raise ValueError("AmpRewards needs a GPU device (deepmimic_amd has no CPU path)")
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 0.0 <= float(discount) < 1.0:
            raise ValueError("discount must be in [0, 1)")
        self.device, self.lib_path = dev, lib_path
        self.reward_scale, self.task_reward_lerp, self.discount = float(reward_scale), None if task_reward_lerp is None else float(task_reward_lerp), float(discount)
        self.bounds = torch.from_numpy(initial_bounds()).to(dev)
        self.stats = torch.zeros(STATS_WORDS, dtype=torch.float64, device=dev)
        self._work, self._work_nbytes = None, 0

    def _where(self) -> dict:
        """the stream and device id of a call: torch's current stream on the GPU"""
        gpu = self.device.type == "cuda"
        return dict(stream=stream_handle(self.device) if gpu else 0, device_id=self.device.index if gpu else 0, lib_path=self.lib_path)

    def update_torch(self, logits, task_reward=None, done=None, valid=None):
        """One rollout: logits [T, N] float32, task_reward [T, N] float32 or None, done [T, N] bool or int32 (None only where valid is), valid [T, N] int32 or
        None.  Writes the statistics, takes the rollout's min / max into `bounds` and returns (rewards float32 [T, N], mask int32 [T, N])."""
        t, dev = self.torch, self.device
        if not isinstance(logits, t.Tensor) or logits.dim() != 2:
            raise ValueError("logits must be a [T, N] tensor")
        T, N = int(logits.shape[0]), int(logits.shape[1])
        if task_reward is not None and self.task_reward_lerp is None:
            raise ValueError("a task reward needs task_reward_lerp (the agent's TaskRewardLerp)")
        if isinstance(done, t.Tensor) and done.dtype == t.bool:
            done = done.to(t.int32)
        tensor_arg("logits", logits, dev, t.float32, [(T, N)])
        for name, x, dtype in (("task_reward", task_reward, t.float32), ("done", done, t.int32), ("valid", valid, t.int32)):
            if x is not None:
                tensor_arg(name, x, dev, dtype, [(T, N)])
        need = workspace_bytes(T, N, self.lib_path)
        if need > self._work_nbytes:          # grows with the widest rollout seen: allocated once for a sampler of one shape
            self._work, self._work_nbytes = t.zeros(need // 8, dtype=t.int64, device=dev), need
        rewards, mask = t.empty((T, N), dtype=t.float32, device=dev), t.empty((T, N), dtype=t.int32, device=dev)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        batch_rewards_device(T, N, logits.data_ptr(), ptr(task_reward), ptr(done), ptr(valid), self.reward_scale, self.task_reward_lerp, rewards.data_ptr(),
                             mask.data_ptr(), self.bounds.data_ptr(), self.stats.data_ptr(), self._work.data_ptr(), self._work_nbytes, **self._where())
        return rewards, mask

    def update_from_disc(self, disc, amp_obs, task_reward=None, done=None, valid=None):
        """The reference's order: after the discriminator's updates, score the stored rollout amp_obs [T, N, A] with `disc` (a `heads.Discriminator`) as it is
        now -- one `eval_torch(raw=True)` -- then `update_torch` on its logits."""
        _, logits = disc.eval_torch(amp_obs, raw=True)
        return self.update_torch(logits, task_reward, done, valid)

    def clip_torch(self, values, row_mask=None, fill: float = 0.0, out=None):
        """values (any shape, float32, contiguous) clipped to bounds / (1 - discount) as the value head clips to lo / hi; row_mask (the same shape, bool or int32): rows
        whose flag is 0 get `fill`.  Returns a new tensor, or `out` (which may be `values`)."""
        t, dev = self.torch, self.device
        if not isinstance(values, t.Tensor):
            raise ValueError("values must be a tensor")
        shape = tuple(values.shape)
        tensor_arg("values", values, dev, t.float32, [shape])
        if isinstance(row_mask, t.Tensor) and row_mask.dtype == t.bool:
            row_mask = row_mask.to(t.int32)
        if row_mask is not None:
            tensor_arg("row_mask", row_mask, dev, t.int32, [shape])
        out = t.empty_like(values) if out is None else tensor_arg("out", out, dev, t.float32, [shape])
        if values.numel():
            value_clip_device(values.numel(), values.data_ptr(), self.bounds.data_ptr(), self.discount, out.data_ptr(), 0 if row_mask is None else row_mask.data_ptr(),
                              fill, **self._where())
        return out

    def state_host(self) -> dict:
        """The one call that synchronises: reward_min / reward_max (the running bounds), val_min / val_max (the bounds over 1 - discount, as the clip rounds them),
        disc_reward_mean / disc_reward_std / n and cur_min / cur_max of the last rollout."""
        b = self.bounds.cpu().numpy(); s = self.stats.cpu().numpy()
        lo, hi = value_bounds(b, self.discount)
        return dict(reward_min=float(b[0]), reward_max=float(b[1]), val_min=float(lo), val_max=float(hi), disc_reward_mean=float(s[STAT_MEAN]),
                    disc_reward_std=float(s[STAT_STD]), n=int(s[STAT_N]), cur_min=float(s[STAT_MIN]), cur_max=float(s[STAT_MAX]))


def value_bounds(bounds, discount: float):
    """(lo, hi) as float32: (float)((double)bounds[k] / (1.0 - discount)), what dm_amp_value_clip clips to"""
    b = np.asarray(bounds, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = (b / (1.0 - float(discount))).astype(np.float32)
    return v[0], v[1]


def reference_mask(done, valid) -> np.ndarray:
    """the mask rule of dm_td_lambda_returns from the flags alone (done, valid [T, N])"""
    done, valid = np.asarray(done), np.asarray(valid)
    T, N = valid.shape
    mask = np.ones((T, N), np.int32)
    inv = np.zeros(N, bool)
    for t in reversed(range(T)):
        d = done[t] != 0
        inv = np.where(d, valid[t] == 0, inv)
        mask[t] = np.where(inv, 0, 1)
    return mask


def _nan_min(a, b):
    """dm_amp_rewards.h nan_min: (b < a || b != b) ? b : a -- np.minimum with the kernel's choice between equal values and between two NaNs"""
    with np.errstate(invalid="ignore"):
        return np.where((b < a) | (b != b), b, a)


def _nan_max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where((b > a) | (b != b), b, a)


def _tree(x: np.ndarray, op) -> np.ndarray:
    """x [G, W] folded along W by the kernels' tree: x[:, j] = op(x[:, j], x[:, j + w]) for j < w, w = W / 2 .. 1; returns [G]"""
    x = x.copy()
    w = x.shape[1] // 2
    while w >= 1:
        x[:, :w] = op(x[:, :w], x[:, w:2 * w])
        w //= 2
    return x[:, 0]


def _fold(col: np.ndarray, op, neutral):
    """per-column partials [N] -> one value in the kernels' order: groups of SCAN columns by the tree (columns past N neutral), the groups in contiguous runs of
    ceil(G / FOLD) per thread, each run in order from the neutral element, then the tree over FOLD"""
    N = col.shape[0]
    G = (N + SCAN - 1) // SCAN
    x = np.full(G * SCAN, neutral, col.dtype); x[:N] = col
    part = _tree(x.reshape(G, SCAN), op)
    per = (G + FOLD - 1) // FOLD
    y = np.full(FOLD * per, neutral, col.dtype); y[:G] = part
    y = y.reshape(FOLD, per)
    run = np.full(FOLD, neutral, col.dtype)
    for k in range(per):
        run = op(run, y[:, k])
    return _tree(run.reshape(1, FOLD), op)[0]


def reference_batch_rewards(logits, task_reward=None, done=None, valid=None, reward_scale: float = 1.0, task_reward_lerp: Optional[float] = None, bounds=None) -> dict:
    """dm_amp_batch_rewards in numpy on host arrays [T, N]: fp32 arithmetic with `train.fma32` at the head's rounding points, the fp64 sums in the kernel's documented
    order.  bounds: float32 [2] on entry (None: the initial {+inf, -inf}; not modified).  Returns rewards, style (s), mask, stats float64 [5], bounds float32 [2]."""
    from .train import fma32
    f32 = np.float32
    y = np.asarray(logits, f32)
    T, N = y.shape
    scale = f32(reward_scale)
    with np.errstate(all="ignore"):
        d = (f32(1.0) - y).astype(f32)
        s = (np.fmax(fma32((f32(-0.25) * d).astype(f32), d, f32(1.0)), f32(0.0)).astype(f32) * scale).astype(f32)
        if task_reward is not None:
            if task_reward_lerp is None:
                raise ValueError("a task reward needs task_reward_lerp")
            lerp = f32(task_reward_lerp)
            r = fma32(lerp, np.asarray(task_reward, f32), ((f32(1.0) - lerp).astype(f32) * s).astype(f32))
        else:
            r = s.copy()
        mask = reference_mask(done, valid) if valid is not None else np.ones((T, N), np.int32)
        counted = mask != 0
        # per column, t = T - 1 down to 0
        cnt = np.zeros(N, np.int64); col_sum = np.zeros(N, np.float64)
        mn = np.full(N, np.inf, f32); mx = np.full(N, -np.inf, f32)
        s64 = s.astype(np.float64)
        for t in reversed(range(T)):
            c = counted[t]
            col_sum = np.where(c, col_sum + s64[t], col_sum); cnt += c
            mn = np.where(c, _nan_min(mn, r[t]), mn); mx = np.where(c, _nan_max(mx, r[t]), mx)
        n = int(_fold(cnt, np.add, 0))
        total = _fold(col_sum, np.add, 0.0)
        cur_min, cur_max = _fold(mn, _nan_min, f32(np.inf)), _fold(mx, _nan_max, f32(-np.inf))
        mean = total / n if n > 0 else 0.0
        col_sq = np.zeros(N, np.float64)
        for t in reversed(range(T)):
            dev = s64[t] - mean
            col_sq = np.where(counted[t], col_sq + dev * dev, col_sq)
        std = float(np.sqrt(_fold(col_sq, np.add, 0.0) / n)) if n > 0 else 0.0
        b = initial_bounds() if bounds is None else np.array(bounds, f32)
        if n > 0:
            b = np.array([_nan_min(b[0], cur_min), _nan_max(b[1], cur_max)], f32)
    stats = np.array([n, mean, std, cur_min, cur_max], np.float64)
    return dict(rewards=r, style=s, mask=mask, stats=stats, bounds=b)


def reference_value_clip(values, bounds, discount: float, row_mask=None, fill: float = 0.0) -> np.ndarray:
    """dm_amp_value_clip in numpy: fminf(fmaxf(v, lo), hi) with lo / hi = `value_bounds`; np.fmax / np.fmin return their other operand for a NaN like fmaxf / fminf,
    so a NaN bound does not clip on its side and a NaN value comes out as lo"""
    lo, hi = value_bounds(bounds, discount)
    v = np.fmin(np.fmax(np.asarray(values, np.float32), lo), hi).astype(np.float32)
    return v if row_mask is None else np.where(np.asarray(row_mask) != 0, v, np.float32(fill)).astype(np.float32)
