"""Replay stores for the AMP discriminator's data on the device (libdm_hip.so `dm_replay_append` / `dm_replay_sample`, deepmimic_amd/csrc/dm_replay.h): the two
`ReplayBufferRandStorage` buffers of the reference's AMPAgent (learning/amp_agent.py:70-77, 216-227; learning/replay_buffer_rand_storage.py) on arrays that never
leave HBM.  A store is `buf [capacity, width]` of 4-byte elements and `state`, an int64[2] = (size, total), both the caller's; the library keeps nothing.

    append    free slots first, then distinct random old slots; a list longer than the store keeps a uniformly chosen subset.  The list is `idx[:count]` with the
              count read ON THE DEVICE -- `PPOBatch.valid_idx` / `PPOBatch.counts[0:1]` plug in without a host read -- and `packed` receives the same rows dense
              and in list order: what `DeviceNormalizer.record_device` takes, with the count the caller already has from `PPOBatch.counts_host()`.
    sample    with replacement, one Philox draw per row.

Slots are a function of (state, seed, call, list position) alone: no atomics, the same sequence of calls gives the same bytes.  `DeviceReplayStore.state_host()`
is the only call that synchronises.  `reference_append_slots` and `reference_sample_slots` are the numpy statements the tests hold the kernels to."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .binding import check, stream_handle, u32, u64, vp
from .core import load_library
from .ppo_batch import reference_permutation
from .streams import philox4x32_10

PASS_VICTIM, PASS_INCOMING, CTR_SAMPLE = 0x564943, 0x494E43, 0x534D50          # dm_replay.h kPassVictim, kPassIncoming, kCtrSample

def append_device(buf_ptr: int, capacity: int, width: int, state_ptr: int, src_ptr: int, idx_ptr: int, count_ptr: int, max_rows: int, seed: int, call: int,
                  packed_ptr: int = 0, slots_ptr: int = 0, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints; idx_ptr, count_ptr, packed_ptr and slots_ptr may be 0), asynchronous on the HIP stream `stream` (0 = the null stream) of `device_id`."""
    lib = load_library(lib_path)
    check(lib, lib.dm_replay_append(int(device_id), vp(buf_ptr), int(capacity), int(width), vp(state_ptr), vp(src_ptr), vp(idx_ptr), vp(count_ptr), int(max_rows),
                                     u64(seed), u32(call), vp(packed_ptr), vp(slots_ptr), vp(stream)))


def sample_device(buf_ptr: int, width: int, state_ptr: int, rows: int, seed: int, call: int, dst_ptr: int, picked_ptr: int = 0, stream: int = 0, device_id: int = 0,
                  lib_path: Optional[str] = None):
    lib = load_library(lib_path)
    check(lib, lib.dm_replay_sample(int(device_id), vp(buf_ptr), int(width), vp(state_ptr), int(rows), u64(seed), u32(call), vp(dst_ptr), vp(picked_ptr), vp(stream)))


class DeviceReplayStore:
    """`buf [capacity, *row_shape]` and `state` int64[2] on `device`, and a call counter for each of append and sample (the `call` the slots are keyed by: every
    append sees fresh victims, every sample fresh draws).  `width` is the row's shape, an int or a tuple."""

    def __init__(self, capacity: int, width, device="cuda:0", seed: int = 0, dtype=None, lib_path: Optional[str] = None):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceReplayStore needs a GPU device (deepmimic_amd has no CPU path)")
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.int32):
            raise ValueError("a store holds float32 or int32 rows")
        self.row_shape = (int(width),) if np.ndim(width) == 0 else tuple(int(w) for w in width)
        self.capacity, self.width = int(capacity), int(math.prod(self.row_shape))
        if self.capacity < 1 or self.width < 1:
            raise ValueError("capacity and width must be >= 1")
        self.seed, self.lib_path = int(seed), lib_path
        self.buf = torch.zeros((self.capacity,) + self.row_shape, dtype=self.dtype, device=self.device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.append_calls = self.sample_calls = 0

    def append(self, src, idx=None, count=None, max_rows=None, packed=None, slots: bool = False):
        """Rows of `src` (contiguous, leading shape [T, N] or [rows]) go into the store on torch's current stream.  idx: int32 list of source rows (None: row j = j);
        count: int32 tensor of one element on the device, the length of the list (None: max_rows); max_rows: the most rows the call can take (None: len(idx), or
        every row of src).  packed: a [max_rows, ...] tensor that receives the list's rows dense and in order.  Returns the int32 [max_rows] slots if `slots`."""
        t = self.torch
        lead = src.dim() - len(self.row_shape)
        if (src.device != self.device or src.dtype != self.dtype or not src.is_contiguous() or lead not in (1, 2) or tuple(src.shape[lead:]) != self.row_shape):
            raise ValueError("src must be a contiguous %s tensor of shape [T, N, ...] or [rows, ...] with rows of shape %s on %s" % (self.dtype, self.row_shape, self.device))
        total = int(math.prod(src.shape[:lead]))
        if idx is not None and (idx.device != self.device or idx.dtype != t.int32 or idx.dim() != 1 or not idx.is_contiguous()):
            raise ValueError("idx must be a contiguous int32 vector on %s" % self.device)
        if count is not None and (count.device != self.device or count.dtype != t.int32 or count.numel() != 1):
            raise ValueError("count must be an int32 tensor of one element on %s" % self.device)
        if max_rows is None:
            max_rows = int(idx.numel()) if idx is not None else total
        max_rows = int(max_rows)
        if max_rows < 1 or (idx is not None and max_rows > idx.numel()) or (idx is None and max_rows > total):
            raise ValueError("max_rows must be in [1, the rows the list / src has]")
        if packed is not None and (packed.device != self.device or packed.dtype != self.dtype or not packed.is_contiguous() or packed.numel() < max_rows * self.width):
            raise ValueError("packed must be a contiguous %s tensor of at least [max_rows, width] on %s" % (self.dtype, self.device))
        out = t.full((max_rows,), -1, dtype=t.int32, device=self.device) if slots else None
        append_device(self.buf.data_ptr(), self.capacity, self.width, self.state.data_ptr(), src.data_ptr(), idx.data_ptr() if idx is not None else 0,
                      count.data_ptr() if count is not None else 0, max_rows, self.seed, self.append_calls, packed_ptr=packed.data_ptr() if packed is not None else 0,
                      slots_ptr=out.data_ptr() if slots else 0, stream=stream_handle(self.device), device_id=self.device.index or 0, lib_path=self.lib_path)
        self.append_calls += 1
        return out

    def append_batch(self, src, ppo_batch, packed=None):
        """the valid samples of a `PPOBatch` (src of leading shape [T, N]): append over `valid_idx` / `counts[0:1]`, no host read"""
        if src.dim() < 2 or tuple(src.shape[:2]) != (ppo_batch.T, ppo_batch.N):
            raise ValueError("src must have the leading shape [%d, %d]" % (ppo_batch.T, ppo_batch.N))
        return self.append(src, idx=ppo_batch.valid_idx, count=ppo_batch.counts[0:1], max_rows=ppo_batch.T * ppo_batch.N, packed=packed)

    def sample(self, rows: int, out=None, picked: bool = False):
        """`rows` rows drawn with replacement, on torch's current stream: a [rows, ...] tensor (`out` if given), and the int32 [rows] slots behind it if `picked`.
        An empty store leaves the rows untouched (a fresh tensor is zeros) and picks -1."""
        t = self.torch
        rows = int(rows)
        if rows < 1:
            raise ValueError("rows must be >= 1")
        if out is None:
            out = t.zeros((rows,) + self.row_shape, dtype=self.dtype, device=self.device)
        elif out.device != self.device or out.dtype != self.dtype or not out.is_contiguous() or out.numel() != rows * self.width:
            raise ValueError("out must be a contiguous %s tensor of [rows, width] on %s" % (self.dtype, self.device))
        src = t.empty(rows, dtype=t.int32, device=self.device) if picked else None
        sample_device(self.buf.data_ptr(), self.width, self.state.data_ptr(), rows, self.seed, self.sample_calls, out.data_ptr(), picked_ptr=src.data_ptr() if picked else 0,
                      stream=stream_handle(self.device), device_id=self.device.index or 0, lib_path=self.lib_path)
        self.sample_calls += 1
        return (out, src) if picked else out

    def state_host(self):
        """(size, total) on the host: the one call that synchronises"""
        s = self.state.cpu()
        return int(s[0]), int(s[1])

    def clear(self):
        """an empty store (the rows keep their bytes; the call counters go on, so a refilled store does not repeat its draws)"""
        self.state.zero_()


# ---- numpy statements of the above (host; the tests hold the kernels to them)

def reference_append_slots(old_size: int, capacity: int, n: int, seed: int, call: int):
    """the slot `dm_replay_append` gives each of the n list rows of call `call` into a store that holds old_size of capacity rows (int32 [n]; -1: dropped)"""
    old, cap, n = int(old_size), int(capacity), int(n)
    free = cap - old
    q = np.arange(n, dtype=np.int64) if n <= cap else reference_permutation(n, seed, call, PASS_INCOMING)
    out = np.full(n, -1, np.int32)
    fresh = q < free
    out[fresh] = old + q[fresh]
    vict = (q >= free) & (q < cap)
    if vict.any():
        out[vict] = reference_permutation(old, seed, call, PASS_VICTIM)[q[vict] - free]
    return out


def reference_sample_slots(size: int, rows: int, seed, call: int):
    """the slots `dm_replay_sample` reads for its `rows` rows from a store of `size` rows (int32 [rows]; all -1 when size == 0).  `seed` may be an array of seeds:
    one row per seed."""
    size, rows = int(size), int(rows)
    seeds = np.atleast_1d(np.asarray(seed, dtype=np.uint64))
    if size == 0:
        out = np.full((seeds.size, rows), -1, np.int32)
        return out if np.ndim(seed) else out[0]
    ctr = np.zeros((seeds.size, rows, 4), np.uint32)
    ctr[..., 0] = np.arange(rows, dtype=np.uint32)[None, :]; ctr[..., 1] = int(call) & 0xFFFFFFFF; ctr[..., 2] = CTR_SAMPLE
    key = np.stack([seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)], axis=-1).astype(np.uint32)[:, None, :]
    w = philox4x32_10(ctr, key)[..., 0].astype(np.uint64)
    out = ((w * np.uint64(size)) >> np.uint64(32)).astype(np.int32)
    return out if np.ndim(seed) else out[0]
