"""Replay stores for the AMP discriminator's data on the device (deepmimic_amd/csrc/dm_replay.h, include/dm_hip.h dm_replay_append / dm_replay_sample,
deepmimic_amd/replay.py) against the numpy statements beside the binding.  Every case runs on the emulator library through host addresses and again, marked `gpu`,
through torch tensors.  Everything is exact: slots, states, every byte of the store, of the packed rows and of the sampled rows, and the guard rows around them.

Shapes are the ones the index arithmetic can break on: capacities 1, 2, 7, 64, 65, 300 with appends below, at and beyond the free space, at n == capacity (every old
row replaced, no incoming shuffle), at capacity + 1 (one row dropped, shuffled ranks) and several times the capacity; widths 1, 3, 4, 105, 108 (dword and 16-byte
copy paths with their tails) from bases on and 4 bytes past a 16-byte boundary; sample tiles of 1, 63, 64, 65 and 257 rows (4 rows per wavefront)."""
import os
import sys

import numpy as np
import pytest

from deepmimic_amd import ppo_batch as pb
from deepmimic_amd import replay as rp
from test_ppo_batch import Emu, Gpu, make_inputs, run_adv, same_bits

SENT = -77
CAPACITIES = [1, 2, 7, 64, 65, 300]
WIDTHS = (1, 3, 4, 105, 108)


def sequence(cap):
    """appends from a cleared store that cross every branch: a partial fill, free slots plus victims, n == capacity, capacity + 1, several times the capacity"""
    if cap == 300:
        return [100, 150, 120, 300, 301, 1000]
    if cap == 1:
        return [1, 1, 3]
    a = max(1, cap // 3)
    return [a, cap - a + max(1, cap // 4), cap, cap + 1, 3 * cap + 1]


def sent_of(dtype):
    return np.array(SENT, dtype).view(np.int32)


def rows_data(rng, n, w, dtype):
    return rng.standard_normal((n, w)).astype(np.float32) if dtype == np.float32 else rng.integers(-2 ** 31, 2 ** 31 - 1, size=(n, w)).astype(np.int32)


class Store:
    """a store on the backend with a guard row in front of and behind buf, and its numpy twin"""
    def __init__(self, be, cap, w, dtype=np.float32, off=0):
        self.be, self.cap, self.w, self.dtype = be, cap, w, dtype
        self.d_buf = be.put(np.full((cap + 2, w), SENT, dtype), off)
        self.d_state = be.put(np.zeros(2, np.int64))
        self.host = np.full((cap, w), SENT, dtype)
        self.size = self.total = 0

    buf_ptr = property(lambda self: self.be.ptr(self.d_buf) + 4 * self.w)
    state_ptr = property(lambda self: self.be.ptr(self.d_state))

    def set_state(self, size, total):
        self.d_state = self.be.put(np.array([size, total], np.int64)); self.size, self.total = size, total

    def check(self, tag):
        got = self.be.get(self.d_buf)
        assert (got[0].view(np.int32) == sent_of(self.dtype)).all() and (got[-1].view(np.int32) == sent_of(self.dtype)).all(), ("guard rows of buf", tag)
        assert same_bits(got[1:-1], self.host), ("buf", tag)
        assert tuple(self.be.get(self.d_state)) == (self.size, self.total), ("state", tag)


def append(be, st, src, idx, count, max_rows, seed, call, mode="list", offs=(0, 0)):
    """one dm_replay_append on the backend and on the numpy twin, with every check of the call.  mode: "list" idx and count; "no_idx" row j = j; "no_count" n = max_rows"""
    w, dtype = st.w, st.dtype
    d_src = be.put(src, offs[0])
    d_idx = None if mode == "no_idx" else be.put(np.asarray(idx, np.int32))
    d_count = None if mode == "no_count" else be.put(np.array([SENT, count, SENT], np.int32))
    d_packed = be.put(np.full((max_rows + 2, w), SENT, dtype), offs[1])
    d_slots = be.put(np.full(max_rows + 1, SENT, np.int32))
    rp.append_device(st.buf_ptr, st.cap, w, st.state_ptr, be.ptr(d_src), 0 if d_idx is None else be.ptr(d_idx), 0 if d_count is None else be.ptr(d_count) + 4, max_rows,
                     seed, call, packed_ptr=be.ptr(d_packed) + 4 * w, slots_ptr=be.ptr(d_slots), stream=be.stream, lib_path=be.lib)
    n = max_rows if mode == "no_count" else min(count, max_rows)
    rows = np.arange(n) if mode == "no_idx" else np.asarray(idx)[:n]
    want = rp.reference_append_slots(st.size, st.cap, n, seed, call)
    tag = (st.cap, w, mode, n, call)
    slots, packed = be.get(d_slots), be.get(d_packed)
    assert (slots[:n] == want).all(), ("slots", tag)
    assert (slots[n:] == SENT).all(), ("slots behind n", tag)
    kept = want >= 0
    assert len(set(want[kept].tolist())) == int(kept.sum()) == min(n, st.cap) and (want[kept] < st.cap).all(), ("distinct slots", tag)
    if n <= st.cap:                        # free slots first, in order; then old rows only
        fresh = min(n, st.cap - st.size)
        assert (want[:fresh] == st.size + np.arange(fresh)).all() and (want[fresh:] < st.size).all(), ("fresh then victims", tag)
    st.host[want[kept]] = src[rows[kept]]
    st.size, st.total = min(st.size + n, st.cap), st.total + n
    st.check(tag)
    assert same_bits(packed[1:1 + n], src[rows]), ("packed rows", tag)
    assert (packed[0].view(np.int32) == sent_of(dtype)).all() and (packed[1 + n:].view(np.int32) == sent_of(dtype)).all(), ("guard rows of packed_out", tag)
    return want


def check_append_sequence(be, cap):
    rng = np.random.default_rng([5, cap])
    for mode, w in (("list", 3), ("short", 3), ("no_idx", 2), ("no_count", 3)):
        st = Store(be, cap, w)
        for call, n in enumerate(sequence(cap)):
            total_rows = 2 * n + 9
            src = rows_data(rng, total_rows, w, np.float32)
            idx = np.sort(rng.choice(total_rows, size=n, replace=False)).astype(np.int32)
            idx_full = np.concatenate([idx, np.full(5, SENT, np.int32)])      # (what a PPOBatch list holds behind its count)
            if mode == "short":            # count_dev smaller than max_rows
                append(be, st, src, idx_full, n, n + 5, 11, call)
            elif mode == "no_idx":
                append(be, st, src, None, n, n + 5, 11, call, mode="no_idx")
            elif mode == "no_count":
                append(be, st, src, idx, None, n, 11, call, mode="no_count")
            else:
                append(be, st, src, idx, n, n, 11, call)
            # count_dev 0: nothing changes (and a count above max_rows is clamped: covered by "short" from the other side)
            append(be, st, src, idx_full, 0, n + 5, 11, call + 100)
        assert st.size == cap and st.total == sum(sequence(cap))
        if cap == 300:                     # the branches the sequence is there for
            assert sequence(cap)[2] == 120 and rp.reference_append_slots(250, 300, 120, 11, 2)[:50].tolist() == list(range(250, 300))
            assert (rp.reference_append_slots(300, 300, 301, 11, 4) == -1).sum() == 1 and (rp.reference_append_slots(300, 300, 1000, 11, 5) == -1).sum() == 700


def check_count_clamped(be):
    """a count above max_rows takes max_rows rows; a negative one none"""
    st = Store(be, 7, 3)
    src = rows_data(np.random.default_rng(3), 40, 3, np.float32)
    d_src, d_count = be.put(src), be.put(np.array([25, -4], np.int32))
    d_slots = be.put(np.full(11, SENT, np.int32))
    rp.append_device(st.buf_ptr, 7, 3, st.state_ptr, be.ptr(d_src), 0, be.ptr(d_count) + 4, 10, 2, 0, slots_ptr=be.ptr(d_slots), stream=be.stream, lib_path=be.lib)
    st.check("negative count")
    assert (be.get(d_slots) == SENT).all()
    rp.append_device(st.buf_ptr, 7, 3, st.state_ptr, be.ptr(d_src), 0, be.ptr(d_count), 10, 2, 1, slots_ptr=be.ptr(d_slots), stream=be.stream, lib_path=be.lib)
    want = rp.reference_append_slots(0, 7, 10, 2, 1)
    st.host[want[want >= 0]] = src[:10][want >= 0]; st.size, st.total = 7, 10
    st.check("count above max_rows")
    got = be.get(d_slots)
    assert (got[:10] == want).all() and got[10] == SENT


def run_sample(be, st, rows, seed, call, off=0, want_picked=True):
    d_dst = be.put(np.full((rows + 2, st.w), SENT, st.dtype), off)
    d_pick = be.put(np.full(rows + 1, SENT, np.int32))
    rp.sample_device(st.buf_ptr, st.w, st.state_ptr, rows, seed, call, be.ptr(d_dst) + 4 * st.w, picked_ptr=be.ptr(d_pick) if want_picked else 0, stream=be.stream,
                     lib_path=be.lib)
    dst, picked = be.get(d_dst), be.get(d_pick)
    assert (dst[0].view(np.int32) == sent_of(st.dtype)).all() and (dst[-1].view(np.int32) == sent_of(st.dtype)).all(), "guard rows of dst"
    assert picked[rows] == SENT
    return dst[1:-1], picked[:rows]


def check_sample_call(be, st, rows, seed, call, off=0):
    dst, picked = run_sample(be, st, rows, seed, call, off)
    want = rp.reference_sample_slots(st.size, rows, seed, call)
    assert (picked == want).all() and (want >= 0).all() and (want < st.size).all(), (st.size, rows, seed, call)
    assert same_bits(dst, st.host[want]), (st.size, rows, st.w, off)
    return picked


def check_widths_and_alignment(be, w, dtype):
    """both copy paths and their tails: append with free slots, victims and a shuffled over-full list, then a sample, from every mix of bases"""
    rng = np.random.default_rng([9, w])
    for o_src, o_buf, o_packed in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        st = Store(be, 40, w, dtype, off=o_buf)
        for call, n in enumerate((25, 30, 90)):
            src = rows_data(rng, n + 20, w, dtype)
            idx = np.sort(rng.choice(n + 20, size=n, replace=False)).astype(np.int32)
            append(be, st, src, idx, n, n, 21, call, offs=(o_src, o_packed))
        for off in (0, 1):
            check_sample_call(be, st, 65, 21, 0, off=off)


def check_from_ppo_batch(be, T, N):
    """append over valid_idx / counts as dm_ppo_advantages leaves them: the stored rows are exactly the masked rows of src"""
    r, v, m, f = make_inputs(T, N)
    out = run_adv(be, r, v, m, f)
    n_valid = int(out["counts"][0])
    assert 0 < n_valid < T * N and (out["valid_idx"][n_valid:] == -77).all()
    w = 5
    src = rows_data(np.random.default_rng([T, N]), T * N, w, np.float32)
    st = Store(be, T * N, w)
    d_src, d_idx, d_counts = be.put(src), be.put(out["valid_idx"]), be.put(out["counts"])
    d_packed = be.put(np.full((T * N, w), SENT, np.float32))
    rp.append_device(st.buf_ptr, st.cap, w, st.state_ptr, be.ptr(d_src), be.ptr(d_idx), be.ptr(d_counts), T * N, 1, 0, packed_ptr=be.ptr(d_packed), stream=be.stream,
                     lib_path=be.lib)
    valid = np.flatnonzero(m.reshape(-1) != 0)
    st.host[:n_valid] = src[valid]; st.size = st.total = n_valid
    st.check((T, N))
    packed = be.get(d_packed)
    assert same_bits(packed[:n_valid], src.reshape(-1, w)[out["valid_idx"][:n_valid]]) and (packed[n_valid:].view(np.int32) == sent_of(np.float32)).all()


def filled_store(be, size, w=3, cap=None):
    st = Store(be, cap or size, w)
    st.host[...] = rows_data(np.random.default_rng([4, size]), st.cap, w, np.float32)
    st.d_buf = be.put(np.concatenate([np.full((1, w), SENT, np.float32), st.host, np.full((1, w), SENT, np.float32)]))
    st.set_state(size, size + 3)
    return st


def check_sample(be, size):
    st = filled_store(be, size, cap=size + 2)          # (two rows of the buffer beyond the store's size: never read)
    for rows in (1, 63, 64, 65, 257):
        a = check_sample_call(be, st, rows, 7, 3)
        b = check_sample_call(be, st, rows, 7, 3)
        assert (a == b).all()
        if size >= 7 and rows >= 63:
            assert (a != check_sample_call(be, st, rows, 7, 4)).any() and (a != check_sample_call(be, st, rows, 8, 3)).any()
            assert (a != check_sample_call(be, st, rows, 7 + (1 << 32), 3)).any()          # (the seed's high word is part of the key)
        if size == 7 and rows == 257:
            assert sorted(set(a.tolist())) == list(range(7))          # with replacement: every slot of a small store is hit, many times
    dst, picked = run_sample(be, st, 65, 7, 3, want_picked=False)
    assert (picked == SENT).all() and same_bits(dst, st.host[rp.reference_sample_slots(size, 65, 7, 3)])
    st.check(size)                         # a sample writes nothing to the store


def check_sample_empty(be):
    st = Store(be, 5, 3)
    dst, picked = run_sample(be, st, 65, 7, 0)
    assert (picked == -1).all() and (dst.view(np.int32) == sent_of(np.float32)).all()
    assert (rp.reference_sample_slots(0, 65, 7, 0) == -1).all()


def check_reproducible(be):
    def once():
        rng = np.random.default_rng(12)
        st = Store(be, 65, 4)
        picks = []
        for call, n in enumerate((30, 50, 65, 200)):
            src = rows_data(rng, n, 4, np.float32)
            append(be, st, src, None, n, n, 99, call, mode="no_idx")
            picks.append(run_sample(be, st, 64, 99, call))
        return be.get(st.d_buf), be.get(st.d_state), picks
    a, b = once(), once()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for (da, pa), (db, pb_) in zip(a[2], b[2]):
        assert da.tobytes() == db.tobytes() and pa.tobytes() == pb_.tobytes()


# ---- the numpy statements alone (CPU)

def worst_cell(draws, nvalues):
    """draws [trials, positions]: the (position, value) cell furthest from trials / nvalues, in standard deviations of its binomial"""
    trials, p = draws.shape[0], 1.0 / nvalues
    cells = np.array([[(draws[:, pos] == val).sum() for val in range(nvalues)] for pos in range(draws.shape[1])])
    return float(np.abs(cells - trials * p).max() / np.sqrt(trials * p * (1 - p)))


def test_reference_draws_are_uniform():
    """Size 7, the statements the kernels are pinned to bit for bit.  Victim choice: a full store of 7 takes 7 rows, row position j replaces slot perm(j); over 4096
    keys every (position, slot) cell within 5 standard deviations of 4096 / 7.  Sample draw: 64 row positions, the same.  An honest uniform draw leaves 5 standard
    deviations in one of these cells with probability below 1e-3.  The same over 512 calls of one key, as a store draws them.  Measured: victims 2.91 (seeds) / 2.92
    (calls), samples 3.76 / 3.52."""
    seeds = (0x5EED << 32) | np.arange(4096, dtype=np.uint64)
    victims = pb.reference_permutation(7, seeds, 3, rp.PASS_VICTIM)
    assert (victims[5] == rp.reference_append_slots(7, 7, 7, int(seeds[5]), 3)).all()          # (what the append statement uses)
    zv = worst_cell(victims, 7)
    samples = rp.reference_sample_slots(7, 64, seeds, 3)
    assert (samples[5] == rp.reference_sample_slots(7, 64, int(seeds[5]), 3)).all()
    zs = worst_cell(samples, 7)
    # over 512 calls with one key, as a store draws them
    calls_v = np.stack([pb.reference_permutation(7, 17, c, rp.PASS_VICTIM) for c in range(512)])
    calls_s = np.stack([rp.reference_sample_slots(7, 64, 17, c) for c in range(512)])
    zcv, zcs = worst_cell(calls_v, 7), worst_cell(calls_s, 7)
    print("worst cell in standard deviations: victims %.2f (over seeds) %.2f (over calls), samples %.2f (over seeds) %.2f (over calls)" % (zv, zcv, zs, zcs))
    assert zv < 5.0 and zs < 5.0 and zcv < 5.0 and zcs < 5.0


def test_reference_append_slots_properties():
    for cap in (1, 2, 7, 64, 65, 300):
        for old in sorted({0, cap // 2, cap - 1, cap}):
            for n in (1, cap - old, cap - old + 1, cap, cap + 1, 4 * cap + 3):
                if n < 1 or (old == 0 and n > cap and cap == 0):
                    continue
                s = rp.reference_append_slots(old, cap, n, 5, 9)
                kept = s[s >= 0]
                assert s.shape == (n,) and len(set(kept.tolist())) == kept.size == min(n, cap) and (kept < cap).all()
                fresh = np.sort(kept[kept >= old])
                assert (fresh == old + np.arange(min(n, cap - old))).all()          # every free slot is used before an old row goes
    assert (rp.reference_append_slots(3, 7, 2, 5, 9) == [3, 4]).all()
    assert (rp.reference_append_slots(7, 7, 9, 5, 9) != rp.reference_append_slots(7, 7, 9, 5, 10)).any() and (rp.reference_append_slots(7, 7, 9, 5, 9) != rp.reference_append_slots(7, 7, 9, 6, 9)).any()


# ---- the emulator library, host addresses

@pytest.mark.parametrize("cap", CAPACITIES)
def test_append_slots_emulator(emu_lib, cap):
    check_append_sequence(Emu(emu_lib), cap)


def test_append_count_clamped_emulator(emu_lib):
    check_count_clamped(Emu(emu_lib))


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_and_alignment_emulator(emu_lib, w, dtype):
    check_widths_and_alignment(Emu(emu_lib), w, dtype)


@pytest.mark.parametrize("T,N", [(5, 65), (33, 130)])
def test_append_from_ppo_batch_emulator(emu_lib, T, N):
    check_from_ppo_batch(Emu(emu_lib), T, N)


@pytest.mark.parametrize("size", [1, 2, 7, 65, 300])
def test_sample_emulator(emu_lib, size):
    check_sample(Emu(emu_lib), size)


def test_sample_empty_store_emulator(emu_lib):
    check_sample_empty(Emu(emu_lib))


def test_reproducible_emulator(emu_lib):
    check_reproducible(Emu(emu_lib))


def test_refusals_emulator(emu_lib):
    """host addresses that are never dereferenced: every call is refused before a launch, with its message"""
    from deepmimic_amd.core import load_library
    lib = load_library(emu_lib)
    buf, src, dst = np.full(64, 7.0, np.float32), np.zeros(64, np.float32), np.full(64, 7.0, np.float32)
    state, idx = np.zeros(2, np.int64), np.full(64, SENT, np.int32)
    good = dict(buf_ptr=buf.ctypes.data, capacity=8, width=2, state_ptr=state.ctypes.data, src_ptr=src.ctypes.data, idx_ptr=0, count_ptr=0, max_rows=4, seed=1, call=0,
                packed_ptr=dst.ctypes.data, slots_ptr=idx.ctypes.data, lib_path=emu_lib)
    bad = [(dict(buf_ptr=0), "null"), (dict(state_ptr=0), "null"), (dict(src_ptr=0), "null"), (dict(capacity=0), "capacity must be >= 1"), (dict(capacity=-2), "capacity"),
           (dict(width=0), "width must be >= 1"), (dict(max_rows=0), "max_rows must be >= 1"), (dict(max_rows=-1), "max_rows"),
           (dict(capacity=65536, width=32768), "2\\^31 - 1"), (dict(max_rows=2 ** 31 - 1, width=2), "2\\^31 - 1"),
           (dict(buf_ptr=buf.ctypes.data + 2), "misaligned"), (dict(src_ptr=src.ctypes.data + 1), "misaligned"), (dict(packed_ptr=dst.ctypes.data + 2), "misaligned"),
           (dict(idx_ptr=idx.ctypes.data + 2), "misaligned"), (dict(count_ptr=idx.ctypes.data + 1), "misaligned"), (dict(slots_ptr=idx.ctypes.data + 3), "misaligned"),
           (dict(state_ptr=state.ctypes.data + 4), "8-byte aligned")]
    for b, msg in bad:
        with pytest.raises(RuntimeError, match="dm_replay_append.*" + msg):
            rp.append_device(**dict(good, **b))
        assert b"dm_replay_append" in lib.dm_last_error()
    sgood = dict(buf_ptr=buf.ctypes.data, width=2, state_ptr=state.ctypes.data, rows=4, seed=1, call=0, dst_ptr=dst.ctypes.data, picked_ptr=idx.ctypes.data, lib_path=emu_lib)
    sbad = [(dict(buf_ptr=0), "null"), (dict(state_ptr=0), "null"), (dict(dst_ptr=0), "null"), (dict(width=0), "width must be >= 1"), (dict(rows=0), "rows must be >= 1"),
            (dict(rows=-3), "rows"), (dict(rows=65536, width=32768), "2\\^31 - 1"), (dict(buf_ptr=buf.ctypes.data + 2), "misaligned"), (dict(dst_ptr=dst.ctypes.data + 1), "misaligned"),
            (dict(picked_ptr=idx.ctypes.data + 2), "misaligned"), (dict(state_ptr=state.ctypes.data + 4), "8-byte aligned")]
    for b, msg in sbad:
        with pytest.raises(RuntimeError, match="dm_replay_sample.*" + msg):
            rp.sample_device(**dict(sgood, **b))
        assert b"dm_replay_sample" in lib.dm_last_error()
    assert (buf == 7.0).all() and (dst == 7.0).all() and (idx == SENT).all() and (state == 0).all()           # nothing was launched


# ---- the HIP library, torch tensors

@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPACITIES)
def test_append_slots_gpu(hip_lib, cap):
    check_append_sequence(Gpu(hip_lib), cap)


@pytest.mark.gpu
def test_append_count_clamped_gpu(hip_lib):
    check_count_clamped(Gpu(hip_lib))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_and_alignment_gpu(hip_lib, w, dtype):
    check_widths_and_alignment(Gpu(hip_lib), w, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(5, 65), (33, 130)])
def test_append_from_ppo_batch_gpu(hip_lib, T, N):
    check_from_ppo_batch(Gpu(hip_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 2, 7, 65, 300])
def test_sample_gpu(hip_lib, size):
    check_sample(Gpu(hip_lib), size)


@pytest.mark.gpu
def test_sample_empty_store_gpu(hip_lib):
    check_sample_empty(Gpu(hip_lib))


@pytest.mark.gpu
def test_reproducible_gpu(hip_lib):
    check_reproducible(Gpu(hip_lib))


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    """what only the HIP library checks: the device id (nothing is launched, the buffers keep their bytes)"""
    import torch
    buf, state, src = torch.full((8, 2), 7.0, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((4, 2), device="cuda")
    for dev in (-1, torch.cuda.device_count()):
        with pytest.raises(RuntimeError, match="dm_replay_append: invalid device_id"):
            rp.append_device(buf.data_ptr(), 8, 2, state.data_ptr(), src.data_ptr(), 0, 0, 4, 1, 0, device_id=dev, lib_path=hip_lib)
        with pytest.raises(RuntimeError, match="dm_replay_sample: invalid device_id"):
            rp.sample_device(buf.data_ptr(), 2, state.data_ptr(), 4, 1, 0, src.data_ptr(), device_id=dev, lib_path=hip_lib)
    with pytest.raises(RuntimeError, match="dm_replay_append.*misaligned"):
        rp.append_device(buf.data_ptr() + 2, 8, 2, state.data_ptr(), src.data_ptr(), 0, 0, 4, 1, 0, lib_path=hip_lib)
    assert (buf == 7.0).all() and (state == 0).all()


@pytest.mark.gpu
def test_torch_store_equals_the_raw_calls_and_checks_its_tensors(hip_lib):
    import torch
    T, N, w = 5, 65, (3, 2)
    r, v, m, f = make_inputs(T, N, seed=4)
    batch = pb.advantages_torch(*(torch.from_numpy(x).cuda() for x in (r, v, m, f)), lib_path=hip_lib)
    n_valid, _ = batch.counts_host()
    valid = np.flatnonzero(m.reshape(-1) != 0)
    src = torch.randn((T, N) + w, device="cuda")
    h_src = src.cpu().numpy().reshape(T * N, 6)
    store = rp.DeviceReplayStore(100, w, seed=13, lib_path=hip_lib)
    assert store.state_host() == (0, 0) and store.buf.shape == (100, 3, 2)
    out, picked = store.sample(9, picked=True)
    assert (picked == -1).all() and (out == 0).all() and out.shape == (9, 3, 2)
    host, size, total = np.zeros((100, 6), np.float32), 0, 0
    packed = torch.full((T * N,) + w, float(SENT), device="cuda")
    for call in range(2):                  # the second append finds 100 - n_valid free slots (or none) and takes victims
        assert store.append_batch(src, batch, packed=packed) is None
        want = rp.reference_append_slots(size, 100, n_valid, 13, call)
        host[want[want >= 0]] = h_src[valid][want >= 0]
        size, total = min(size + n_valid, 100), total + n_valid
        assert store.state_host() == (size, total) and same_bits(store.buf.cpu().numpy().reshape(100, 6), host)
    assert n_valid > 100 and same_bits(packed.cpu().numpy().reshape(T * N, 6)[:n_valid], h_src[valid]) and (packed.reshape(T * N, 6)[n_valid:] == SENT).all()
    slots = store.append(src.reshape(T * N, 3, 2), max_rows=7, slots=True)          # dense rows, idx and count absent
    want = rp.reference_append_slots(100, 100, 7, 13, 2)
    host[want] = h_src[:7]
    assert slots.dtype == torch.int32 and (slots.cpu().numpy() == want).all() and same_bits(store.buf.cpu().numpy().reshape(100, 6), host)
    for call in range(2):                  # the sample counter advances
        out, picked = store.sample(65, picked=True)
        want = rp.reference_sample_slots(100, 65, 13, call + 1)          # (call 0 was the sample of the empty store)
        assert (picked.cpu().numpy() == want).all() and same_bits(out.cpu().numpy().reshape(65, 6), host[want])
    mine = torch.empty((4, 3, 2), device="cuda")
    assert store.sample(4, out=mine) is mine
    store.clear()
    assert store.state_host() == (0, 0)
    ints = rp.DeviceReplayStore(8, 2, seed=1, dtype=torch.int32, lib_path=hip_lib)
    ints.append(torch.arange(12, dtype=torch.int32, device="cuda").reshape(6, 2))
    assert ints.state_host() == (6, 6) and (ints.buf[:6].cpu().numpy() == np.arange(12).reshape(6, 2)).all()
    for bad in (dict(src=src.double()), dict(src=src[:, :10]), dict(src=src.reshape(T * N * 3, 2)), dict(src=src, idx=batch.valid_idx.long()), dict(src=src, count=batch.counts),
                dict(src=src, max_rows=T * N + 1), dict(src=src, max_rows=0), dict(src=src, packed=packed.reshape(-1)[:10]), dict(src=src.cpu())):
        with pytest.raises(ValueError):
            store.append(**bad)
    for bad in (dict(rows=0), dict(rows=4, out=mine.double()), dict(rows=5, out=mine)):
        with pytest.raises(ValueError):
            store.sample(**bad)
    with pytest.raises(ValueError):
        rp.DeviceReplayStore(0, 3, lib_path=hip_lib)
    with pytest.raises(ValueError):
        rp.DeviceReplayStore(4, 3, dtype=torch.float64, lib_path=hip_lib)
    with pytest.raises(ValueError):
        rp.DeviceReplayStore(4, 3, device="cpu", lib_path=hip_lib)


@pytest.mark.gpu
def test_rollout_to_discriminator_batches_end_to_end_gpu(hip_lib):
    """One loop of the data stage (learning/amp_agent.py:216-249, 287-292) behind a 64-env rollout of amp_heading_clips4 (8 steps, episode timers of 0.1 .. 0.2 s):
    actor -> step with AMP observations -> returns -> advantages_torch -> append_batch of the agent observations with the packed rows -> amp_expert_draw of n_valid
    rows and a dense append -> one sample from each store -> the discriminator on both, finite.  The agent store holds exactly the valid observations, the packed
    rows are the valid observations in order, and DeviceNormalizer.record_device on them agrees with a numpy record of the same rows (tests/test_normalizer.py's
    tolerance: 1e-12 relative, 1e-13 absolute)."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    from normalizer_oracle import NormalizerOracle
    from deepmimic_amd import model, returns
    from deepmimic_amd.heads import Critic, Discriminator
    from deepmimic_amd.normalizer import DeviceNormalizer
    from deepmimic_amd.policy import Policy, random_weights
    from deepmimic_amd.vec_env import TorchVecEnv
    from test_scalar_heads import random_scalar_net
    T, N, B = 8, 64, 48
    env = TorchVecEnv(model.load_asset("amp_heading_clips4"), N, seed=3, lib_path=hip_lib, amp_obs=True)
    env.env.set_time_limits(0.1, 0.2)
    S, G, A, AMP = env.obs_dim, env.goal_dim, env.act_dim, env.env.amp_size
    assert AMP > 0 and G > 0
    actor = Policy(random_weights(S + G, A, seed=4), lib_path=hip_lib)
    critic = Critic(random_scalar_net(S + G, seed=5, scale=1.0), val_fail=0.0, val_succ=20.0, lib_path=hip_lib)
    disc = Discriminator(random_scalar_net(AMP, seed=6, scale=0.5), reward_scale=2.0, lib_path=hip_lib)
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    obs_all, tobs = torch.zeros((T + 1, N, S + G), **f32), torch.zeros((T, N, S + G), **f32)
    acts, amp, rewards = torch.zeros((T, N, A), **f32), torch.zeros((T, N, AMP), **f32), torch.zeros((T, N), **f32)
    flags, terminate, done, valid = (torch.zeros((T, N), **i32) for _ in range(4))
    stream = int(torch.cuda.current_stream().cuda_stream)
    obs = env.reset()
    goal = torch.from_numpy(env.env.query_goal()).to(obs.device)
    for t in range(T):
        obs_all[t] = torch.cat([obs, goal], dim=1)
        actor.forward_device_ex(obs_all[t].data_ptr(), N, acts[t].data_ptr(), exp_flags_ptr=flags[t].data_ptr(), exp_rate=0.5, sample=True, seed=21, step=t, stream=stream)
        obs, r, d, info = env.step(acts[t])
        goal = info["goal"]
        amp[t] = info["amp_obs"]
        rewards[t] = disc.eval_torch(info["amp_obs"])
        terminate[t], done[t], valid[t] = info["terminate"], d.to(torch.int32), info["valid"]
        tobs[t] = torch.cat([info["terminal_obs"], info["terminal_goal"]], dim=1)
    obs_all[T] = torch.cat([obs, goal], dim=1)
    ret, mask, values = returns.critic_returns_torch(critic, obs_all, None, tobs, None, terminate, done, valid, rewards, 0.95, 0.95, lib_path=hip_lib, return_values=True)
    batch = pb.advantages_torch(ret, values, mask, flags, lib_path=hip_lib)
    # ---- the data stage
    agent_store = rp.DeviceReplayStore(T * N, AMP, seed=31, lib_path=hip_lib)
    expert_store = rp.DeviceReplayStore(300, AMP, seed=32, lib_path=hip_lib)          # smaller than the rollout: keeps a subset
    packed = torch.zeros((T * N, AMP), **f32)
    agent_store.append_batch(amp, batch, packed=packed)
    n_valid, _ = batch.counts_host()                       # the iteration's one host read
    expert = env.amp_expert_draw(n_valid)
    expert_store.append(expert)
    amp_norm = DeviceNormalizer(AMP, lib_path=hip_lib)
    amp_norm.set_stream(stream)
    amp_norm.record_device(packed.data_ptr(), n_valid); amp_norm.record_device(expert.data_ptr(), n_valid)
    amp_norm.update()
    a_rows, a_pick = agent_store.sample(B, picked=True)
    e_rows, e_pick = expert_store.sample(B, picked=True)
    d_agent, d_expert = disc.eval_torch(a_rows, raw=True)[1], disc.eval_torch(e_rows, raw=True)[1]
    torch.cuda.synchronize()
    # ---- checks
    h_mask, h_amp, h_expert = mask.cpu().numpy().reshape(-1), amp.cpu().numpy().reshape(T * N, AMP), expert.cpu().numpy()
    valid_rows = np.flatnonzero(h_mask != 0)
    assert n_valid == valid_rows.size and 300 < n_valid <= T * N
    assert agent_store.state_host() == (n_valid, n_valid) and expert_store.state_host() == (300, n_valid)
    assert same_bits(agent_store.buf[:n_valid].cpu().numpy(), h_amp[valid_rows]) and same_bits(packed[:n_valid].cpu().numpy(), h_amp[valid_rows]) and (packed[n_valid:] == 0).all()
    slots = rp.reference_append_slots(0, 300, n_valid, 32, 0)
    want_expert = np.zeros((300, AMP), np.float32); want_expert[slots[slots >= 0]] = h_expert[slots >= 0]
    assert same_bits(expert_store.buf.cpu().numpy(), want_expert)
    assert (a_pick.cpu().numpy() == rp.reference_sample_slots(n_valid, B, 31, 0)).all() and same_bits(a_rows.cpu().numpy(), h_amp[valid_rows][a_pick.cpu().numpy()])
    assert (e_pick.cpu().numpy() == rp.reference_sample_slots(300, B, 32, 0)).all() and same_bits(e_rows.cpu().numpy(), want_expert[e_pick.cpu().numpy()])
    assert d_agent.shape == (B,) and torch.isfinite(d_agent).all() and torch.isfinite(d_expert).all() and float(d_agent.std()) > 0 and float(d_expert.std()) > 0
    assert np.isfinite(h_expert).all() and np.abs(h_expert).max() < 50
    ora = NormalizerOracle(AMP)
    ora.record(h_amp[valid_rows]); ora.record(h_expert); ora.update()
    assert amp_norm.count == 2 * n_valid == ora.count
    assert np.allclose(amp_norm.mean, ora.mean, rtol=1e-12, atol=1e-13) and np.allclose(amp_norm.std, ora.std, rtol=1e-12, atol=1e-13)
    for x in (actor, critic, disc, amp_norm, env):
        x.close()
