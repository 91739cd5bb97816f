"""Episode returns, lengths and end-cause totals on the device (deepmimic_amd/csrc/dm_episode.h, include/dm_hip.h dm_episode_stats, deepmimic_amd/episodes.py)
against `episodes.reference_episode_stats`, the same recursion in numpy float64 with math.fsum totals.  The kernel adds in fp64 in time order and rounds once, so the
per-step rows and the carries are compared bit for bit, integer totals and the histogram exactly, ret_min / ret_max exactly; an fp64 sum of k terms x_i is held to
k * 2^-52 * sum |x_i| of math.fsum -- the worst case of ANY summation order (each of the k - 1 additions rounds a partial sum of magnitude <= sum |x_i| by at most
2^-53 relative, plus the rounding of fsum itself), derived, not measured.  Shapes: T in {1, 5, 7} x N in {3, 64, 65, 257}: one partial wave, one full wave, one
wave + 1, one workgroup (256 lanes) + 1."""
import math

import numpy as np
import pytest

from deepmimic_amd import episodes as ep
from deepmimic_amd.core import load_library

W = 256                                  # the workgroup width of k_episode_scan
SHAPES = [(T, N) for T in (1, 5, 7) for N in (3, 64, 65, W + 1)]
BINS, BIN_STEPS = 5, 2


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(T, N, seed=0):
    """a seeded random [T, N] rollout with the forced columns below (those the shape has room for: column j needs N > j, the multi-step ones T >= 5)"""
    rng = np.random.default_rng(1000 * T + N + seed)
    r = rng.uniform(-0.5, 1.0, (T, N)).astype(np.float32)
    term = rng.integers(0, 3, (T, N)).astype(np.int32)
    done = (rng.random((T, N)) < 0.3).astype(np.int32)
    valid = (rng.random((T, N)) >= 0.1).astype(np.int32)
    acc = np.zeros(N, np.float64); ln = np.zeros(N, np.int32)
    far = np.arange(N) >= 9
    acc[far] = rng.uniform(-3, 30, far.sum()) * (rng.random(far.sum()) < 0.5); ln[far] = rng.integers(0, 40, far.sum())      # random carries on the random columns
    L = T - 1

    def col(j, dones, terms=None, valids=None):
        if j < N:
            done[:, j] = 0; valid[:, j] = 1; acc[j] = 0.0; ln[j] = 0
            for k, t in enumerate(dones):
                done[t, j] = 1
                if terms is not None:
                    term[t, j] = terms[k]
                if valids is not None:
                    valid[t, j] = valids[k]
    col(0, [])                                                    # no done
    col(1, [0], [1])                                              # done at t = 0
    col(2, [L], [1])                                              # done at t = T - 1 ...
    if N > 2:
        acc[2], ln[2] = 2.5, 11                                   # ... of an episode that began before the window: a non-zero carry on entry
    if T >= 5:
        col(3, [1, 2, 3], [0, 1, 2])                              # consecutive dones of class Null / Fail / Succ
        col(4, [2], [1], [0])                                     # valid == 0 at a done
        col(5, [1, 3], [1, 2], [1, 1])                            # a NaN reward inside an episode that ends with valid == 1, then a clean episode
        col(6, [1, 4], [2, 0], [1, 1])                            # the same with +inf
        col(7, [2], [7])                                          # terminate 7 at a done: counts as Null
    else:                                                         # T = 1: the one-step forms
        col(3, [0], [2]); col(4, [0], [1], [0]); col(5, [0], [1], [1]); col(6, [0], [2], [1]); col(7, [0], [7])
    if N > 5:
        r[0, 5] = np.nan
    if N > 6:
        r[0, 6] = np.inf
    return dict(rewards=r, terminate=term, done=done, valid=valid, acc_return=acc, acc_len=ln)


_cache = {}


def case(T, N):
    """the inputs of a shape and the reference on them: computed once, shared, never modified"""
    if (T, N) not in _cache:
        inp = make_inputs(T, N)
        ref = ep.reference_episode_stats(inp["rewards"], inp["terminate"], inp["done"], inp["valid"], inp["acc_return"], inp["acc_len"], BINS, BIN_STEPS)
        for a in list(inp.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[(T, N)] = (inp, ref)
    return _cache[(T, N)]


@pytest.mark.parametrize("T,N", SHAPES)
def test_inputs_contain_the_forced_cases(T, N):
    inp, ref = case(T, N)
    r, term, done, valid, acc, ln = (inp[k] for k in ("rewards", "terminate", "done", "valid", "acc_return", "acc_len"))
    b = ref["block"]
    assert not done[:, 0].any() and ref["ep_len"][T - 1, 0] == T and ref["acc_len"][0] == T                  # no done: the episode stays in the carry
    assert done[0, 1] == 1 and ref["ep_len"][0, 1] == 1                                                     # done at t = 0
    assert done[T - 1, 2] == 1 and term[T - 1, 2] == 1 and ref["acc_len"][2] == 0                           # done at t = T - 1
    assert acc[2] == 2.5 and ln[2] == 11 and ref["ep_len"][T - 1, 2] == 11 + T                              # a non-zero carry on entry, counted with what it held
    assert b[ep.LEN_MAX + ep.FAIL] >= 11 + T
    if N >= 9:
        t4 = 2 if T >= 5 else 0
        assert done[t4, 4] == 1 and valid[t4, 4] == 0                                                       # valid == 0 at a done
        t5 = 1 if T >= 5 else 0
        assert np.isnan(r[0, 5]) and done[t5, 5] == 1 and valid[t5, 5] == 1 and np.isnan(ref["ep_return"][t5, 5])      # NaN inside an episode that ends valid
        assert np.isposinf(r[0, 6]) and done[t5, 6] == 1 and valid[t5, 6] == 1 and np.isposinf(ref["ep_return"][t5, 6])
        assert term[t4, 7] == 7 and done[t4, 7] == 1 and valid[t4, 7] == 1                                  # terminate 7 at a done
        assert b[ep.EPISODES + ep.INVALID] >= 3 and b[ep.EPISODES + ep.NULL] >= 1
        if T >= 5:
            assert done[1:4, 3].all() and list(term[1:4, 3]) == [0, 1, 2] and (valid[1:4, 3] == 1).all()    # consecutive dones of every class
            assert list(ref["ep_len"][1:4, 3]) == [2, 1, 1]
            assert done[3, 5] == 1 and np.isfinite(ref["ep_return"][2:4, 5]).all() and ref["ep_len"][3, 5] == 2      # ... followed by a clean episode in the column
            assert done[4, 6] == 1 and np.isfinite(ref["ep_return"][2:5, 6]).all() and ref["ep_len"][4, 6] == 3
        assert all(np.isfinite(x) for c in range(3) for x in ref["returns"][c])                             # no non-finite return reaches a sum
    if N >= 64:
        assert (acc[9:] != 0).any() and (ln[9:] != 0).any() and (done[:, 9:] != 0).any() and (valid[:, 9:] == 0).any()


# ---------------------------------------------------------------------------------------------------------------- the two ways to run a call
class Emulator:
    """host arrays, the CPU build of the same sources"""
    gpu = False

    def __init__(self, lib):
        self.lib = lib

    def dev(self, a):
        return np.array(a)                       # a private, writable copy

    def ptr(self, a):
        return a.ctypes.data if a is not None else 0

    def host(self, a):
        return a


class Gpu:
    """torch tensors on the GPU, torch's current stream"""
    gpu = True

    def __init__(self, lib):
        import torch
        self.lib, self.torch = lib, torch

    def dev(self, a):
        return self.torch.from_numpy(np.array(a)).cuda()

    def ptr(self, a):
        return a.data_ptr() if a is not None else 0

    def host(self, a):
        return a.cpu().numpy()


def call(be, inp, rows=slice(None), carry=None, block=None, bins=BINS, bin_steps=BIN_STEPS, use_valid=True, per_step=True, totals=True, hist=True, work=True):
    """one dm_episode_stats call on rows `rows` of the inputs, on `carry` = (acc_return, acc_len) and `block` (both backend arrays, modified in place; None: the
    inputs' carry / the initial block).  Returns host copies, the backend carry and block for a next window, and the sentinel-filled per-step arrays."""
    r, term, done, valid = (be.dev(inp[k][rows]) for k in ("rewards", "terminate", "done", "valid"))
    T, N = inp["rewards"][rows].shape
    carry = carry if carry is not None else (be.dev(inp["acc_return"]), be.dev(inp["acc_len"]))
    block = block if block is not None else be.dev(ep.initial_block(bins))
    out_r, out_l = be.dev(np.full((T, N), -7.0, np.float32)), be.dev(np.full((T, N), -7, np.int32))
    nbytes = ep.workspace_bytes(N, be.lib)
    ws = be.dev(np.zeros(nbytes // 8, np.int64))
    stream = 0
    if be.gpu:
        from deepmimic_amd.binding import stream_handle
        stream = stream_handle(r.device)
    ep.episode_stats_device(T, N, be.ptr(r), be.ptr(term), be.ptr(done), be.ptr(valid) if use_valid else 0, be.ptr(carry[0]), be.ptr(carry[1]),
                            be.ptr(out_r) if per_step else 0, be.ptr(out_l) if per_step else 0, totals_ptr=be.ptr(block) if totals else 0,
                            hist_ptr=be.ptr(block) + 8 * ep.TOTALS_WORDS if (hist and bins) else 0, bins=bins, bin_steps=bin_steps,
                            work_ptr=be.ptr(ws) if work else 0, work_nbytes=nbytes if work else 0, stream=stream, lib_path=be.lib)
    return dict(ep_return=be.host(out_r), ep_len=be.host(out_l), acc_return=be.host(carry[0]), acc_len=be.host(carry[1]), block=be.host(block), carry=carry, dev_block=block)


def sums_within_bound(block, ref):
    """every fp64 sum of `block` against math.fsum of the reference's terms: |got - fsum| <= k * 2^-52 * sum |x|"""
    f = np.asarray(block).view(np.float64)
    for c in range(3):
        for word, terms in ((ep.RET_SUM + c, ref["returns"][c]), (ep.RET_SQ + c, ref["squares"][c])):
            want, bound = math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(abs(x) for x in terms)
            assert abs(f[word] - want) <= bound, (c, word, f[word], want, bound)


def totals_agree(block, ref):
    want = ref["block"]
    ints = list(range(ep.EPISODES, ep.RET_SUM)) + list(range(ep.STEPS_SEEN, len(want)))         # episodes, steps, len_max; steps_seen and the histogram
    assert (np.asarray(block)[ints] == want[ints]).all(), (np.asarray(block)[ints], want[ints])
    assert same_bits(np.asarray(block)[ep.RET_MIN:ep.STEPS_SEEN], want[ep.RET_MIN:ep.STEPS_SEEN])      # ret_min / ret_max: exact
    sums_within_bound(block, ref)


def recursion(be, T, N):
    inp, ref = case(T, N)
    got = call(be, inp)
    for k in ("ep_return", "ep_len", "acc_return", "acc_len"):
        assert same_bits(got[k], ref[k]), (k, T, N)
    totals_agree(got["block"], ref)
    assert got["block"][ep.STEPS_SEEN] == T * N and got["block"][ep.TOTALS_WORDS:].sum() == got["block"][ep.EPISODES:ep.EPISODES + 3].sum()


@pytest.mark.parametrize("T,N", SHAPES)
def test_recursion_equals_the_reference_emulator(emu_lib, T, N):
    recursion(Emulator(emu_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_recursion_equals_the_reference_gpu(hip_lib, T, N):
    recursion(Gpu(hip_lib), T, N)


def test_the_bound_has_room_on_a_long_sum():
    """100 000 terms added left to right sit orders of magnitude inside k * 2^-52 * sum |x| of math.fsum (the bound is the worst case, not a fit)"""
    x = np.random.default_rng(5).uniform(-0.5, 30.0, 100000)
    s = 0.0
    for v in x:
        s += float(v)
    err, bound = abs(s - math.fsum(x)), len(x) * 2.0 ** -52 * math.fsum(np.abs(x))
    assert err <= bound * 1e-3, (err, bound)


# ---------------------------------------------------------------------------------------------------------------- windows, reproducibility
def windows_compose(be, N):
    inp, ref = case(7, N)
    whole = call(be, inp)
    carry = block = None
    rows_r, rows_l = [], []
    for a, b in ((0, 3), (3, 4), (4, 7)):
        part = call(be, inp, rows=slice(a, b), carry=carry, block=block)
        carry, block = part["carry"], part["dev_block"]
        rows_r.append(part["ep_return"]); rows_l.append(part["ep_len"])
    assert same_bits(np.concatenate(rows_r), whole["ep_return"]) and same_bits(np.concatenate(rows_l), whole["ep_len"])
    assert same_bits(part["acc_return"], whole["acc_return"]) and same_bits(part["acc_len"], whole["acc_len"])
    totals_agree(part["block"], ref); totals_agree(whole["block"], ref)
    assert same_bits(part["block"][:ep.RET_SUM], whole["block"][:ep.RET_SUM]) and same_bits(part["block"][ep.RET_MIN:], whole["block"][ep.RET_MIN:])


@pytest.mark.parametrize("N", [3, 65, W + 1])
def test_windows_compose_through_the_carry_emulator(emu_lib, N):
    windows_compose(Emulator(emu_lib), N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [3, 65, W + 1])
def test_windows_compose_through_the_carry_gpu(hip_lib, N):
    windows_compose(Gpu(hip_lib), N)


def reproducible(be):
    inp, _ = case(7, W + 1)
    a, b = call(be, inp), call(be, inp)
    for k in ("ep_return", "ep_len", "acc_return", "acc_len", "block"):
        assert same_bits(a[k], b[k]), k


def test_two_runs_give_the_same_bytes_emulator(emu_lib):
    reproducible(Emulator(emu_lib))


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes_gpu(hip_lib):
    reproducible(Gpu(hip_lib))


# ---------------------------------------------------------------------------------------------------------------- optional arrays, histogram edges
def optional_arrays(be):
    inp, ref = case(7, 65)
    ones = dict(inp, valid=np.ones_like(inp["valid"]))
    a, b = call(be, ones), call(be, inp, use_valid=False)                       # valid NULL = all ones
    for k in ("ep_return", "ep_len", "acc_return", "acc_len", "block"):
        assert same_bits(a[k], b[k]), k
    assert a["block"][ep.EPISODES + ep.INVALID] < ref["block"][ep.EPISODES + ep.INVALID]          # (the inputs do have valid == 0 at a done)
    full = call(be, inp)
    c = call(be, inp, per_step=False)                                           # ep_*_out NULL: the sentinel buffers keep their bytes, everything else is as before
    assert (c["ep_return"] == -7.0).all() and (c["ep_len"] == -7).all()
    assert same_bits(c["block"], full["block"]) and same_bits(c["acc_return"], full["acc_return"]) and same_bits(c["acc_len"], full["acc_len"])
    d = call(be, inp, totals=False, hist=False, work=False)                     # no totals, no histogram, no workspace: the carry and the rows still move
    assert same_bits(d["block"], ep.initial_block(BINS))
    for k in ("ep_return", "ep_len", "acc_return", "acc_len"):
        assert same_bits(d[k], ref[k]), k
    e = call(be, inp, totals=False)                                             # a histogram alone
    assert same_bits(e["block"][ep.TOTALS_WORDS:], ref["block"][ep.TOTALS_WORDS:]) and same_bits(e["block"][:ep.TOTALS_WORDS], ep.initial_block(0))
    # histogram edges, bin_steps = 3: L = 3 -> bin 0, L = 4 -> bin 1, L = 7 -> bin 2, or the last bin there is
    done = np.zeros((7, 3), np.int32); done[2, 0] = done[3, 1] = done[6, 2] = 1
    edges = dict(rewards=np.ones((7, 3), np.float32), terminate=np.zeros((7, 3), np.int32), done=done, valid=np.ones((7, 3), np.int32),
                 acc_return=np.zeros(3), acc_len=np.zeros(3, np.int32))
    for bins, want in ((1, [3]), (2, [1, 2]), (3, [1, 1, 1]), (4, [1, 1, 1, 0])):
        h = call(be, edges, bins=bins, bin_steps=3)["block"]
        assert list(h[ep.TOTALS_WORDS:]) == want and h[ep.EPISODES] == 3 and h[ep.STEPS] == 14 and h[ep.LEN_MAX] == 7, (bins, h)
        assert same_bits(h, ep.reference_episode_stats(edges["rewards"], edges["terminate"], done, None, edges["acc_return"], edges["acc_len"], bins, 3)["block"])


def test_optional_arrays_and_histogram_edges_emulator(emu_lib):
    optional_arrays(Emulator(emu_lib))


@pytest.mark.gpu
def test_optional_arrays_and_histogram_edges_gpu(hip_lib):
    optional_arrays(Gpu(hip_lib))


# ---------------------------------------------------------------------------------------------------------------- refusals
def refusals(lib_path):
    """host addresses: every call is refused before a launch, so none is dereferenced (on the GPU too)"""
    lib = load_library(lib_path)
    T, N = 2, 4
    f = np.zeros(T * N, np.float32); i = np.zeros(T * N, np.int32)
    acc = np.full(N + 1, 7.0); ln = np.full(N, 7, np.int32); out_r = np.full(T * N, 7.0, np.float32); out_l = np.full(T * N, 7, np.int32)
    block = np.full(ep.TOTALS_WORDS + 4, 7, np.int64)
    nbytes = ep.workspace_bytes(N, lib_path)
    ws = np.full(nbytes // 8 + 1, 7, np.int64)
    assert nbytes >= 8 and nbytes % 8 == 0
    with pytest.raises(RuntimeError, match="dm_episode_workspace_bytes"):
        ep.workspace_bytes(0, lib_path)
    good = dict(T=T, N=N, rewards_ptr=f.ctypes.data, terminate_ptr=i.ctypes.data, done_ptr=i.ctypes.data, valid_ptr=i.ctypes.data, acc_return_ptr=acc.ctypes.data,
                acc_len_ptr=ln.ctypes.data, ep_return_ptr=out_r.ctypes.data, ep_len_ptr=out_l.ctypes.data, totals_ptr=block.ctypes.data,
                hist_ptr=block.ctypes.data + 8 * ep.TOTALS_WORDS, bins=4, bin_steps=1, work_ptr=ws.ctypes.data, work_nbytes=nbytes, lib_path=lib_path)
    bad = [dict(T=0), dict(N=0), dict(T=-3), dict(N=-1), dict(T=65536, N=32768),                                   # T * N = 2^31
           dict(rewards_ptr=0), dict(terminate_ptr=0), dict(done_ptr=0), dict(acc_return_ptr=0), dict(acc_len_ptr=0),
           dict(bins=0), dict(bin_steps=0), dict(bins=-2),
           dict(work_nbytes=nbytes - 1), dict(work_nbytes=0), dict(work_nbytes=nbytes - 1, hist_ptr=0), dict(work_nbytes=nbytes - 1, totals_ptr=0),
           dict(work_ptr=0),
           dict(acc_return_ptr=acc.ctypes.data + 4), dict(totals_ptr=block.ctypes.data + 4), dict(hist_ptr=block.ctypes.data + 8 * ep.TOTALS_WORDS + 4)]
    for b in bad:
        with pytest.raises(RuntimeError, match="dm_episode_stats"):
            ep.episode_stats_device(**dict(good, **b))
        assert b"dm_episode_stats" in lib.dm_last_error()
    for a in (acc, ln, out_r, out_l, block, ws):
        assert (a == 7).all()               # nothing was launched


def test_refusals_emulator(emu_lib):
    refusals(emu_lib)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    import torch
    refusals(hip_lib)
    # a device_id that names no device, on device arrays: refused by name, the arrays keep their bytes
    be = Gpu(hip_lib)
    r, i = be.dev(np.zeros((1, 4), np.float32)), be.dev(np.ones((1, 4), np.int32))
    acc, ln, block = be.dev(np.full(4, -77.0)), be.dev(np.full(4, -77, np.int32)), be.dev(np.full(ep.TOTALS_WORDS, -77, np.int64))
    ws = be.dev(np.full(ep.workspace_bytes(4, hip_lib) // 8, -77, np.int64))
    for dev in (-1, torch.cuda.device_count()):
        with pytest.raises(RuntimeError, match="dm_episode_stats: invalid device_id"):
            ep.episode_stats_device(1, 4, r.data_ptr(), i.data_ptr(), i.data_ptr(), 0, acc.data_ptr(), ln.data_ptr(), totals_ptr=block.data_ptr(), work_ptr=ws.data_ptr(),
                                    work_nbytes=ws.numel() * 8, device_id=dev, lib_path=hip_lib)
    torch.cuda.synchronize()
    for t in (acc, ln, block, ws):
        assert (t == -77).all()


# ---------------------------------------------------------------------------------------------------------------- the torch front end
@pytest.mark.gpu
def test_episode_stats_class_checks_its_tensors_gpu(hip_lib):
    import torch
    T, N = 3, 4
    f = lambda *s: torch.ones(s, dtype=torch.float32, device="cuda")
    i = lambda *s: torch.ones(s, dtype=torch.int32, device="cuda")
    st = ep.EpisodeStats(N, "cuda:0", bins=3, bin_steps=2, lib_path=hip_lib)
    ok = dict(rewards=f(T, N), terminate=i(T, N), done=i(T, N), valid=i(T, N))
    for k, bad in (("rewards", f(T, N).double()), ("rewards", f(N, T).t()), ("terminate", i(T, N).cpu()), ("done", i(T, N + 1)), ("done", i(T + 1, N)), ("valid", f(T, N))):
        with pytest.raises(ValueError):
            st.update(**dict(ok, **{k: bad}))
    assert same_bits(st.raw(), ep.initial_block(3)) and (st.acc_len == 0).all()          # a rejected call changed nothing
    ret, ln = st.update(**dict(ok, done=torch.zeros((T, N), dtype=torch.bool, device="cuda")))      # a bool `done`
    assert ret.shape == (T, N) and (ln.cpu().numpy() == np.arange(1, T + 1)[:, None]).all() and (st.acc_len == T).all()
    ret, ln = st.update(f(N), i(N), torch.ones(N, dtype=torch.bool, device="cuda"), i(N))                 # a 1-D step: every env ends after T + 1 steps with Fail
    assert ret.shape == (N,) and (ln == T + 1).all() and (ret == T + 1.0).all() and (st.acc_len == 0).all()
    assert st.update(f(N), i(N), i(N), per_step=False) is None                                           # valid None: length-1 episodes
    tot = st.totals()
    assert tot["episodes"] == 2 * N and tot["fail"]["episodes"] == 2 * N and tot["fall_share"] == 1.0 and tot["invalid_share"] == 0.0 and tot["steps_seen"] == (T + 2) * N
    assert tot["max_length"] == T + 1 and tot["mean_length"] == (T + 2) / 2 and tot["mean_return"] == (T + 2) / 2 and tot["min_return"] == 1.0 and tot["max_return"] == T + 1.0
    assert abs(tot["std_return"] - T / 2) < 1e-12 and list(tot["histogram"]) == [N, N, 0]                # lengths 1 and 4 in bins of 2 steps
    merged = ep.decode_block(ep.EpisodeStats.merge([st.raw(), st.raw()]), 2)
    assert merged["episodes"] == 4 * N and merged["max_length"] == T + 1 and merged["min_return"] == 1.0 and list(merged["histogram"]) == [2 * N, 2 * N, 0]
    st.clear_totals(); st.acc_len.fill_(5); st.reset_carry(torch.tensor([1], device="cuda"))
    assert same_bits(st.raw(), ep.initial_block(3)) and st.acc_len.tolist() == [5, 0, 5, 5]
    st.reset_carry()
    assert (st.acc_len == 0).all() and (st.acc_return == 0).all()


def test_merge_and_decode_are_host_functions():
    """raw blocks add in list order without a GPU; an empty window decodes to NaN means and shares"""
    inp, ref = case(7, 65)
    two = ep.merge_blocks([ref["block"], ref["block"], ep.initial_block(BINS)])
    assert (two[ep.EPISODES:ep.LEN_MAX] == 2 * ref["block"][ep.EPISODES:ep.LEN_MAX]).all() and (two[ep.STEPS_SEEN:] == 2 * ref["block"][ep.STEPS_SEEN:]).all()
    assert same_bits(two[ep.LEN_MAX:ep.RET_SUM], ref["block"][ep.LEN_MAX:ep.RET_SUM]) and same_bits(two[ep.RET_MIN:ep.STEPS_SEEN], ref["block"][ep.RET_MIN:ep.STEPS_SEEN])
    d = ep.decode_block(ref["block"], BIN_STEPS)
    n = sum(len(x) for x in ref["returns"])
    assert d["episodes"] == n and d["fall_share"] == len(ref["returns"][1]) / n and abs(d["mean_return"] - math.fsum(sum(ref["returns"], [])) / n) < 1e-12
    empty = ep.decode_block(ep.initial_block(2))
    assert empty["episodes"] == 0 and math.isnan(empty["mean_return"]) and math.isnan(empty["fall_share"]) and math.isnan(empty["invalid_share"])
    with pytest.raises(ValueError):
        ep.merge_blocks([ref["block"], ep.initial_block(0)])


# ---------------------------------------------------------------------------------------------------------------- end to end
def rollout(make, hip_lib, episode_stats):
    """humanoid3d_walk, 64 envs, 8 steps, episode timers of 0.1 .. 0.2 s, actions 0.6 * randn: the stacked host copies of every step's outputs"""
    import torch
    from deepmimic_amd import model
    T, N = 8, 64
    env = make(model.load_asset("humanoid3d_walk"), N, seed=3, lib_path=hip_lib, episode_stats=episode_stats)
    for c in ([env.env] if hasattr(env, "env") else env.g.envs):
        c.set_time_limits(0.1, 0.2)
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    env.reset()
    keys, rows = None, {k: [] for k in ("rewards", "terminate", "done", "valid", "episode_return", "episode_length")}
    for t in range(T):
        acts = 0.6 * torch.randn((N, env.act_dim), generator=gen, dtype=torch.float32, device="cuda")
        _, r, d, info = env.step(acts)
        keys = sorted(info)
        rows["rewards"].append(r.cpu().numpy()); rows["done"].append(d.to(torch.int32).cpu().numpy())
        rows["terminate"].append(info["terminate"].cpu().numpy()); rows["valid"].append(info["valid"].cpu().numpy())
        if episode_stats:
            rows["episode_return"].append(info["episode_return"].cpu().numpy()); rows["episode_length"].append(info["episode_length"].cpu().numpy())
    out = {k: np.stack(v) for k, v in rows.items() if v}
    out["keys"] = keys
    out["totals"] = env.episode_totals() if episode_stats else None
    if not episode_stats:
        with pytest.raises(RuntimeError):
            env.episode_totals()
    env.close()
    return out


@pytest.mark.gpu
def test_vec_env_episode_stats_end_to_end_gpu(hip_lib):
    from deepmimic_amd.vec_env import TorchVecEnv, TorchVecEnvGroups
    T, N = 8, 64
    one = rollout(TorchVecEnv, hip_lib, True)
    done, term, valid = one["done"], one["terminate"], one["valid"]
    assert done.sum() >= N and ((done != 0) & (term == 0) & (valid != 0)).any()              # every env's timer ran out at least once: Null ends are in
    ref = ep.reference_episode_stats(one["rewards"], term, done, valid, np.zeros(N), np.zeros(N, np.int32))
    assert same_bits(one["episode_return"], ref["ep_return"]) and same_bits(one["episode_length"], ref["ep_len"])
    cls = np.where((valid == 0) | ~np.isfinite(ref["ep_return"].astype(np.float64)), 3, np.where((term == 1) | (term == 2), term, 0))
    tot = one["totals"]
    for c, name in enumerate(ep.CLASS_NAMES):
        rows_c = (done != 0) & (cls == c)
        assert tot[name]["episodes"] == rows_c.sum() and tot[name]["steps"] == one["episode_length"][rows_c].sum(), name
        assert tot[name]["max_length"] == (one["episode_length"][rows_c].max() if rows_c.any() else 0)
    assert tot["steps_seen"] == T * N and tot["episodes"] + tot["invalid"]["episodes"] == done.sum()
    totals_agree(tot["block"], ref)
    grp = rollout(lambda t, n, **kw: TorchVecEnvGroups(t, n, groups=2, **kw), hip_lib, True)
    for k in ("rewards", "terminate", "done", "valid", "episode_return", "episode_length"):
        assert same_bits(grp[k], one[k]), k
    ints = list(range(ep.EPISODES, ep.RET_SUM)) + [ep.STEPS_SEEN]
    assert (grp["totals"]["block"][ints] == tot["block"][ints]).all()
    assert same_bits(grp["totals"]["block"][ep.RET_MIN:ep.STEPS_SEEN], tot["block"][ep.RET_MIN:ep.STEPS_SEEN])
    sums_within_bound(grp["totals"]["block"], ref)
    assert grp["keys"] == one["keys"] == ["episode_length", "episode_return", "terminal_obs", "terminate", "valid"]
    for make in (TorchVecEnv, lambda t, n, **kw: TorchVecEnvGroups(t, n, groups=2, **kw)):
        off = rollout(make, hip_lib, False)
        assert off["keys"] == ["terminal_obs", "terminate", "valid"]                          # the set it is today
        for k in ("rewards", "terminate", "done", "valid"):
            assert same_bits(off[k], one[k]), k
