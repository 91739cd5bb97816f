"""PPO training batches on the device (deepmimic_amd/csrc/dm_ppo_batch.h, include/dm_hip.h dm_ppo_advantages / dm_ppo_gather, deepmimic_amd/ppo_batch.py) against
the numpy statements beside the binding.  Every case runs on the emulator library through host addresses and again, marked `gpu`, through torch tensors.

Shapes are the ones the index arithmetic can break on: one element, less than a wavefront, exactly one, one past one, one past a 256-thread workgroup, and
33 x 130 = 4290 samples = 5 groups of the kernels' 1024-sample partials (test_shapes_cover_three_partial_groups holds that against dm_ppo_workspace_bytes).
Tolerances: the lists, counts, targets, picked rows and gathered rows are exact.  The statistics are held to 1e-12 relative -- fp64 summation error at <= 10^4
terms is ~1e-15 -- which a one-pass variance misses by eight decades on the a = 1000 + 1e-3 normal input.  adv is held to one fp32 ulp of the float32 rounding of
the reference: what a last-bit difference in the fp64 statistics can move through the final rounding."""
import numpy as np
import pytest

from deepmimic_amd import ppo_batch as pb

SHAPES = [(1, 1), (3, 5), (2, 64), (5, 65), (4, 257), (33, 130)]
SENT = -77
PERM_COUNTS = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 257, 1000]


class Emu:
    """host memory and the emulator library: a 'device array' is a numpy view whose first byte is 16-byte aligned, or `off` elements behind such a byte"""
    def __init__(self, lib):
        self.lib, self.stream = lib, 0

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        buf = np.zeros(a.size + 8, a.dtype)
        start = ((-buf.ctypes.data) % 16) // a.itemsize + off
        view = buf[start:start + a.size].reshape(a.shape)
        view[...] = a
        return view

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return h.copy()


class Gpu:
    """torch tensors on the GPU and the HIP library, on torch's current stream"""
    def __init__(self, lib):
        import torch
        self.lib, self.torch, self.stream = lib, torch, int(torch.cuda.current_stream().cuda_stream)

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        buf = self.torch.zeros(a.size + 8, dtype=getattr(self.torch, a.dtype.name), device="cuda")        # (the allocator's blocks are 16-byte aligned)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + a.size].view(a.shape)
        view.copy_(self.torch.from_numpy(a))
        return view

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        return h.cpu().numpy()


def make_inputs(T, N, seed=0, big_offset=False):
    """seeded normals; mask with about 20 % zeros in runs along t; exp_flags with about 30 % zeros"""
    rng = np.random.default_rng([seed, T, N])
    values = rng.standard_normal((T + 1, N)).astype(np.float32)
    returns = rng.standard_normal((T, N)).astype(np.float32)
    if big_offset:                         # a = 1000 + 1e-3 normal: E[x^2] - E[x]^2 loses every digit of this variance
        returns = (values[:T].astype(np.float64) + 1000.0 + 1e-3 * rng.standard_normal((T, N))).astype(np.float32)
    mask = np.ones((T, N), np.int32)
    for n in range(N):
        if rng.random() < 0.5:
            t0, length = int(rng.integers(0, T)), int(rng.integers(1, max(1, (4 * T + 4) // 5) + 1))
            mask[t0:t0 + length, n] = 0
    flags = (rng.random((T, N)) >= 0.3).astype(np.int32)
    return returns, values, mask, flags


def run_adv(be, returns, values, mask, flags, eps=1e-5, clip=5.0, vmin=-np.inf, vmax=np.inf):
    T, N = returns.shape
    nbytes = pb.workspace_bytes(T, N, be.lib)
    d = dict(returns=be.put(returns), values=be.put(values), mask=None if mask is None else be.put(mask), flags=None if flags is None else be.put(flags),
             adv=be.put(np.full((T, N), np.nan, np.float32)), targets=be.put(np.full((T, N), np.nan, np.float32)),
             valid_idx=be.put(np.full(T * N, SENT, np.int32)), exp_idx=be.put(np.full(T * N, SENT, np.int32)), counts=be.put(np.full(2, SENT, np.int32)),
             stats=be.put(np.full(2, np.nan, np.float64)), work=be.put(np.zeros(nbytes // 8, np.float64)))
    pb.advantages_device(T, N, be.ptr(d["returns"]), be.ptr(d["values"]), 0 if mask is None else be.ptr(d["mask"]), 0 if flags is None else be.ptr(d["flags"]),
                         eps, clip, vmin, vmax, be.ptr(d["adv"]), be.ptr(d["targets"]), be.ptr(d["valid_idx"]), be.ptr(d["exp_idx"]), be.ptr(d["counts"]),
                         be.ptr(d["stats"]), be.ptr(d["work"]), nbytes, stream=be.stream, lib_path=be.lib)
    return {k: be.get(d[k]) for k in ("adv", "targets", "valid_idx", "exp_idx", "counts", "stats")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_lists(out, ref):
    nv, ne = ref["counts"]
    assert tuple(out["counts"]) == (nv, ne)
    assert (out["valid_idx"][:nv] == ref["valid_idx"]).all() and (out["valid_idx"][nv:] == SENT).all()
    assert (out["exp_idx"][:ne] == ref["exp_idx"]).all() and (out["exp_idx"][ne:] == SENT).all()


def variants(T, N):
    r, v, m, f = make_inputs(T, N)
    one = np.zeros((T, N), np.int32); one.reshape(-1)[(T * N) // 2] = 1
    return [("both", r, v, m, f), ("no mask", r, v, None, f), ("no flags", r, v, m, None), ("neither", r, v, None, None),
            ("all masked", r, v, np.zeros((T, N), np.int32), f), ("one exp sample", r, v, np.ones((T, N), np.int32), one)]


def check_counts_and_lists(be, T, N):
    for name, r, v, m, f in variants(T, N):
        out, ref = run_adv(be, r, v, m, f), pb.reference_advantages(r, v, m, f)
        check_lists(out, ref)
        if name == "all masked":
            assert tuple(out["counts"]) == (0, 0) and same_bits(out["stats"], np.zeros(2)) and same_bits(out["adv"], np.zeros((T, N), np.float32))
        if name == "one exp sample":
            assert tuple(out["counts"]) == (T * N, 1) and out["stats"][1] == 0.0 and same_bits(out["adv"], np.zeros((T, N), np.float32))
            a = float(r.reshape(-1)[(T * N) // 2]) - float(v[:T].reshape(-1)[(T * N) // 2])
            assert out["stats"][0] == a


def check_statistics(be, T, N):
    for big in (False, True):
        r, v, m, f = make_inputs(T, N, seed=1, big_offset=big)
        out, ref = run_adv(be, r, v, m, f), pb.reference_advantages(r, v, m, f)
        exp = (m != 0) & (f != 0)
        if not exp.any():
            assert same_bits(out["stats"], np.zeros(2))
            continue
        a = (r.astype(np.float64) - v[:T].astype(np.float64))[exp]
        mean, std = out["stats"]
        print("T %d N %d big %d: mean err %.3e (bound %.3e), std err %.3e (bound %.3e)" % (T, N, big, abs(mean - np.mean(a)), 1e-12 * np.mean(np.abs(a)),
                                                                                         abs(std - np.std(a)), 1e-12 * np.std(a)))
        assert (ref["stats"][0], ref["stats"][1]) == (np.mean(a), np.std(a))
        assert abs(mean - np.mean(a)) <= 1e-12 * np.mean(np.abs(a))
        assert abs(std - np.std(a)) <= 1e-12 * np.std(a)
        if big:
            assert 999.0 < mean < 1001.0 and (a.size < 8 or 1e-4 < std < 1e-2)


def check_advantages_and_targets(be, T, N):
    r, v, m, f = make_inputs(T, N, seed=2)
    for vmin, vmax in ((-0.3, 0.7), (-np.inf, np.inf), (-np.inf, 0.1)):
        out = run_adv(be, r, v, m, f, clip=1.0, vmin=vmin, vmax=vmax)
        ref = pb.reference_advantages(r, v, m, f, norm_adv_clip=1.0, val_min=vmin, val_max=vmax)
        exp = ((m != 0) & (f != 0))
        want = ref["adv"].astype(np.float32)
        assert out["adv"].dtype == np.float32 and (out["adv"][~exp] == 0).all() and not np.signbit(out["adv"][~exp]).any()
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(out["adv"])))
        assert (np.abs(out["adv"].astype(np.float64) - want.astype(np.float64)) <= ulp)[exp].all()
        clipped = exp & (np.abs(ref["adv"]) == 1.0)
        assert same_bits(out["adv"][clipped], want[clipped])
        if T * N >= 320:
            assert 0.2 < clipped.sum() / exp.sum() < 0.45           # |z| > 1: about a third of the samples clip
        assert same_bits(out["targets"], np.clip(r, vmin, vmax).astype(np.float32))
        assert same_bits(out["targets"], ref["targets"].astype(np.float32))
        if np.isinf(vmin) and np.isinf(vmax):
            assert same_bits(out["targets"], r)


def check_determinism(be, T, N):
    r, v, m, f = make_inputs(T, N, seed=3)
    a, b = run_adv(be, r, v, m, f), run_adv(be, r, v, m, f)
    for k in a:
        assert same_bits(a[k], b[k]), k


def run_gather(be, idx, count, first, rows, seed, epoch, srcs, off=0, want_picked=True):
    """srcs: host arrays [n, width]; returns (dst host arrays [rows + 1, width] -- the last row is the guard --, picked)"""
    d_idx, d_count = be.put(np.asarray(idx, np.int32)), be.put(np.array([SENT, count, SENT], np.int32))
    d_src = [be.put(s, off) for s in srcs]
    d_dst = [be.put(np.full((rows + 1, s.shape[1]), SENT, s.dtype), off) for s in srcs]
    d_pick = be.put(np.full(rows + 1, SENT, np.int32))
    pb.gather_device(be.ptr(d_idx), be.ptr(d_count) + 4, first, rows, seed, epoch, [(be.ptr(s), be.ptr(d), s.shape[1]) for s, d in zip(d_src, d_dst)],
                     picked_ptr=be.ptr(d_pick) if want_picked else 0, stream=be.stream, lib_path=be.lib)
    return [be.get(d) for d in d_dst], be.get(d_pick)


def check_permutation(be, count):
    ident, dummy = np.arange(count, dtype=np.int32), [np.arange(count, dtype=np.int32).reshape(count, 1)]
    seen = {}
    for seed, epoch, first in ((1, 0, 0), (1, 1, 0), (2, 0, 0), (1, 0, count)):
        dst, picked = run_gather(be, ident, count, first, count, seed, epoch, dummy)
        p = picked[:count]
        assert picked[count] == SENT and sorted(p.tolist()) == list(range(count))
        assert (p == pb.reference_permutation(count, seed, epoch, first // count)).all()
        assert (dst[0][:count, 0] == p).all()
        seen[(seed, epoch, first)] = p
    if count >= 16:                        # (below that two shuffles may well coincide: 1 / count! is not small)
        base = seen[(1, 0, 0)]
        assert (base != seen[(1, 1, 0)]).any() and (base != seen[(2, 0, 0)]).any() and (base != seen[(1, 0, count)]).any()
    big = ((0x9E3779B9 << 32) | 0x7F4A7C15, 0xFFFFFFFF)            # a seed with a high word, the last epoch
    dst, picked = run_gather(be, ident, count, 0, count, big[0], big[1], dummy)
    assert (picked[:count] == pb.reference_permutation(count, big[0], big[1], 0)).all()


GATHER_WIDTHS = (1, 3, 4, 227, 228)


def check_gather(be, off):
    n, count = 5 * 65, 201
    rng = np.random.default_rng(7)
    idx = np.sort(rng.choice(n, size=count, replace=False)).astype(np.int32)
    srcs = [rng.standard_normal((n, w)).astype(np.float32) if k % 2 == 0 else rng.integers(-2 ** 31, 2 ** 31 - 1, size=(n, w)).astype(np.int32)
            for k, w in enumerate(GATHER_WIDTHS)]
    for first in (0, count - 1, 3 * count + 2):
        for rows in (1, 63, 64, 65, 300):
            dst, picked = run_gather(be, idx, count, first, rows, 5, 2, srcs, off=off)
            want = pb.reference_gather_rows(idx, count, first, rows, 5, 2)
            assert (picked[:rows] == want).all() and picked[rows] == SENT, (first, rows)
            for s, d in zip(srcs, dst):
                assert same_bits(d[:rows], s[want]), (first, rows, s.shape, s.dtype)
                assert (d[rows].view(np.int32) == np.array(SENT, s.dtype).view(np.int32)).all(), "guard row"
    # an empty list: nothing is copied, picked = -1
    dst, picked = run_gather(be, idx, 0, 3, 65, 5, 2, srcs, off=off)
    assert (picked[:65] == -1).all() and picked[65] == SENT
    for s, d in zip(srcs, dst):
        assert (d.view(np.int32) == np.array(SENT, s.dtype).view(np.int32)).all()
    # picked_out is optional
    dst, picked = run_gather(be, idx, count, 7, 65, 5, 2, srcs, off=off, want_picked=False)
    want = pb.reference_gather_rows(idx, count, 7, 65, 5, 2)
    assert (picked == SENT).all() and all(same_bits(d[:65], s[want]) for s, d in zip(srcs, dst))


# ---- the emulator library, host addresses

def test_shapes_cover_three_partial_groups(emu_lib):
    per_group = pb.workspace_bytes(1, 1, emu_lib)
    assert pb.workspace_bytes(33, 130, emu_lib) // per_group >= 3 and pb.workspace_bytes(4, 256, emu_lib) == per_group and pb.workspace_bytes(4, 257, emu_lib) == 2 * per_group


@pytest.mark.parametrize("T,N", SHAPES)
def test_counts_and_lists_emulator(emu_lib, T, N):
    check_counts_and_lists(Emu(emu_lib), T, N)


@pytest.mark.parametrize("T,N", SHAPES)
def test_statistics_emulator(emu_lib, T, N):
    check_statistics(Emu(emu_lib), T, N)


@pytest.mark.parametrize("T,N", SHAPES)
def test_advantages_and_targets_emulator(emu_lib, T, N):
    check_advantages_and_targets(Emu(emu_lib), T, N)


@pytest.mark.parametrize("T,N", [(5, 65), (33, 130)])
def test_determinism_emulator(emu_lib, T, N):
    check_determinism(Emu(emu_lib), T, N)


@pytest.mark.parametrize("count", PERM_COUNTS)
def test_permutation_emulator(emu_lib, count):
    check_permutation(Emu(emu_lib), count)


@pytest.mark.parametrize("off", [0, 1])
def test_gather_emulator(emu_lib, off):
    check_gather(Emu(emu_lib), off)


def test_reference_permutation_is_uniform():
    """the Python statement alone, fixed inputs: every (position, value) cell within 4 standard deviations of its binomial expectation.  An honest uniform shuffle
    exceeds 4 in one of 49 cells with probability about 0.3 %; the construction gives 1.82 (count 5) and 2.49 (count 7) with its 6 rounds and 10.4 with 4."""
    def worst(count, nseeds, rounds=6):
        perms = pb.reference_permutation(count, (99 << 32) | np.arange(nseeds, dtype=np.uint64), 3, 0x50504F, rounds)
        assert (np.sort(perms, axis=1) == np.arange(count)).all()
        p = 1.0 / count
        cells = np.array([[(perms[:, pos] == val).sum() for val in range(count)] for pos in range(count)])
        return float(np.abs(cells - nseeds * p).max() / np.sqrt(nseeds * p * (1 - p)))
    z5, z7, z5_4 = worst(5, 4000), worst(7, 4096), worst(5, 4000, rounds=4)
    print("worst cell in standard deviations: count 5: %.2f, count 7: %.2f, count 5 with 4 rounds: %.2f" % (z5, z7, z5_4))
    assert z5 < 4.0 and z7 < 4.0
    assert z5_4 > 4.0                      # (the test can tell: four rounds are visibly non-uniform)


def test_reference_permutation_is_a_bijection():
    for count in list(range(1, 70)) + [255, 256, 257, 1000, 4097]:
        assert sorted(pb.reference_permutation(count, 11, 1, 2).tolist()) == list(range(count))


def test_refusals_emulator(emu_lib):
    """host addresses that are never dereferenced: every call is refused before a launch"""
    from deepmimic_amd.core import load_library
    lib = load_library(emu_lib)
    f, i, d = np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(64, np.float64)
    adv, idx = np.full(64, 7.0, np.float32), np.full(64, SENT, np.int32)
    good = dict(T=2, N=4, returns_ptr=f.ctypes.data, values_ptr=f.ctypes.data, mask_ptr=i.ctypes.data, exp_flags_ptr=i.ctypes.data, adv_eps=1e-5, norm_adv_clip=5.0,
                val_min=-1.0, val_max=1.0, adv_ptr=adv.ctypes.data, targets_ptr=adv.ctypes.data, valid_idx_ptr=idx.ctypes.data, exp_idx_ptr=idx.ctypes.data,
                counts_ptr=idx.ctypes.data, stats_ptr=d.ctypes.data, workspace_ptr=d.ctypes.data, workspace_nbytes=pb.workspace_bytes(2, 4, emu_lib), lib_path=emu_lib)
    bad = [dict(T=0), dict(N=0), dict(T=-3), dict(T=65536, N=32768), dict(returns_ptr=0), dict(values_ptr=0), dict(adv_ptr=0), dict(targets_ptr=0), dict(valid_idx_ptr=0),
           dict(exp_idx_ptr=0), dict(counts_ptr=0), dict(stats_ptr=0), dict(workspace_ptr=0), dict(workspace_nbytes=good["workspace_nbytes"] - 1), dict(adv_eps=-1e-9),
           dict(norm_adv_clip=0.0), dict(norm_adv_clip=-1.0), dict(val_min=1.0, val_max=0.5), dict(adv_eps=float("nan")), dict(T=3, N=400)]      # (last: 2 groups' workspace)
    for b in bad:
        with pytest.raises(RuntimeError, match="dm_ppo_"):
            pb.advantages_device(**dict(good, **b))
        assert b"dm_ppo_" in lib.dm_last_error()
    assert (adv == 7.0).all() and (idx == SENT).all()           # nothing was launched
    for T, N in ((0, 4), (4, 0), (65536, 32768)):
        with pytest.raises(RuntimeError, match="dm_ppo_workspace_bytes"):
            pb.workspace_bytes(T, N, emu_lib)
    assert pb.workspace_bytes(32768, 65535, emu_lib) > 0           # 2^31 - 32768 samples: the largest shapes are taken
    src, dst = np.zeros(64, np.float32), np.full(64, 7.0, np.float32)
    col = (src.ctypes.data, dst.ctypes.data, 2)
    ggood = dict(idx_ptr=i.ctypes.data, count_ptr=i.ctypes.data, first=0, rows=4, seed=1, epoch=0, columns=[col], picked_ptr=idx.ctypes.data, lib_path=emu_lib)
    gbad = [dict(idx_ptr=0), dict(count_ptr=0), dict(first=-1), dict(rows=0), dict(rows=-5), dict(columns=[]), dict(columns=[col] * 9), dict(columns=[(col[0], col[1], 0)]),
            dict(columns=[(col[0], col[1], -2)]), dict(columns=[(0, col[1], 2)]), dict(columns=[col, (col[0], 0, 2)])]
    for b in gbad:
        with pytest.raises(RuntimeError, match="dm_ppo_gather"):
            pb.gather_device(**dict(ggood, **b))
        assert b"dm_ppo_gather" in lib.dm_last_error()
    assert (dst == 7.0).all() and (idx == SENT).all()


# ---- the HIP library, torch tensors

@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_counts_and_lists_gpu(hip_lib, T, N):
    check_counts_and_lists(Gpu(hip_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_statistics_gpu(hip_lib, T, N):
    check_statistics(Gpu(hip_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_advantages_and_targets_gpu(hip_lib, T, N):
    check_advantages_and_targets(Gpu(hip_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(5, 65), (33, 130)])
def test_determinism_gpu(hip_lib, T, N):
    check_determinism(Gpu(hip_lib), T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("count", PERM_COUNTS)
def test_permutation_gpu(hip_lib, count):
    check_permutation(Gpu(hip_lib), count)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
def test_gather_gpu(hip_lib, off):
    check_gather(Gpu(hip_lib), off)


@pytest.mark.gpu
def test_torch_binding_equals_the_raw_call_and_checks_its_tensors(hip_lib):
    import torch
    T, N = 5, 65
    r, v, m, f = make_inputs(T, N, seed=4)
    raw = run_adv(Gpu(hip_lib), r, v, m, f, clip=1.0, vmin=-0.5, vmax=0.5)
    tr, tv, tm, tf = (torch.from_numpy(x).cuda() for x in (r, v, m, f))
    for values in (tv, tv[:T].contiguous()):
        b = pb.advantages_torch(tr, values, tm, tf, norm_adv_clip=1.0, val_min=-0.5, val_max=0.5, lib_path=hip_lib)
        nv, ne = b.counts_host()
        assert (nv, ne) == tuple(raw["counts"]) and same_bits(b.adv.cpu().numpy(), raw["adv"]) and same_bits(b.targets.cpu().numpy(), raw["targets"])
        assert same_bits(b.stats.cpu().numpy(), raw["stats"])
        assert same_bits(b.valid_idx[:nv].cpu().numpy(), raw["valid_idx"][:nv]) and same_bits(b.exp_idx[:ne].cpu().numpy(), raw["exp_idx"][:ne])
    none = pb.advantages_torch(tr, tv, lib_path=hip_lib)
    assert none.counts_host() == (T * N, T * N)
    for bad in (dict(returns=tr.double()), dict(values=tv[:T - 1].contiguous()), dict(mask=tm.float()), dict(exp_flags=tf.cpu()), dict(mask=tm.t().contiguous().t())):
        with pytest.raises(ValueError):
            pb.advantages_torch(**dict(dict(returns=tr, values=tv, mask=tm, exp_flags=tf), **bad), lib_path=hip_lib)
    obs = torch.randn((T, N, 3, 2), device="cuda")
    rows, ids, picked = b.gather("exp", 2, 70, 9, 1, obs, tm, picked=True)
    want = pb.reference_gather_rows(raw["exp_idx"], ne, 2, 70, 9, 1)
    assert rows.shape == (70, 3, 2) and ids.shape == (70,) and (picked.cpu().numpy() == want).all()
    assert same_bits(rows.cpu().numpy(), obs.reshape(T * N, 3, 2).cpu().numpy()[want]) and (ids == 1).all()
    for bad in ((obs.double(),), (obs[:, :10],), (obs[:T - 1],), ()):
        with pytest.raises(ValueError):
            b.gather("exp", 0, 4, 9, 1, *bad)
    with pytest.raises(ValueError):
        b.gather("all", 0, 4, 9, 1, obs)


@pytest.mark.gpu
def test_rollout_to_minibatches_end_to_end_gpu(hip_lib):
    """TorchVecEnv rollout (walk, 64 envs, 8 steps, episode timers of 0.1 .. 0.2 s) under the random-weights actor with exp_rate 0.5 and a random critic ->
    critic_returns_torch -> advantages_torch -> one epoch of minibatches of 32: every actor row is an explored, valid sample; the critic rows of the epoch are
    exactly the valid set; the actor's adv column is adv at the rows it was picked from"""
    import torch
    from deepmimic_amd import model, returns
    from deepmimic_amd.heads import Critic
    from deepmimic_amd.policy import Policy, random_weights
    from deepmimic_amd.vec_env import TorchVecEnv
    from test_scalar_heads import random_scalar_net
    T, N, M = 8, 64, 32
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), N, seed=3, lib_path=hip_lib)
    env.env.set_time_limits(0.1, 0.2)
    S, A = env.obs_dim, env.act_dim
    actor = Policy(random_weights(S, A, seed=4), lib_path=hip_lib)
    critic = Critic(random_scalar_net(S, seed=5, scale=1.0), val_fail=0.0, val_succ=20.0, lib_path=hip_lib)
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    obs_all, tobs = torch.zeros((T + 1, N, S), **f32), torch.zeros((T, N, S), **f32)
    acts, logp, rewards = torch.zeros((T, N, A), **f32), torch.zeros((T, N), **f32), torch.zeros((T, N), **f32)
    flags, terminate, done, valid = (torch.zeros((T, N), **i32) for _ in range(4))
    stream = int(torch.cuda.current_stream().cuda_stream)
    obs = env.reset()
    for t in range(T):
        obs_all[t] = obs
        actor.forward_device_ex(obs.data_ptr(), N, acts[t].data_ptr(), logp_ptr=logp[t].data_ptr(), exp_flags_ptr=flags[t].data_ptr(), exp_rate=0.5, sample=True,
                                seed=21, step=t, stream=stream)
        obs, r, d, info = env.step(acts[t])
        rewards[t], terminate[t], done[t], valid[t], tobs[t] = r, info["terminate"], d.to(torch.int32), info["valid"], info["terminal_obs"]
    obs_all[T] = obs
    ret, mask, values = returns.critic_returns_torch(critic, obs_all, None, tobs, None, terminate, done, valid, rewards, 0.95, 0.95, lib_path=hip_lib, return_values=True)
    batch = pb.advantages_torch(ret, values, mask, flags, lib_path=hip_lib)
    n_valid, n_exp = batch.counts_host()
    h_mask, h_flags, h_adv = mask.cpu().numpy().reshape(-1), flags.cpu().numpy().reshape(-1), batch.adv.cpu().numpy().reshape(-1)
    assert n_valid == int((h_mask != 0).sum()) and n_exp == int(((h_mask != 0) & (h_flags != 0)).sum()) and 0 < n_exp < n_valid
    ref = pb.reference_advantages(ret.cpu().numpy(), values.cpu().numpy(), mask.cpu().numpy(), flags.cpu().numpy())
    want = ref["adv"].reshape(-1).astype(np.float32)
    assert (np.abs(h_adv.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(want), np.abs(h_adv)))).all()           # one fp32 ulp, as in the unit tests
    obs_rows, act_rows = obs_all[:T], acts
    critic_seen, batches = [], 0
    for e, b, (c_obs, c_tar, c_pick), (a_obs, a_act, a_logp, a_adv, a_pick) in batch.minibatches(M, 1, 17, [obs_rows, batch.targets], [obs_rows, act_rows, logp, batch.adv],
                                                                                                 picked=True):
        cp, ap = c_pick.cpu().numpy(), a_pick.cpu().numpy()
        assert c_obs.shape == (M, S) and a_act.shape == (M, A) and a_adv.shape == (M,)
        assert (h_mask[ap] != 0).all() and (h_flags[ap] != 0).all() and (h_mask[cp] != 0).all()
        assert same_bits(a_adv.cpu().numpy(), h_adv[ap]) and same_bits(a_logp.cpu().numpy(), logp.cpu().numpy().reshape(-1)[ap])
        assert same_bits(a_obs.cpu().numpy(), obs_rows.reshape(T * N, S).cpu().numpy()[ap]) and same_bits(a_act.cpu().numpy(), acts.reshape(T * N, A).cpu().numpy()[ap])
        assert same_bits(c_tar.cpu().numpy(), batch.targets.cpu().numpy().reshape(-1)[cp]) and same_bits(c_obs.cpu().numpy(), obs_rows.reshape(T * N, S).cpu().numpy()[cp])
        assert (cp == pb.reference_gather_rows(ref["valid_idx"], n_valid, b * M, M, 17, e)).all() and (ap == pb.reference_gather_rows(ref["exp_idx"], n_exp, b * M, M, 17, e)).all()
        critic_seen.append(cp); batches += 1
    assert batches == -(-n_valid // M)
    assert sorted(set(np.concatenate(critic_seen).tolist())) == np.flatnonzero(h_mask != 0).tolist()
    actor.close(); critic.close(); env.close()
