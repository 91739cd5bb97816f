"""The device normaliser (deepmimic_amd/csrc/dm_norm.h) at the shapes its index arithmetic branches on; tests/test_normalizer.py replays the
reference's golden vectors, which all fit the first branch of almost every index computation (one workgroup of k_norm_apply, at most 19 slabs of 16
rows in k_norm_partial, one pass of the 256 threads over the columns).  Here, on the CPU emulator build and, under -m gpu, on the GPU:
 * normalize: more than one workgroup with a moving column phase, a tail in the last workgroup, wraps inside a quad (size < 4), pointers that are not
   16-byte aligned (the scalar path), the last width whose statistics are staged in LDS and the first that is not.  The kernel is (x - mean_f) *
   inv_std_f and two compares in fp32, which no compiler contracts into an FMA: the numpy float32 expression is its result to the bit.
 * record: 1 .. 16385 rows (rows_per_group 16 and 17, a short last slab, more than 64 slabs so that a fold lane adds several partials, a second pass
   over the columns) and small calls after large ones (stale partials behind the slab count).  With x = k / 1024, |k| <= 2^16, every partial sum of x
   and of x^2 in any order is an exact fp64 number, so `pending` equals the integer sums to the bit; with ordinary data the any-order bound holds.
 * update: 600 columns (a thread owns up to three columns, group members in other threads' later passes), every kind of group id.
 * the element limit of one normalize call, and the stream a call is ordered on."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from normalizer_oracle import NormalizerOracle       # noqa: E402

from deepmimic_amd.normalizer import DeviceNormalizer  # noqa: E402

SENTINEL = np.float32(-777.25)
GUARD = 8                                 # elements of the output buffer checked in front of and behind the result


# ---- device memory of either build: numpy arrays on the emulator (a device pointer is a host address), torch tensors on the GPU
def _ptr(b):
    return b.data_ptr() if hasattr(b, "data_ptr") else b.ctypes.data


def _sync(on_gpu):
    if on_gpu:
        import torch
        torch.cuda.synchronize()


def _dev(a, on_gpu):
    a = np.ascontiguousarray(a)
    if on_gpu:
        import torch
        return torch.from_numpy(a).cuda()
    return a


def _host(b):
    if hasattr(b, "data_ptr"):
        import torch
        torch.cuda.synchronize()
        return b.cpu().numpy()
    return b.copy()


def _flat(on_gpu, nelem, fill):
    """a flat float32 buffer of at least `nelem` elements behind `lead`, the index of its first 16-byte aligned element"""
    if on_gpu:
        import torch
        buf = torch.full((nelem + 4,), float(fill), dtype=torch.float32, device="cuda")
    else:
        buf = np.full(nelem + 4, fill, np.float32)
    assert _ptr(buf) % 4 == 0
    return buf, ((-_ptr(buf)) % 16) // 4


def _read_pending(nrm, on_gpu):
    ptr, n = nrm.pending_ptr()
    assert n == 1 + 2 * nrm.size
    if on_gpu:
        import torch
        hip = C.CDLL("libamdhip64.so")
        cur = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert hip.hipMemcpy(C.c_void_p(cur.data_ptr()), C.c_void_p(ptr), C.c_size_t(8 * n), 3) == 0       # (3 = hipMemcpyDeviceToDevice)
        torch.cuda.synchronize()
        return cur.cpu().numpy()
    return np.ctypeslib.as_array((C.c_double * n).from_address(ptr)).copy()


def _fp32_statement(x, mean, std, clip):
    """what k_norm_apply computes, in numpy float32: mean_f = (float)mean, inv_std_f = (float)(1.0 / std), one subtraction, one product, two compares"""
    mf, sf = np.asarray(mean, np.float64).astype(np.float32), (1.0 / np.asarray(std, np.float64)).astype(np.float32)
    want = np.clip((x - mf) * sf, np.float32(-clip), np.float32(clip))
    assert want.dtype == np.float32 and not np.isnan(want).any()
    return want


def _check_apply(nrm, x, mean, std, clip, on_gpu, x_off=0, out_off=0):
    """normalize x [n x size] read at `x_off` and written at `out_off` floats past a 16-byte boundary: bit-equal to the fp32 statement, and not one
    element written in front of or behind the n x size results"""
    n, total = x.shape[0], x.size
    xb, xl = _flat(on_gpu, total + 4, 0.0)
    xs = xl + x_off
    xb[xs:xs + total] = _dev(x.ravel(), on_gpu)
    ob, ol = _flat(on_gpu, total + 2 * GUARD + 8, SENTINEL)
    os_ = ol + GUARD + out_off                                 # (GUARD floats are 32 bytes: the alignment of `ol` is kept)
    assert _ptr(xb[xs:]) % 16 == 4 * x_off and _ptr(ob[os_:]) % 16 == 4 * out_off
    _sync(on_gpu)
    nrm.normalize_device(_ptr(xb[xs:]), n, _ptr(ob[os_:]))
    got = _host(ob)
    assert os_ >= GUARD and got.size - (os_ + total) >= GUARD
    assert (got[:os_] == SENTINEL).all() and (got[os_ + total:] == SENTINEL).all(), "normalize wrote outside its n x size elements"
    want = _fp32_statement(x, mean, std, clip)
    assert np.array_equal(got[os_:os_ + total].view(np.uint32), want.ravel().view(np.uint32)), \
        (x.shape, x_off, out_off, np.flatnonzero(got[os_:os_ + total] != want.ravel())[:8])


def _apply_case(rng, size, n, clip):
    """mean, std and an [n x size] block with a few elements exactly on the clip boundary and a few far outside it (no NaN, no overflow)"""
    mean, std = rng.normal(size=size), 0.5 + rng.random(size)
    x = (rng.normal(size=(n, size)) * 2.0 * std + mean).astype(np.float32)
    c = clip if np.isfinite(clip) else 5.0
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=min(16, flat.size), replace=False)
    for j, i in enumerate(idx):
        col = i % size
        flat[i] = (np.float32(mean[col] + c * std[col]), np.float32(mean[col] - c * std[col]), np.float32(1e6), np.float32(-1e6),
                   np.float32(1e30), np.float32(-1e30), np.float32(0.0), np.float32(mean[col]))[j % 8]
    return mean, std, x


# ---- 1. normalize, bit-equal to its fp32 statement
# size x n: a workgroup owns 4096 floats
APPLY_SHAPES = (
    (227, 19, 5.0),        # 4313 floats: workgroup 1 starts at column 4096 % 227 = 10; total % 4 = 1
    (227, 37, np.inf),     # three workgroups, unclipped
    (1, 4099, 5.0),        # one column: the phase wraps at every element
    (3, 2731, 5.0),        # 8193 floats: a one-element tail in a third workgroup, a wrap or two inside every quad
    (5, 1639, 5.0),        # 8195 floats: a three-element tail
    (7, 1171, 5.0),        # 8197 floats
    (2048, 3, 5.0),        # the widest row whose statistics are staged in LDS
    (2049, 3, 5.0),        # the narrowest that reads them from global memory
    (4096, 2, 5.0),        # a row is a whole workgroup
    (96, 128, 5.0),        # 12288 floats = exactly three workgroups (no tail), the phase moves by 4096 % 96 = 64 per workgroup
    (2, 3, 5.0),           # six floats: one full quad and a tail of two in the first workgroup
)
# floats past a 16-byte boundary of (x, out): the 16-byte loads and stores are taken only when both are 0
ALIGNMENTS = ((0, 0), (1, 0), (0, 1), (3, 3))


def _normalize_shapes(lib, on_gpu):
    rng = np.random.default_rng(11)
    for size, n, clip in APPLY_SHAPES:
        mean, std, x = _apply_case(rng, size, n, clip)
        nrm = DeviceNormalizer(size, None, eps=0.02, clip=clip, lib_path=lib)
        nrm.set_mean_std(mean, std)
        _check_apply(nrm, x, mean, std, clip, on_gpu)
        nrm.close()


def _normalize_alignments(lib, on_gpu):
    rng = np.random.default_rng(12)
    for size, n in ((7, 1171), (227, 19), (3, 2731)):
        mean, std, x = _apply_case(rng, size, n, 5.0)
        nrm = DeviceNormalizer(size, None, eps=0.02, clip=5.0, lib_path=lib)
        nrm.set_mean_std(mean, std)
        for x_off, out_off in ALIGNMENTS:
            _check_apply(nrm, x, mean, std, 5.0, on_gpu, x_off, out_off)
        nrm.close()


def test_normalize_bit_equal_at_every_index_branch_emulator(emu_lib):
    _normalize_shapes(emu_lib, False)


@pytest.mark.gpu
def test_normalize_bit_equal_at_every_index_branch_gpu(hip_lib):
    _normalize_shapes(hip_lib, True)


def test_normalize_unaligned_pointers_and_guards_emulator(emu_lib):
    _normalize_alignments(emu_lib, False)


@pytest.mark.gpu
def test_normalize_unaligned_pointers_and_guards_gpu(hip_lib):
    _normalize_alignments(hip_lib, True)


# ---- 2. / 3. record
# size -> the row counts recorded one after another into one handle.  nb = min(ceil(n / 16), 1024) slabs of ceil(n / nb) rows:
RECORD_SHAPES = (
    (3, (1, 15, 16, 17, 1023, 1024, 1025)),      # one short slab .. 65 slabs (fold lane 0 adds a second partial), the last one of a single row
    (5, (16384, 16385, 7, 16384)),               # 1024 slabs of 16; 964 slabs of 17, the last one of 14; one slab in front of 1023 stale ones; again
    (257, (70, 1040, 70)),                       # a second pass over the columns for thread 0; 65 slabs, then 5 in front of 60 stale ones
    (300, (70, 1040, 70)),
)
ROUTES = ("host", "device")


def _record(nrm, x, route, on_gpu, keep):
    if route == "host":
        nrm.record(x)
    else:
        xd = _dev(x, on_gpu); keep.append(xd)                # (the launch is asynchronous: the block lives until the pending sums are read)
        _sync(on_gpu)
        nrm.record_device(_ptr(xd), x.shape[0])


def _record_exact(lib, on_gpu, size, counts, route):
    """x = k / 1024 with integer |k| <= 2^16 is exact in fp32, sum x = sum k / 2^10 and sum x^2 = sum k^2 / 2^20 with numerators below 2^53 for up to
    50 000 rows: every partial sum is exact in fp64 in whatever order it is formed, so `pending` is the int64 sums, bit for bit"""
    assert sum(counts) <= 50000
    rng = np.random.default_rng(21 + size)
    nrm = DeviceNormalizer(size, None, lib_path=lib)
    keep, rows, sk, sk2 = [], 0, np.zeros(size, np.int64), np.zeros(size, np.int64)
    for n in counts:
        k = rng.integers(-2 ** 16, 2 ** 16 + 1, size=(n, size), dtype=np.int64)
        x = (k / 1024.0).astype(np.float32)
        assert np.array_equal(x.astype(np.float64) * 1024.0, k)
        _record(nrm, x, route, on_gpu, keep)
        rows += n; sk += k.sum(0); sk2 += (k * k).sum(0)
        assert np.abs(sk).max() < 2 ** 53 and sk2.max() < 2 ** 53
        p = _read_pending(nrm, on_gpu)
        assert p[0] == rows, n
        assert np.array_equal(p[1:1 + size], sk.astype(np.float64) / 2.0 ** 10), (n, "sum")
        assert np.array_equal(p[1 + size:], sk2.astype(np.float64) / 2.0 ** 20), (n, "sum of squares")
    nrm.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("size,counts", RECORD_SHAPES, ids=[str(s) for s, _ in RECORD_SHAPES])
def test_record_exact_sums_in_any_order_emulator(emu_lib, size, counts, route):
    _record_exact(emu_lib, False, size, counts, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("size,counts", RECORD_SHAPES, ids=[str(s) for s, _ in RECORD_SHAPES])
def test_record_exact_sums_in_any_order_gpu(hip_lib, size, counts, route):
    _record_exact(hip_lib, True, size, counts, route)


def _fsum_columns(blocks):
    """exact column sums, correctly rounded (math.fsum), of x, |x| and x^2 (v * v of an fp32 value is exact in fp64) over the rows of all blocks"""
    a = np.concatenate(blocks).astype(np.float64)
    s = np.array([math.fsum(col) for col in a.T])
    sa = np.array([math.fsum(col) for col in np.abs(a).T])
    q = np.array([math.fsum(col) for col in (a * a).T])
    return s, sa, q


def _record_bounded(lib, on_gpu, size, counts):
    """ordinary data: a sum of N fp64 numbers formed in any order differs from the exact one by at most (N - 1) u sum |x| to first order, u = 2^-53
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); the kernel's addends are (double)x and its exact square, so N u sum |x| and
    N u sum x^2 bound the two halves of `pending` (N the rows recorded so far), the rounding of the fsum reference included.  Two handles fed the
    same blocks agree bit for bit (the header's "deterministic"): one fresh through record_device(), one through record() whose scratch buffers
    were grown by a larger block before"""
    rng = np.random.default_rng(31 + size)
    fresh = DeviceNormalizer(size, None, lib_path=lib)
    used = DeviceNormalizer(size, None, lib_path=lib)
    used.record((rng.normal(size=(max(counts) + 33, size)) * 7 + 3).astype(np.float32))
    used.update()
    assert used.count == max(counts) + 33 and not _read_pending(used, on_gpu).any()
    scale, offset = 0.2 + rng.random(size), rng.normal(size=size)
    keep, blocks, u = [], [], 2.0 ** -53
    for n in counts:
        x = (rng.normal(size=(n, size)) * scale + offset).astype(np.float32)
        blocks.append(x)
        _record(fresh, x, "device", on_gpu, keep)
        _record(used, x, "host", on_gpu, keep)
        p, p2 = _read_pending(fresh, on_gpu), _read_pending(used, on_gpu)
        assert np.array_equal(p.view(np.uint64), p2.view(np.uint64)), (n, "the sums depend on the history of the scratch buffers")
        s, sa, q = _fsum_columns(blocks)
        rows = sum(b.shape[0] for b in blocks)
        assert p[0] == rows
        es, eq = np.abs(p[1:1 + size] - s), np.abs(p[1 + size:] - q)
        print("record %d x %d (%d rows pending): max error / bound: sum %.3g, sum of squares %.3g" % (n, size, rows, (es / (rows * u * sa)).max(), (eq / (rows * u * q)).max()))
        assert (es <= rows * u * sa).all(), (n, "sum")
        assert (eq <= rows * u * q).all(), (n, "sum of squares")
    fresh.close(); used.close()


@pytest.mark.parametrize("size,counts", RECORD_SHAPES, ids=[str(s) for s, _ in RECORD_SHAPES])
def test_record_ordinary_data_bounded_and_deterministic_emulator(emu_lib, size, counts):
    _record_bounded(emu_lib, False, size, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("size,counts", RECORD_SHAPES, ids=[str(s) for s, _ in RECORD_SHAPES])
def test_record_ordinary_data_bounded_and_deterministic_gpu(hip_lib, size, counts):
    _record_bounded(hip_lib, True, size, counts)


# ---- 4. update beyond one pass of the block's 256 threads
def _state_bits(nrm):
    return np.concatenate([nrm.mean, nrm.mean_sq, nrm.std, [float(nrm.count)]]).view(np.uint64)


def _update_wide(lib, on_gpu):
    S, n, eps, clip = 600, 33, 0.02, 5.0
    gids = np.zeros(S, np.int32)
    gids[::7] = 9; gids[1::7] = 1000000           # members 7 columns apart: every thread's group reaches into all three passes of the other threads
    none = [5, 599]; gids[none] = -1
    gids[2] = 3                                   # a group of one
    const = [100, 101, 102, 103, 104]             # exactly constant columns
    assert not gids[const].any()
    rng = np.random.default_rng(41)
    x = (rng.normal(size=(n, S)) * (0.2 + rng.random(S)) + rng.normal(size=S)).astype(np.float32)
    x[:, const] = np.float32(0.75)
    q = (rng.normal(size=(40, S)) * 2.0 + rng.normal(size=S)).astype(np.float32)          # 24000 floats: six workgroups of k_norm_apply
    m0, s0 = rng.normal(size=S), 0.5 + rng.random(S)
    # the columns that keep their value: m and q come back as w_old v + w_new v, two roundings each, and std = sqrt(q - m^2) then moves by about
    # u (q + 2 m^2) / (q - m^2) relative, u = 2^-53: 13 u at (-1.25, 0.75), 2 u at (0.5, 1.0), inside 1e-14 without an absolute term
    m0[none] = (0.5, -1.25); s0[none] = (1.0, 0.75)
    for start in ("count 100", "fresh"):
        nrm = DeviceNormalizer(S, gids, eps=eps, clip=clip, lib_path=lib)
        ora = NormalizerOracle(S, gids, eps, clip)
        keep = []
        if start == "count 100":
            nrm.set_mean_std(m0, s0, count=100); ora.set_mean_std(m0, s0); ora.count = 100
            _record(nrm, x, "device", on_gpu, keep)
        else:
            _record(nrm, x, "host", on_gpu, keep)
        ora.record(x)
        nrm.update(); ora.update()
        mean, mean_sq, std, count = nrm.mean, nrm.mean_sq, nrm.std, nrm.count
        assert count == ora.count == (133 if start == "count 100" else 33)
        for name, got, ref in (("mean", mean, ora.mean), ("mean_sq", mean_sq, ora.mean_sq), ("std", std, ora.std)):
            assert np.allclose(got, ref, rtol=1e-12, atol=1e-13), (start, name, np.abs(got - ref).max())
        if start == "count 100":
            assert np.allclose(mean[none], m0[none], rtol=1e-14, atol=0) and np.allclose(std[none], s0[none], rtol=1e-14, atol=0)
        else:                                     # w_old = 0: mean 0 and mean_sq 0 stay, the constant columns have no variance at all
            assert not mean[none].any() and not mean_sq[none].any() and (std[none] == eps).all()
            assert (mean[const] == 0.75).all() and (std[const] == eps).all()
            assert np.unique(mean[::7]).size == 1 and np.unique(mean_sq[1::7]).size == 1          # one average for all members of a group
        assert not _read_pending(nrm, on_gpu).any()
        before = _state_bits(nrm)
        nrm.update()                              # nothing pending: not one bit of the state moves
        assert np.array_equal(_state_bits(nrm), before), start
        _check_apply(nrm, q, mean, std, clip, on_gpu)
        nrm.close()


def test_update_600_columns_every_group_kind_emulator(emu_lib):
    _update_wide(emu_lib, False)


@pytest.mark.gpu
def test_update_600_columns_every_group_kind_gpu(hip_lib):
    _update_wide(hip_lib, True)


# ---- 5. the element limit of one call
def test_normalize_refuses_more_than_int32_elements_emulator(emu_lib):
    """n x size = 2^31 does not fit the kernel's int total: refused before anything is launched (the four-float dummies are not touched)"""
    nrm = DeviceNormalizer(1 << 20, None, lib_path=emu_lib)
    x, out = np.full(4, 1.5, np.float32), np.full(4, SENTINEL, np.float32)
    with pytest.raises(RuntimeError, match="too many elements"):
        nrm.normalize_device(x.ctypes.data, 2048, out.ctypes.data)
    assert (x == 1.5).all() and (out == SENTINEL).all()
    nrm.close()


# ---- 6. the stream a call is ordered on
@pytest.mark.gpu
@pytest.mark.parametrize("first", ("get", "set", "normalize"))
def test_call_on_a_new_stream_sees_the_old_streams_update_gpu(hip_lib, first):
    """record_device() and update() on stream A, then set_stream(B): whichever call comes first on B -- a read of the state, set_mean_std(count=-1),
    which reads the count and writes it back, or normalize_device() -- works on what the update wrote, because every entry point waits for the
    handle's previous stream before it touches the handle's buffers (dm_normalizer::order_on).
    A pass does not prove that ordering: without it the update usually wins the race by luck.  The test pins the result that the ordering guarantees."""
    import torch
    size, n, clip = 5, 16385, 5.0
    rng = np.random.default_rng(61)
    x = (rng.normal(size=(n, size)) * (0.2 + rng.random(size)) + rng.normal(size=size)).astype(np.float32)
    q = (rng.normal(size=(2731, size)) * 2.0).astype(np.float32)
    m0, s0 = rng.normal(size=size), 0.5 + rng.random(size)
    m1, s1 = rng.normal(size=size), 0.5 + rng.random(size)
    ora = NormalizerOracle(size, None, 0.02, clip)
    ora.set_mean_std(m0, s0); ora.count = 100; ora.record(x); ora.update()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    out = torch.full((q.size,), float(SENTINEL), dtype=torch.float32, device="cuda")
    nrm = DeviceNormalizer(size, None, eps=0.02, clip=clip, lib_path=hip_lib)
    nrm.set_stream(sa.cuda_stream)
    nrm.set_mean_std(m0, s0, count=100)
    torch.cuda.synchronize()
    nrm.record_device(xd.data_ptr(), n)
    nrm.update()
    nrm.set_stream(sb.cuda_stream)

    def check_state():
        assert nrm.count == ora.count == 100 + n
        assert np.allclose(nrm.mean, ora.mean, rtol=1e-12, atol=1e-13) and np.allclose(nrm.std, ora.std, rtol=1e-12, atol=1e-13)

    def normalize():
        out.fill_(float(SENTINEL)); torch.cuda.synchronize()
        nrm.normalize_device(qd.data_ptr(), q.shape[0], out.data_ptr())
        sb.synchronize()
        return out.cpu().numpy()

    def check_normalized(got, mean, std):
        assert np.array_equal(got.view(np.uint32), _fp32_statement(q, mean, std, clip).ravel().view(np.uint32))

    if first == "get":
        check_state()
    if first != "set":
        got = normalize()                        # (first == "normalize": the first call on B)
        check_state()
        check_normalized(got, nrm.mean, nrm.std)
    nrm.set_mean_std(m1, s1)                     # count = -1: keeps the count of the update
    assert nrm.count == 100 + n
    assert np.array_equal(nrm.mean, m1) and np.array_equal(nrm.std, s1)
    check_normalized(normalize(), m1, s1)
    torch.cuda.synchronize()
    nrm.close()
