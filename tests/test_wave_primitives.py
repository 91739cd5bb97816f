"""The wave-level primitives at the top of deepmimic_amd/csrc/dm_device.h and dm_device_duo.h, one at a time, through dm_wave_probe (include/dm_hip.h,
deepmimic_amd/csrc/dm_wave_probe.h): ONE dmk:: primitive per launch, every workgroup one wavefront on its own block of the input, in float or in double.

These helpers have two bodies: a plain statement under DM_EMU and, for gfx950, DPP butterflies, v_permlane swaps, inline-asm selects on SGPR lane masks, M0-indexed
register vectors, MFMA chains and v_rcp / v_rsq / v_med3.  Every case runs on the emulator library and, marked gpu, on libdm_hip.so, in both precisions, against plain
numpy written here and evaluated on the inputs AFTER rounding to the primitive's type.  No expected value comes from what a primitive returned.

Data movement (shuffles, broadcasts, selects, chain_keep, RowFile, xd_gram_operands, ballot) is compared as raw bits, over payloads that hold +-0, +-inf, denormals, the
largest finite number and quiet NaNs with a different payload in every lane.  Reductions and Gram matrices are compared bit for bit on integer-valued inputs whose sums are
exact in any order and with any fusing, and against the running bound gamma_k * sum |terms| (the convention of tests/test_math_device.py: gamma_k = k R / (1 - k R), R = u
for float, 2 u for double where the float64 reference rounds as often as the primitive) on random ones.  No case needs an exclusion (`excluded` asserts that).

dm_rcp / dm_rsqrt, float on the device: seed + one Newton step, bound derived at `NEWTON_BOUND`.  Everything else: the correctly rounded division / sqrt.

WHERE THE BODIES DIFFER, and whether a call site can get there (read at the call sites of dm_device.h / dm_device_duo.h):
  * dm_rcp(0) is inf on the emulator and in double, NaN in float on the device (inf * (2 - 0 * inf)); dm_rcp(inf), dm_rsqrt(0), dm_rsqrt(inf) likewise (0 or inf against
    NaN); a float denormal input has a seed the hardware may flush.  The collision code guards every call (`a > 1e-12`, `e > 1e-12`, `denom > 1e-12`, `d2n > 1e-18`).  The
    Cholesky pivots (chol_solve, tree_elim, DuoSim::chol_solve: dm_rsqrt(piv), dm_rsqrt(M), dm_rcp(L_kk)) are unguarded, but a pivot of H = M + dt Kd of a loaded character
    is positive and normal -- lanes past D carry identity rows (pivot 1), M is the total mass -- and a pivot <= 0 is a factorisation that has already failed on either body
    (0 * inf = NaN in the pivot lane on the emulator as well).  Not reachable by a valid state: the domain (finite, normal, > 0; measured over [1e-18, 1e6]) is pinned here,
    the outside is tabulated by `case_outside_domain` and documented as unspecified at the primitives.
  * dm_med3(lo, x, hi) with lo > hi: the median in float on the device, `lo` in double there (fmax(lo, fmin(hi, x))), `lo` or `hi` by x on the emulator.  Every caller passes
    (0, t, 1), (0, t, lim_max_impulse | 1e30) or (-mu ln, t, mu ln) with ln a normal impulse that the same clamp keeps >= 0 and mu >= 0: lo <= hi always.  A NaN x needs a NaN
    state.  Pinned: lo <= hi, x not NaN; the outside is tabulated and unspecified.
  * chain_keep of a dropped value is +0.0 on both bodies, for -0.0, NaN and inf too (checked here, no difference found).
  * wave_gram32 on the float device fills lanes 32..63 with the rows of lanes 0..31 (the callers have at most 32 rows there); the emulator gives them their own rows.  Only
    lanes 0..31 are specified and compared.
  * wave_shfl with a source outside 0..63 takes lane `src & 63` on the emulator; the device (ds_bpermute) is held to the same.
"""
import os
import re

import numpy as np
import pytest

from deepmimic_amd import wave_probe as wp
from deepmimic_amd.core import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepmimic_amd", "csrc")
U = {0: 2.0 ** -24, 1: 2.0 ** -53}
REAL = {0: np.float32, 1: np.float64}
UINT = {0: np.uint32, 1: np.uint64}
R = {0: U[0], 1: 2 * U[1]}              # unit of one rounding against the float64 reference (tests/test_math_device.py)
W, IN, OUT = wp.WAVE, wp.IN, wp.OUT
FILL = -7777.0
LANE = np.arange(W)


def gamma(k, f64):
    return k * R[f64] / (1 - k * R[f64])


def rnd(x, f64):
    return np.asarray(x, np.float64).astype(REAL[f64]).astype(np.float64)


def bits(x, f64):
    """the bit pattern of float64 values that are values of Real"""
    return np.ascontiguousarray(np.asarray(x, np.float64).astype(REAL[f64])).view(UINT[f64])


def ulp(x, f64):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(REAL[f64])).astype(np.float64)


# ---------------------------------------------------------------- plumbing
class Probe:
    """inp [n_waves, 64, <= IN] float64 -> [n_waves, 64, OUT] float64 through dm_wave_probe of `lib_path`; host arrays on the emulator, torch tensors on the GPU"""

    def __init__(self, lib_path, gpu):
        self.lib_path, self.gpu, self.name = lib_path, gpu, "gpu" if gpu else "emulator"

    def __call__(self, op, f64, inp, arg=0, n_waves=None):
        inp = np.asarray(inp, np.float64)
        if n_waves is None:             # (an op that reads nothing is given the grid alone)
            n_waves = inp.shape[0]
            full = np.zeros((n_waves, W, IN))
            full[:, :, :inp.shape[2]] = inp
        else:
            full = np.zeros((1, W, IN))
        if self.gpu:
            import torch
            d_in = torch.from_numpy(full).cuda()
            d_out = torch.full((n_waves, W, OUT), FILL, dtype=torch.float64, device="cuda")
            wp.wave_probe(op, f64, n_waves, d_in.data_ptr(), d_out.data_ptr(), arg=arg, stream=int(torch.cuda.current_stream().cuda_stream), lib_path=self.lib_path)
            torch.cuda.synchronize()
            return d_out.cpu().numpy()
        out = np.full((n_waves, W, OUT), FILL, np.float64)
        wp.wave_probe(op, f64, n_waves, full.ctypes.data, out.ctypes.data, arg=arg, lib_path=self.lib_path)
        return out


def same_bits(probe, f64, what, got, want):
    """got[..., :k] carries the bits of want [..., k]; the columns past k keep the fill"""
    want = np.asarray(want, np.float64)
    k = want.shape[-1]
    g, w = bits(got[..., :k], f64), bits(want, f64)
    bad = g != w
    print("WAVEPRIM %-8s f%d %-40s values %7d  mismatching bits %d" % (probe.name, 64 if f64 else 32, what, w.size, int(bad.sum())))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: (wave, lane, column) %s holds %#x, want %#x (%d of %d differ)" % (what, i, int(g[i]), int(w[i]), int(bad.sum()), w.size))
    assert (got[..., k:] == FILL).all(), "%s: a column past %d was written" % (what, k)


def hold(probe, f64, what, err, bound):
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    assert err.size > 0 and np.isfinite(err).all() and np.isfinite(bound).all() and (bound >= 0).all(), what
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("WAVEPRIM %-8s f%d %-40s values %7d  worst |err| %.3e  worst err/bound %.3f" % (probe.name, 64 if f64 else 32, what, err.size, err.max(), ratio[i]))
    assert ratio[i] <= 1.0, "%s: |err| %.3e > bound %.3e at %s" % (what, err[i], bound[i], i)


def excluded(what, f64, dropped, total):
    """rows a case leaves out because an input sits on a branch threshold: under 1 % (the inputs are chosen so that none is)"""
    print("WAVEPRIM excluded %-32s f%d %d of %d" % (what, 64 if f64 else 32, dropped, total))
    assert dropped <= 0.01 * total, what


def payload(rng, f64, shape):
    """values of Real as float64: random bit patterns (so every lane differs), every 4th slot a special: +-0, +-inf, the largest finite, denormals, and quiet NaNs whose
    payload is the slot's own number.  (Quiet: a conversion may set the quiet bit of a signalling one, which is no fault of a shuffle.)"""
    n = int(np.prod(shape))
    if f64:
        b = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        expo, qbit, sign = np.uint64(0x7ff) << np.uint64(52), np.uint64(1) << np.uint64(51), np.uint64(1) << np.uint64(63)
    else:
        b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        expo, qbit, sign = np.uint32(0xff) << np.uint32(23), np.uint32(1) << np.uint32(22), np.uint32(1) << np.uint32(31)
    one = UINT[f64](1)
    idx = np.arange(n).astype(UINT[f64])
    nan = (b & expo) == expo
    b = np.where(nan, b & ~(one << UINT[f64](52 if f64 else 23)), b)          # random patterns: no NaN / inf by accident (exponent made even)
    kind = np.arange(n) % 64            # (each non-NaN special once per 64 slots: the lanes of a wave still all differ)
    sp = np.arange(n) % 4 == 3
    special = np.select([kind == 3, kind == 11, kind == 19, kind == 27, kind == 35, kind == 43],
                        [UINT[f64](0), sign, expo, expo | sign, expo - one, (idx & UINT[f64](0xffff)) + one],             # +0 -0 +inf -inf max denormal
                        default=expo | qbit | ((idx & UINT[f64](0xfffff)) + one) | np.where(kind % 32 == 31, sign, UINT[f64](0)))      # quiet NaN, payload = slot + 1
    b = np.where(sp, special, b).astype(UINT[f64])
    v = b.view(REAL[f64]).astype(np.float64).reshape(shape)
    assert (bits(v, f64).ravel() == b).all()            # widening and narrowing back keep every pattern, NaN payloads included
    return v


def lanes_differ(v):
    """[nw, 64] payload columns: within a wave no two lanes hold the same bits (a shuffle from the wrong lane cannot pass)"""
    b = np.ascontiguousarray(v).view(np.uint64)
    return all(len(set(row.tolist())) == W for row in b.reshape(-1, W))


# ---------------------------------------------------------------- data movement
def case_wave_shfl(probe, f64):
    rng = np.random.default_rng(1)
    src = np.concatenate([rng.integers(0, 64, (6, W)), np.tile((LANE + 1) % 64, (1, 1)), np.tile(63 - LANE, (1, 1)),
                          rng.integers(-4096, 4096, (4, W)), np.tile(np.array([-1, 64, 65, 127, -64, -65, 128, 1000] * 8), (1, 1))])
    nw = len(src)
    v = payload(rng, f64, (nw, W))
    assert lanes_differ(v)
    out = probe("WAVE_SHFL", f64, np.stack([v, src.astype(np.float64)], axis=2))
    same_bits(probe, f64, "wave_shfl(v, src & 63)", out, np.take_along_axis(v, src & 63, axis=1)[..., None])


def case_bcast(probe, f64):
    rng = np.random.default_rng(2)
    nw = 4
    v = payload(rng, f64, (nw, W))
    assert lanes_differ(v)
    srcs = np.stack([np.arange(63), 63 - np.arange(63), rng.integers(0, 64, 63), np.full(63, 63)])
    inp = np.zeros((nw, W, 64))
    inp[:, :, 0] = v
    inp[:, 0, 1:64] = srcs
    out = probe("LANE_BCAST", f64, inp)
    same_bits(probe, f64, "lane_bcast(v, src)", out, np.broadcast_to(np.stack([v[w, srcs[w]] for w in range(nw)])[:, None, :], (nw, W, 63)))
    srcs = np.stack([np.arange(63) % 32, 31 - np.arange(63) % 32, rng.integers(0, 32, 63), np.full(63, 31)])
    inp[:, 0, 1:64] = srcs
    out = probe("HALF_BCAST", f64, inp)
    want = np.stack([np.stack([v[w, 32 * (l // 32) + srcs[w]] for l in range(W)]) for w in range(nw)])
    same_bits(probe, f64, "half_bcast(v, src, half)", out, want)


def case_half_bcast_c(probe, f64):
    """every lane of a half receives lane SRC of ITS half, for all 32 SRC (15 | 16 and 31 are the seams of the DPP / permlane16 paths); the halves hold different data"""
    rng = np.random.default_rng(3)
    v = payload(rng, f64, (8, W))
    assert lanes_differ(v)
    out = probe("HALF_BCAST_C", f64, v[..., None])
    want = np.stack([v[:, 32 * (LANE // 32) + s] for s in range(32)], axis=2)
    same_bits(probe, f64, "half_bcast_c<0..31>", out, want)


def case_shfl_xor_c(probe, f64):
    rng = np.random.default_rng(4)
    v = payload(rng, f64, (8, W))
    assert lanes_differ(v)
    out = probe("SHFL_XOR_C", f64, v[..., None])
    same_bits(probe, f64, "wave_shfl_xor_c<1..32>", out, np.stack([v[:, LANE ^ (1 << b)] for b in range(6)], axis=2))


def topo_tables(name):
    """anc / desc / levmask of a compiled topology (dm_types.h make_topo), from the PAR array in the header"""
    src = open(os.path.join(CSRC, "dm_types.h")).read()
    body = re.search(r"struct %s \{.*?PAR\[\d+\] = \{(.*?)\};" % name, src, re.S).group(1)
    par = [int(t) for t in body.replace("\n", " ").split(",")]
    n = len(par)
    anc, depth = [0] * n, [0] * n
    for k in range(n):
        if par[k] >= 0:
            depth[k], anc[k] = depth[par[k]] + 1, anc[par[k]] | (1 << par[k])
    desc = [sum(1 << i for i in range(n) if (anc[i] >> k) & 1) for k in range(n)]
    md = max(depth)
    lev = [sum(1 << k for k in range(n) if depth[k] == md - v) for v in range(md + 1)] + [0] * (n - md - 1)
    return anc, desc, lev


def sel_masks():
    """the lane masks of the LANE_SEL op, chunk by chunk (dm_wave_probe.h wp_mask): the masks the kernels instantiate lane_sel with -- the tree tables of both compiled
    topologies, `lanes below i`, the two-per-wave kernel's keep / below pairs -- then 0, ~0, single bits and arbitrary words"""
    M = (1 << 64) - 1
    pad = lambda a: (list(a) + [0] * 64)[:64]
    dog, hum = topo_tables("TopoDog3d"), topo_tables("TopoHumanoid3d")
    assert len(dog[0]) == 64 and len(hum[0]) == 34
    chunks = [pad(dog[0]), pad(dog[1]), pad(dog[2]), pad(hum[0]), pad(hum[1]), pad(hum[2]), [(1 << c) - 1 for c in range(64)]]
    duo = []
    for c in range(31):
        keep = ~((1 << (c + 1)) - 1) & 0xffffffff
        duo.append((keep << 32) | keep)
    for c in range(31, 61):
        below = (1 << (c - 30)) - 1
        duo.append((below << 32) | below)
    chunks.append(duo + [M, 0xffffffff00000000, 0x00000000ffffffff])
    chunks.append([0, M, 1, 1 << 31, 1 << 32, 1 << 63] + [(c * 0x9E3779B97F4A7C15) & M for c in range(6, 64)])
    assert len(chunks) == wp.MASK_CHUNKS and all(len(c) == 64 for c in chunks)
    return chunks


def case_lane_sel(probe, f64):
    rng = np.random.default_rng(5)
    chunks = sel_masks()
    assert any(m == (1 << 17) - 1 for m in chunks[6]) and sum(1 for m in chunks[0] if m) == 63           # (the tables are the real ones: only the dog's root has no ancestor)
    for ch, masks in enumerate(chunks):
        ab = payload(rng, f64, (3, W, 2))
        out = probe("LANE_SEL", f64, ab, arg=ch)
        pick = np.array([[(m >> l) & 1 for m in masks] for l in range(W)], bool)             # [lane, column]
        same_bits(probe, f64, "lane_sel<mask chunk %d>" % ch, out, np.where(pick[None], ab[:, :, :1], ab[:, :, 1:2]))


def case_row_half_sel(probe, f64):
    """exactly lane R (lanes R and R + 32) takes newv, every other lane keeps oldv, for every R"""
    rng = np.random.default_rng(6)
    on = payload(rng, f64, (4, W, 2))
    out = probe("ROW_SEL_C", f64, on)
    same_bits(probe, f64, "row_sel_c<0..63>", out, np.where((LANE[:, None] == np.arange(64)[None])[None], on[:, :, 1:2], on[:, :, :1]))
    out = probe("HALF_SEL_C", f64, on)
    same_bits(probe, f64, "half_sel_c<0..31>", out, np.where(((LANE % 32)[:, None] == np.arange(32)[None])[None], on[:, :, 1:2], on[:, :, :1]))


def case_chain_keep(probe, f64):
    """bit J of the lane's (lo, hi) ? v : +0.0 -- a kept value keeps its bits, a dropped one is +0.0 whatever it was (-0.0, NaN, inf)"""
    rng = np.random.default_rng(7)
    nw = 6 + 64
    words = rng.integers(0, 2 ** 32, (nw, W, 2)).astype(np.float64)
    words[1], words[2] = 0.0, float(2 ** 32 - 1)
    words[3, :, 0], words[3, :, 1] = 0.0, float(2 ** 32 - 1)
    words[4, :, 0], words[4, :, 1] = float(2 ** 32 - 1), 0.0
    for j in range(64):                 # only bit J, in the word it belongs to; the other word has every bit BUT J & 31 (a test of the wrong word fails either way)
        own, other = float(1 << (j & 31)), float((2 ** 32 - 1) ^ (1 << (j & 31)))
        words[6 + j, :, 0], words[6 + j, :, 1] = (own, other) if j < 32 else (other, own)
    v = payload(rng, f64, (nw, W))
    v[5] = np.tile(np.array([-0.0, np.nan, np.inf, -np.inf]), 16)
    out = probe("CHAIN_KEEP", f64, np.concatenate([v[..., None], words], axis=2))
    lo, hi = words[..., 0].astype(np.uint64), words[..., 1].astype(np.uint64)
    keep = np.stack([(((lo if j < 32 else hi) >> np.uint64(j & 31)) & np.uint64(1)).astype(bool) for j in range(64)], axis=2)
    assert 0.3 < keep[0].mean() < 0.7 and not keep[1].any() and keep[2].all()
    same_bits(probe, f64, "chain_keep<0..63>", out, np.where(keep, v[..., None], 0.0))


def row_file_expected(x, s, g, n):
    e = x[:n].copy()
    for k in range(n):
        if 0 <= s[k] < n:
            e[s[k]] = x[k]
    return np.array([e[g[k]] if 0 <= g[k] < n else FILL for k in range(n)])


def case_row_file(probe, f64):
    """a distinct value per (lane, index); every index read back; a set at r leaves all other indices alone (r = 31 | 32 and N - 1 are the seams of the register vectors)"""
    rng = np.random.default_rng(8)
    for n in (32, 40, 48, 56, 64):
        ident, none = np.arange(n), np.full(n, -1)
        progs = [(none, ident), (ident, ident), (rng.permutation(n), ident), (none, rng.permutation(n)), (rng.permutation(n), rng.permutation(n)), (none, ident[::-1].copy())]
        for r in sorted({0, 1, 15, 16, 30, 31, 32, 33, 39, 40, 47, 48, 55, 56, n - 2, n - 1}):
            if r < n:
                s = none.copy()
                s[(r + 5) % n] = r
                progs.append((s, ident))
        g_only = none.copy()
        g_only[3] = n - 1
        progs.append((none, g_only))            # (entries of g outside 0..N-1 are skipped: their columns keep the fill)
        nw = len(progs)
        inp = np.zeros((nw, W, IN))
        inp[:, :, :n] = payload(rng, f64, (nw, W, n))
        for w, (s, g) in enumerate(progs):
            inp[w, 0, 64:64 + n], inp[w, 1, 64:64 + n] = s, g
        out = probe("ROW_FILE", f64, inp, arg=n)
        want = np.stack([np.stack([row_file_expected(inp[w, l], *progs[w], n) for l in range(W)]) for w in range(nw)])
        skipped = want == FILL
        assert skipped.sum() == W * (n - 1)
        assert (out[..., :n][skipped] == FILL).all()
        want[skipped] = 0.0
        got = out.copy()
        got[..., :n][skipped] = 0.0
        same_bits(probe, f64, "RowFile<Real, %d> set / get" % n, got, want)


def case_xd_operands(probe, f64):
    """float on the device: the column pairs become [Y[k0][0..31] | Y[k1][0..31]], [Y[k0][32..63] | Y[k1][32..63]] (one v_permlane32_swap); a no-op in double and on the emulator"""
    rng = np.random.default_rng(9)
    y = payload(rng, f64, (4, W, 34))
    out = probe("XD_OPERANDS", f64, y)
    want = y.copy()
    if probe.gpu and not f64:
        want[:, :32, 1::2] = y[:, 32:, 0::2]
        want[:, 32:, 0::2] = y[:, :32, 1::2]
    same_bits(probe, f64, "xd_gram_operands<17>", out, want)


def case_ballot(probe, f64):
    rng = np.random.default_rng(10)
    p = np.concatenate([np.eye(W), np.zeros((1, W)), np.ones((1, W)), (LANE < 32)[None] * 1.0, (LANE >= 32)[None] * 1.0, rng.integers(0, 2, (8, W)) * 1.0])
    p[-1] *= -0.0           # (-0.0 != 0 is false)
    p[-2] = np.where(p[-2] != 0, np.nan, 0.0)          # (NaN != 0 is true)
    out = probe("BALLOT", f64, p[..., None])
    mask = [sum(1 << l for l in range(W) if row[l] != 0) for row in p]
    assert mask[-1] == 0 and mask[5] == 1 << 5 and mask[65] == (1 << 64) - 1 and mask[66] == (1 << 32) - 1
    want = np.array([[float(m & 0xffffffff), float(m >> 32)] for m in mask])
    got = out[..., :2]
    assert (got == want[:, None, :]).all(), "wave_ballot: wave %d" % int(np.argwhere((got != want[:, None, :]).any(axis=(1, 2)))[0, 0])
    assert (out[..., 2:] == FILL).all()
    print("WAVEPRIM %-8s f%d %-40s waves %d exact" % (probe.name, 64 if f64 else 32, "wave_ballot", len(p)))


WG_GRIDS = (1, 7, 8, 16, 24, 4096, 4100)


def case_wg_unit(probe, f64):
    """the workgroup -> unit map: a bijection of 0..G-1; on the device (b & 7) * (G / 8) + (b >> 3) when 8 divides G (XCD x takes a contiguous block), else the identity;
    the identity on the emulator"""
    for G in WG_GRIDS:
        out = probe("WG_UNIT", f64, np.zeros((1, W, 1)), n_waves=G)
        b = np.arange(G)
        want = (b & 7) * (G // 8) + (b >> 3) if (probe.gpu and G % 8 == 0) else b
        assert sorted(want.tolist()) == list(range(G))
        assert (out[:, :, 0] == want[:, None]).all() and (out[:, :, 1:] == FILL).all(), "dm_wg_unit: G = %d" % G
    print("WAVEPRIM %-8s f%d %-40s grids %s exact" % (probe.name, 64 if f64 else 32, "dm_wg_unit", WG_GRIDS))


def tr_stage_ref(w, n, mask):
    """xd_tr_stage<N, MASK> on [64, 17] (dm_device_duo.h): pairs (w[2i], w[2i+1]) fold into w[i], a lane keeps one of the pair and adds its partner's other one"""
    w = w.copy()
    bit = ((LANE % 32) & mask) != 0
    for i in range((n + 1) // 2):
        a, b = w[:, 2 * i].copy(), (w[:, 2 * i + 1].copy() if 2 * i + 1 < n else np.zeros(W))
        keep, send = np.where(bit, b, a), np.where(bit, a, b)
        w[:, i] = keep + send[LANE ^ mask]
    return w


def case_xd_tr_stage(probe, f64):
    rng = np.random.default_rng(11)
    for stage, (n, mask) in enumerate(((17, 2), (9, 4), (5, 8), (3, 16))):
        w = rng.integers(-1000, 1001, (4, W, 17)).astype(np.float64)            # integers: the one addition per entry is exact
        out = probe("XD_TR_STAGE", f64, w, arg=stage)
        same_bits(probe, f64, "xd_tr_stage<%d, %d, 17>" % (n, mask), out, np.stack([tr_stage_ref(x, n, mask) for x in w]))


# ---------------------------------------------------------------- reductions
def _sum_case(probe, f64, op, width):
    rng = np.random.default_rng(12)
    nh = W // width
    seg = lambda a: a.reshape(a.shape[0], nh, width)
    big = 2 ** (24 if not f64 else 53)
    ints = [np.eye(W) * (LANE + 1), np.ones((1, W)), (LANE + 1.0)[None], -(LANE + 1.0)[None] * 3, rng.integers(-(big // 128), big // 128, (8, W)).astype(np.float64)]
    if width == 32:         # the halves hold different data: one-hot in one half, a ramp in the other
        ints.append(np.where(LANE < 32, 0.0, LANE + 100.0)[None] + np.eye(W)[:32])
        ints.append(np.where(LANE >= 32, 0.0, LANE + 100.0)[None] + np.eye(W)[32:])
    x = np.concatenate(ints)
    assert np.abs(seg(x)).sum(axis=2).max() < big and (x == np.round(x)).all()            # every partial sum is an integer below 2^24 (2^53): exact in any order
    out = probe(op, f64, x[..., None])
    want = np.repeat(seg(x).sum(axis=2), width, axis=1)
    same_bits(probe, f64, "%s: integers, every lane" % op.lower(), out, want[..., None])
    # mixed sign and magnitude: any association is within gamma_(n-1) * sum |x_i|; every lane of the wave (half) returns the same bits
    x = rnd(rng.standard_normal((64, W)) * 2.0 ** rng.integers(-20, 21, (64, W)), f64)
    out = probe(op, f64, x[..., None])
    got = out[..., 0]
    assert (bits(seg(got), f64) == bits(seg(got)[:, :, :1], f64)).all(), "%s: the lanes disagree" % op
    assert (out[..., 1:] == FILL).all()
    hold(probe, f64, "%s: random, gamma_%d" % (op.lower(), width - 1), np.abs(got - np.repeat(seg(x).sum(axis=2), width, axis=1)),
         gamma(width - 1, f64) * np.repeat(np.abs(seg(x)).sum(axis=2), width, axis=1))


def case_wave_sum(probe, f64):
    _sum_case(probe, f64, "WAVE_SUM", 64)


def case_half_sum(probe, f64):
    _sum_case(probe, f64, "HALF_SUM", 32)


# ---------------------------------------------------------------- Gram matrices
ROW_COUNTS = (1, 17, 31, 32, 33, 64)            # the row counts the callers branch on


def gram_inputs(rng, f64, k):
    """[waves, 64, k]: integer entries |y| <= 8 (every dot product an exact integer < 2^24 in any order, fused or not) -- one wave full, one per row count with only the rows
    below it non-zero -- and, apart, random normal rows with per-row scales spread over 2^+-10"""
    full = rng.integers(-8, 9, (2 + len(ROW_COUNTS), W, k)).astype(np.float64)
    for i, r in enumerate(ROW_COUNTS):
        full[2 + i, r:] = 0.0
    assert k * 64 < 2 ** 24
    smooth = rnd(rng.standard_normal((6, W, k)) * 2.0 ** rng.integers(-10, 11, (6, W, 1)), f64)
    return full, smooth


def gram_check(probe, f64, what, k, run, pick, lanes=W):
    """run(y) -> out; pick(G [waves, 64, 64]) -> the entries each lane is documented to receive [waves, 64, cols]"""
    rng = np.random.default_rng(13 + k)
    ints, smooth = gram_inputs(rng, f64, k)
    G = lambda y: np.einsum("wlk,wik->wli", y, y)
    same_bits(probe, f64, what + ": integer layout", run(ints)[:, :lanes], pick(G(ints))[:, :lanes])
    got, want = run(smooth), pick(G(smooth))
    cols = want.shape[2]
    assert (got[:, :, cols:] == FILL).all()
    hold(probe, f64, what + ": random, gamma_%d" % k, np.abs(got[:, :lanes, :cols] - want[:, :lanes]), gamma(k, f64) * pick(G(np.abs(smooth)))[:, :lanes])


def case_gram32(probe, f64):
    """G[l][i], i < 32, for the lanes 0..31 (see the module docstring for the upper lanes); their y is arbitrary data here and must not leak in"""
    for np2 in (17, 20, 32):
        gram_check(probe, f64, "wave_gram32<%d>" % np2, 2 * np2, lambda y: probe("GRAM32", f64, y, arg=np2), lambda G: G[:, :, :32], lanes=32)


def case_gram64(probe, f64):
    for np2 in (17, 32):
        gram_check(probe, f64, "wave_gram64_half<%d, 0 | 1>" % np2, 2 * np2, lambda y: probe("GRAM64", f64, y, arg=np2), lambda G: G)


def case_duo_gram32(probe, f64):
    """lane l: G[l][32 * (l / 32) + i] -- the rows of its own half, whose data differs from the other's"""
    own = lambda G: np.concatenate([G[:, :32, :32], G[:, 32:, 32:]], axis=1)
    for np2 in (17, 20):
        gram_check(probe, f64, "duo_gram32<%d>" % np2, 2 * np2, lambda y: probe("DUO_GRAM32", f64, y, arg=np2), own)


def case_xd_gram_block(probe, f64):
    """f(r, .) gets G[32 X + r][32 Y + (lane & 31)]: column lane & 31 of block (X, Y).  The off-diagonal blocks are not symmetric (the halves are drawn independently), so a
    transposed unpacking shows"""
    for X in (0, 1):
        for Y in (0, 1):
            blk = lambda G: np.tile(np.swapaxes(G[:, 32 * X:32 * X + 32, 32 * Y:32 * Y + 32], 1, 2), (1, 2, 1))         # [w, lane & 31 = column, r = row]
            gram_check(probe, f64, "xd_gram_block<17, %d, %d>" % (X, Y), 34, lambda y: probe("XD_BLOCK", f64, y, arg=2 * X + Y), blk)


# ---------------------------------------------------------------- dm_rcp, dm_rsqrt
# NEWTON_BOUND -- float on the device: r0 = seed, result = r0 * (2 - x r0)  /  r0 * (1.5 - 0.5 x r0 r0), in units of u = 2^-24, relative to the exact value.
#   Seed: no statement of the accuracy of v_rcp_f32 / v_rsq_f32 was at hand when this was written; ASSUMED 1 ulp, as the public CDNA ISA manuals say for
#   both ("1 ULP accuracy"), i.e. r0 = t (1 + e), |e| <= 2 u, t the exact value.  docs/HISTORY.md section 22 records the measured worst error against this bound
#   (MI355X: rcp 1.59 u, rsqrt 2.00 u of the 3 u).
#   rcp:   exactly, r0 (2 - x r0) = t (1 + e)(1 - e) = t (1 - e^2): the seed error enters squared, e^2 <= 4 u^2.  Roundings: x r0 (|.| ~ 1: abs u, or none if fused into the
#          subtraction), 2 - (.) (~ 1: u), the final product (u): <= 3 u, first order.
#   rsqrt: exactly, r0 (1.5 - 0.5 (1 + e)^2) = t (1 + e)(1 - e - e^2 / 2) = t (1 - 1.5 e^2 - ...): 1.5 e^2 <= 6 u^2.  Roundings: 0.5 x is exact, (0.5 x) r0 and (.) r0 each u
#          relative of a value ~ 0.5, together abs u; 1.5 - (.) ~ 1: u; the final product: u: <= 3 u, first order.
#   Second-order terms (products of the above, e times a rounding: < 20 u^2) are covered by the factor (1 + 2^-20).  Bound: 3 u (1 + 2^-20) = 1.5 ulp-of-1, both ops.
# Double, and both types on the emulator: 1 / x is one correctly rounded division: within 1 ulp of the float64 value; 1 / sqrt(x) two
# roundings: within 2 ulp.  (In double the reference is the same expression.)
NEWTON_BOUND = 3 * U[0] * (1 + 2.0 ** -20)
GUARDS = (1e-12, 1e-18)                 # `a > eps`, `a > 1e-12`, `denom > eps`; `d2n > 1e-18` (pair_eval, the sphere tests of both kernels)


def rcp_inputs(rng, f64, lo):
    """what the call sites can pass: > the guard, pivots / masses / squared lengths up to about 1e6.  Log-uniform, the guards and their neighbours, powers of two and of four
    (where the seed is exact) and the values one ulp either side"""
    x = [np.exp(rng.uniform(np.log(lo), np.log(1e6), 64 * W * 8))]
    p = 2.0 ** np.arange(int(np.ceil(np.log2(lo))), 21)
    edges = np.concatenate([p, np.array(GUARDS)[np.array(GUARDS) >= lo], [1e6, 1.0, 3.0, 1.0 / 3.0]])
    e = rnd(edges, f64).astype(REAL[f64])
    up, dn = np.nextafter(e, REAL[f64](np.inf)), np.nextafter(e, REAL[f64](0))
    x.append(np.concatenate([e, up, dn, np.nextafter(up, REAL[f64](np.inf))]).astype(np.float64))
    x = rnd(np.concatenate(x), f64)
    x = x[x >= rnd(lo, f64) / 2]        # (the guard's lower neighbour stays in: the primitive does not know of the guard)
    pad = (-len(x)) % (64 * W)
    return np.concatenate([x, np.ones(pad)]).reshape(-1, W, 64)


def _newton_case(probe, f64, op, lo, ref, soft_ulps):
    rng = np.random.default_rng(14)
    x = rcp_inputs(rng, f64, lo)
    out = probe(op, f64, x)
    want = ref(x)
    excluded(op.lower(), f64, 0, x.size)
    if probe.gpu and not f64:
        hold(probe, f64, "%s: seed + Newton, 3 u relative" % op.lower(), np.abs(out - want) / want, NEWTON_BOUND)
    else:
        hold(probe, f64, "%s: %d ulp" % (op.lower(), soft_ulps), np.abs(out - want), soft_ulps * ulp(want, f64))


def case_rcp(probe, f64):
    _newton_case(probe, f64, "RCP", GUARDS[0], lambda x: 1.0 / x, 1)


def case_rsqrt(probe, f64):
    _newton_case(probe, f64, "RSQRT", GUARDS[1], lambda x: 1.0 / np.sqrt(x), 2)


# ---------------------------------------------------------------- dm_med3
def med3_rows(f64):
    """(lo, x, hi), lo <= hi: x below, on and above each bound, one representable number either side of each, lo == hi, x = +-inf; zeros of both signs"""
    T = REAL[f64]
    rows = []
    bounds = [(0.0, 1.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (-2.5, 2.5), (-1e-3, 1e-3), (0.0, 1e30), (3.0, 3.0), (-7.0, -7.0), (0.0, 0.125), (-0.0, 1.0), (-1.0, -0.0), (-1.0, 0.0)]
    for lo, hi in bounds:
        lo, hi = T(lo), T(hi)
        xs = [lo, hi, np.nextafter(lo, T(-np.inf)), np.nextafter(lo, T(np.inf)), np.nextafter(hi, T(-np.inf)), np.nextafter(hi, T(np.inf)), T(-np.inf), T(np.inf),
              T(0.0), T(-0.0), (lo + hi) / T(2), lo - T(10), hi + T(10), T(-1e35), T(1e35)]
        rows += [(float(lo), float(x), float(hi)) for x in xs]
    return np.array(rows)


def case_med3(probe, f64):
    """on lo <= hi, x not NaN: min(max(x, lo), hi) bit for bit -- up to the sign of a zero result where zeros of both signs are among (lo, x, hi): `x < lo ? lo : ...` keeps
    x = -0 between lo = +0 and hi, v_med3_f32 and fmax / fmin order -0 < +0 or not as they please; either zero is right there"""
    rows = med3_rows(f64)
    rng = np.random.default_rng(15)
    rand = np.sort(rnd(rng.standard_normal((4096, 3)) * 2.0 ** rng.integers(-8, 9, (4096, 1)), f64), axis=1)[:, [0, 1, 2]]
    rand = np.concatenate([rand, rand[:, [0, 2, 2]], rand[:, [0, 0, 2]], rand[:, [1, 0, 2]], rand[:, [0, 2, 1]]])          # inside, on hi, on lo, below, above
    rows = np.concatenate([rows, rand])
    assert (rows[:, 0] <= rows[:, 2]).all() and not np.isnan(rows).any()
    n = len(rows)
    per = W * 32
    padded = np.concatenate([rows, np.tile([[0.0, 0.5, 1.0]], ((-n) % per, 1))])
    out = probe("MED3", f64, padded.reshape(-1, W, 96))
    assert (out[..., 32:] == FILL).all()
    got = out[..., :32].reshape(-1)[:n]
    want = np.minimum(np.maximum(rows[:, 1], rows[:, 0]), rows[:, 2])
    sgn = np.signbit(rows)
    free = (want == 0) & (got == 0) & ((rows == 0) & sgn).any(axis=1) & ((rows == 0) & ~sgn).any(axis=1)
    excluded("dm_med3 (none: a zero of either sign is accepted, not dropped)", f64, 0, n)
    g, w = bits(np.where(free, 0.0, got), f64), bits(np.where(free, 0.0, want), f64)
    print("WAVEPRIM %-8s f%d %-40s rows %d  either-sign zeros %d  mismatching bits %d" % (probe.name, 64 if f64 else 32, "dm_med3 on lo <= hi", n, int(free.sum()), int((g != w).sum())))
    assert (g == w).all(), "dm_med3%r: %r, want %r" % (tuple(rows[np.argmax(g != w)]), got[np.argmax(g != w)], want[np.argmax(g != w)])


def case_outside_domain(probe, f64):
    """OUTSIDE the pinned domains (module docstring: no call site gets here): what each body returns, tabulated.  The plain statements -- the emulator's, and the double
    ones of the device -- are held to their own text; the hardware paths (v_rcp / v_rsq + Newton step, v_med3_f32) are printed and held only to `one of the operands or
    NaN` / `not a finite non-zero number`: unspecified."""
    T = REAL[f64]
    den = float(np.nextafter(T(0), T(1))) * 3
    xs = np.array([0.0, -0.0, np.inf, np.nan, den])
    inp = np.ones((1, W, 64))
    inp[0, :, :5] = xs
    plain = (not probe.gpu) or f64
    with np.errstate(all="ignore"):
        for op, ref in (("RCP", lambda x: 1.0 / x), ("RSQRT", lambda x: 1.0 / np.sqrt(x))):
            got = probe(op, f64, inp)[0, :, :5]
            assert (bits(got, f64) == bits(got[:1], f64)).all()
            print("WAVEPRIM %-8s f%d %-6s outside: %s" % (probe.name, 64 if f64 else 32, op.lower(), ", ".join("%g -> %g" % (a, b) for a, b in zip(xs, got[0]))))
            want = rnd(ref(rnd(xs, f64)), f64)
            if plain:
                assert (bits(got[0, :4], f64) == bits(want[:4], f64)).all() or (np.isnan(want[3]) and np.isnan(got[0, 3]) and (got[0, :3] == want[:3]).all())
                assert abs(got[0, 4] - want[4]) <= 2 * ulp(want[4], f64) or np.isinf(want[4])
            else:
                assert all(np.isnan(v) or np.isinf(v) or v == 0 for v in got[0, :4])
    tri = np.array([(1.0, 0.0, -1.0), (1.0, 5.0, -1.0), (1.0, -5.0, -1.0), (2.0, 0.5, 0.25), (0.0, np.nan, 1.0), (-1.0, np.nan, 1.0), (1.0, np.nan, -1.0)])
    inp = np.tile(np.array([0.0, 0.5, 1.0]), (1, W, 32))
    inp[0, :, :tri.size] = tri.ravel()
    got = probe("MED3", f64, inp)[0, 0, :len(tri)]
    print("WAVEPRIM %-8s f%d med3   outside: %s" % (probe.name, 64 if f64 else 32, ", ".join("(%g, %g, %g) -> %g" % (*t, g) for t, g in zip(tri, got))))
    lo, x, hi = tri.T
    with np.errstate(all="ignore"):
        if not probe.gpu:
            want = np.where(x < lo, lo, np.where(x > hi, hi, x))                   # x < lo ? lo : (x > hi ? hi : x): NaN x passes through
        elif f64:
            want = np.fmax(lo, np.fmin(hi, x))                                     # fmax(lo, fmin(hi, x)): lo when lo > hi, the larger bound when x is NaN
        else:
            want = None
    if want is not None:
        assert (bits(got, f64) == bits(want, f64)).all() or all((np.isnan(a) and np.isnan(b)) or a == b for a, b in zip(got, want))
    else:
        assert (got[:4] == np.median(tri[:4], axis=1)).all()                       # v_med3_f32 IS the median of three numbers
        assert all(np.isnan(g) or g in (t[0], t[2]) for t, g in zip(tri[4:], got[4:]))


CASES = dict(wave_shfl=case_wave_shfl, bcast=case_bcast, half_bcast_c=case_half_bcast_c, shfl_xor_c=case_shfl_xor_c, lane_sel=case_lane_sel, row_half_sel=case_row_half_sel,
             chain_keep=case_chain_keep, row_file=case_row_file, xd_operands=case_xd_operands, ballot=case_ballot, wg_unit=case_wg_unit, xd_tr_stage=case_xd_tr_stage,
             wave_sum=case_wave_sum, half_sum=case_half_sum, gram32=case_gram32, gram64=case_gram64, duo_gram32=case_duo_gram32, xd_gram_block=case_xd_gram_block,
             rcp=case_rcp, rsqrt=case_rsqrt, med3=case_med3, outside_domain=case_outside_domain)


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_primitive_emulator(emu_lib, case, f64):
    CASES[case](Probe(emu_lib, gpu=False), f64)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_primitive_gpu(hip_lib, case, f64):
    CASES[case](Probe(hip_lib, gpu=True), f64)


# ---------------------------------------------------------------- the entry point
def _argument_checks(lib_path):
    lib = load_library(lib_path)
    inp = np.zeros((2, W, IN))
    out = np.full((2, W, OUT), 7.0)
    good = dict(op="WAVE_SUM", f64=0, n_waves=2, in_ptr=inp.ctypes.data, out_ptr=out.ctypes.data, lib_path=lib_path)
    bads = [dict(n_waves=0), dict(n_waves=-3), dict(n_waves=65537), dict(in_ptr=0), dict(out_ptr=0), dict(op=-1), dict(op=len(wp.OPS)), dict(arg=1), dict(op="ROW_FILE", arg=0),
            dict(op="ROW_FILE", arg=33), dict(op="GRAM32", arg=0), dict(op="GRAM64", arg=20), dict(op="DUO_GRAM32", arg=32), dict(op="XD_BLOCK", arg=4), dict(op="XD_TR_STAGE", arg=-1),
            dict(op="LANE_SEL", arg=wp.MASK_CHUNKS)]
    for bad in bads:
        with pytest.raises(RuntimeError, match="dm_wave_probe"):
            wp.wave_probe(**dict(good, **bad))
        assert b"dm_wave_probe" in lib.dm_last_error()
    assert (out == 7.0).all()           # nothing was launched


def test_argument_checks_emulator(emu_lib):
    _argument_checks(emu_lib)


@pytest.mark.gpu
def test_argument_checks_gpu(hip_lib):
    """host addresses: every call is refused before a launch, so none is dereferenced"""
    _argument_checks(hip_lib)


def test_binding_names_the_ops_of_the_header():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    enum = re.search(r"enum \{ (DM_WOP_WAVE_SHFL = 0,[^}]*)\}", src).group(1)
    names = [s.strip().split(" ")[0] for s in enum.split(",")]
    assert names == ["DM_WOP_" + o for o in wp.OPS] + ["DM_WOP_COUNT"]
    for macro, value in (("IN", wp.IN), ("OUT", wp.OUT), ("MASK_CHUNKS", wp.MASK_CHUNKS)):
        assert int(re.search(r"#define DM_WAVE_PROBE_%s (\d+)" % macro, src).group(1)) == value
    probe = open(os.path.join(CSRC, "dm_wave_probe.h")).read()
    for o in wp.OPS:                    # every op of the header has a branch in the kernel, and a case here reaches it
        assert "case DM_WOP_%s:" % o in probe, o
    assert len(CASES) == 22


def test_probe_is_compiled_into_the_misc_object_only():
    """the step-family objects never see the probe: dm_kernels.cpp includes it under DM_MISC_FAMILY alone, dm_host.cpp only declares its launcher"""
    k = open(os.path.join(CSRC, "dm_kernels.cpp")).read()
    assert re.search(r'#if DM_TU_ID == DM_MISC_FAMILY\n#include "dm_wave_probe.h"[^\n]*\n#endif', k)
    assert '#include "dm_wave_probe.h"' not in open(os.path.join(CSRC, "dm_host.cpp")).read()
    for f in ("dm_device.h", "dm_device_duo.h"):
        assert "wave_probe" not in open(os.path.join(CSRC, f)).read()
