"""New weights into a live policy context (include/dm_hip.h dm_policy_set_weights, dm_policy_read_packed; k_policy_pack of deepmimic_amd/csrc/dm_policy.h).

dm_policy_create(_gated) and dm_policy_set_weights pack through the same kernel, so "refresh equals create" says nothing about the layout.  Two things here do:

* np_packed: the layout stated once more, in numpy -- fragment order, the fused stream's block order (plain and gated), bias slots as fp32 bits, 1 / s_std, zero
  padding, round-to-nearest-even to bf16 with NaN -> 0x7fc0.  Every expected byte of the refresh tests comes from it.
* tests/golden/policy_packed_sha256.json: SHA-256 of every packed array of every shape, recorded from the last commit whose dm_policy_create packed on the host
  (tests/golden/make_policy_packed_sha256.py).  A fresh context AND np_packed must reproduce them from golden_weights (integer arithmetic only).

For every shape of SHAPES -- the smallest set that reaches every packing branch -- two contexts P_A, P_B are created from the asymmetric random weights A and B
(all biases, normalisers and logstd non-zero and different), P_A takes B through set_weights*, and then

* read_packed of EVERY array (padding included) of P_A and of P_B is byte-equal to np_packed(B) -- and P_A's differed before the call;
* forward (mode, and sampled with one seed; 33 rows, so a 32-row tile is crossed) gives bit-identical actions and log-probabilities -- and differed before.

Modes: "device" (device pointers, [in, out]; every source starts 4 bytes behind a 16-byte boundary, as a torch view may), "out_in" (the same B handed over as
transposed copies with DM_WEIGHTS_OUT_IN) and "host" (numpy arrays, staged by the library).  Each runs on the CPU emulator build (device pointers are host
pointers there) and under `-m gpu`.  The emulated MFMA is slow: on the emulator the width-1024 forward runs once, on the first shape; the other 1024-wide shapes
compare bytes there and the small widths run the forward.
"""
import ctypes as C
import functools
import hashlib
import json
import os
from dataclasses import dataclass

import numpy as np
import pytest

from deepmimic_amd.policy import GATE_KEYS, PACKED_IDS, PLAIN_KEYS, Policy, _GateParams, _PolicyParams, random_weights, reference_forward

ROWS = 33
S_CLIP = 5.0


@dataclass(frozen=True)
class Shape:
    S: int
    A: int
    H1: int = 1024
    H2: int = 512
    G: int = 0
    GC: int = 0
    GH: int = 0
    K1: int = 0
    N3: int = 0
    fused: bool = True
    emu_forward: bool = False


SHAPES = {
    "hum": Shape(197, 28, K1=256, N3=32, emu_forward=True),                                   # fused, K1 = 256, N3 = 32
    "k384": Shape(270, 36, K1=384, N3=64),                                                    # fused, K1 320 promoted to 384, N3 = 64
    "critic": Shape(100, 1, K1=256, N3=32),                                                   # fused, K1 128 promoted to 256; the critic / discriminator shape
    "small": Shape(70, 5, 128, 64, K1=128, N3=32, fused=False, emu_forward=True),             # the per-layer paths: no fused stream
    "gated_fused": Shape(200, 36, G=3, GC=128, GH=64, K1=256, N3=64),                         # 197 + 3: the gated fused stream
    "gated_layered": Shape(200, 28, G=3, GC=64, GH=32, K1=256, N3=32, fused=False),           # gate widths 64 / 32: gated per-layer kernels at 1024 / 512
    "gated_small": Shape(73, 5, 128, 64, G=3, GC=64, GH=32, K1=128, N3=32, fused=False, emu_forward=True),   # the same at widths the emulator forwards quickly
}
MODES = ("device", "out_in", "host")
MATRICES = ("w1", "w2", "w3", "gc_w", "g0_w", "g0_bias_w", "g0_scale_w", "g1_w", "g1_bias_w", "g1_scale_w")


@functools.lru_cache(maxsize=None)
def weights(name, seed):
    """random_weights plus what it leaves zero or constant: every bias, both normalisers, logstd.  Shared between the tests: never written to."""
    sh = SHAPES[name]
    w = random_weights(sh.S, sh.A, sh.H1, sh.H2, seed=seed, init_output_scale=0.3, gated_goal_dim=sh.G, gate_common=sh.GC or 128, gate_hidden=sh.GH or 64)
    rng = np.random.default_rng(1000 + seed)
    for k, v in list(w.items()):
        if k != "goal_dim" and v.ndim == 1:
            w[k] = (rng.normal(size=v.shape) * 0.1 + 0.05).astype(np.float32)
    w["logstd"] = rng.uniform(-3.0, -2.0, sh.A).astype(np.float32)
    w["s_mean"] = rng.normal(size=sh.S).astype(np.float32); w["s_std"] = rng.uniform(0.5, 2.0, sh.S).astype(np.float32)
    w["a_mean"] = rng.normal(size=sh.A).astype(np.float32); w["a_std"] = rng.uniform(0.5, 2.0, sh.A).astype(np.float32)
    for v in w.values():
        if isinstance(v, np.ndarray):
            assert np.all(v != 0)
            v.setflags(write=False)
    return w


def arrays(w):
    return {k: v for k, v in w.items() if k != "goal_dim"}


def states(name):
    return (np.random.default_rng(7).normal(size=(ROWS, SHAPES[name].S)) * 1.5 + 0.3).astype(np.float32)


class Side:
    """where the library's device pointers point: host memory on the emulator build, torch tensors on the GPU"""

    def __init__(self, on_gpu):
        self.on_gpu = on_gpu
        self.keep = []

    def put(self, a):
        """device address of a copy of `a` that starts 4 bytes behind a 16-byte boundary"""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        if self.on_gpu:
            import torch
            buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
            buf[1:].copy_(torch.from_numpy(a))
            torch.cuda.synchronize()
            self.keep.append(buf)
            ptr = buf[1:].data_ptr()
        else:
            buf = np.empty(a.size + 8, np.float32)
            off = (1 - buf.ctypes.data // 4) % 4
            buf[off:off + a.size] = a
            self.keep.append(buf)
            ptr = buf.ctypes.data + 4 * off
        assert ptr % 16 == 4
        return ptr

    def forward(self, pol, s, **kw):
        if not self.on_gpu:
            return pol.forward_host(s, **kw)
        import torch
        ts = torch.from_numpy(s).cuda(); ta = torch.zeros((s.shape[0], pol.A), device="cuda"); tl = torch.zeros(s.shape[0], device="cuda")
        torch.cuda.synchronize()
        pol.forward_device(ts.data_ptr(), s.shape[0], ta.data_ptr(), tl.data_ptr(), **kw)
        torch.cuda.synchronize()
        return ta.cpu().numpy(), tl.cpu().numpy()

    def set(self, pol, w, mode="device"):
        if mode == "host":
            pol.set_weights(w)
        elif mode == "out_in":
            pol.set_weights_device({k: self.put(v.T if v.ndim == 2 else v) for k, v in arrays(w).items()}, out_in=True)
        else:
            pol.set_weights_device({k: self.put(v) for k, v in arrays(w).items()})


def names(pol):
    """every packed array the context holds"""
    info = pol.info()
    return [k for k in PACKED_IDS if (k != "wfs" or info["fused"]) and (not k.startswith("gate_") or info["gated"])]


def packed(pol):
    return {k: pol.read_packed(k) for k in names(pol)}


def assert_same_bytes(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %s differs in %d of %d bytes" % (what, k, int((got[k] != want[k]).sum()), want[k].size)


def frag_index(k, n, Kp):
    """position of W[k, n] in a packed array [n-tile][k-step][lane][8] (bf16 elements)"""
    return (((n // 16) * (Kp // 32) + k // 32) * 64 + (n % 16) + 16 * ((k % 32) // 8)) * 8 + k % 8


# ---------------------------------------------------------------------------------------------------------------------------------- the layout, in numpy
def bf16_bits(x):
    """fp32 -> bf16 codes: round to nearest, ties to even; every NaN -> 0x7fc0"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC0
    return out


def frags(W, Kp, Np):
    """W [K x N] as MFMA B-operand fragments [n-tile][k-step][512]: bf16, zero-padded to Kp x Np; inside a fragment lane l = 16 g + c holds the eight
    consecutive k = 32 ks + 8 g + i of column n = 16 nt + c (frag_index says the same per element)"""
    K, N = W.shape
    P = np.zeros((Kp, Np), np.uint16)
    P[:K, :N] = bf16_bits(W)
    return P.reshape(Kp // 32, 4, 8, Np // 16, 16).transpose(3, 0, 1, 4, 2).reshape(Np // 16, Kp // 32, 512)      # [ks, g, i, nt, c] -> [nt, ks, g, c, i]


def bias_slot(b, ft):
    """a 1 KB slot of fp32 bits: lane l holds the four biases of features 16 ft + 4 (l >> 4) + r"""
    return np.repeat(np.ascontiguousarray(b[16 * ft:16 * ft + 16], dtype=np.float32).reshape(4, 1, 4), 16, axis=1).reshape(-1).view(np.uint16)


def fused_stream(w, K1, gated):
    """the weight stream of the one-launch actor (H1 = 1024, H2 = 512, gate_hidden = 64): 1 KB slots (one fragment each), eight to a block.  Per wave w = 0 .. 3 and
    per layer-1 chunk q = 0 .. 3: K1 / 64 blocks {k-steps 2 b, 2 b + 1 x feature tiles 16 q + 4 w + j} of layer 1; gated: 3 blocks = the gate tiles of those four
    feature tiles; 8 blocks {k-step 8 q + ksl x feature tiles 8 w + n} of layer 2.  Gated: behind the last chunk 6 blocks = the gate tiles of layer 2's feature
    tiles 8 w + n.  A gate tile is six slots: sigma fragments of k-steps 0, 1, beta fragments of k-steps 0, 1, the sigma biases, the beta biases."""
    F1, F2 = frags(w["w1"], K1, 1024), frags(w["w2"], 1024, 512)
    if gated:
        Fs = [frags(w["g%d_scale_w" % i], 64, H) for i, H in ((0, 1024), (1, 512))]
        Fb = [frags(w["g%d_bias_w" % i], 64, H) for i, H in ((0, 1024), (1, 512))]
    out = []

    def gate_tile(i, ft):
        out.extend([Fs[i][ft, 0], Fs[i][ft, 1], Fb[i][ft, 0], Fb[i][ft, 1], bias_slot(w["g%d_scale_b" % i], ft), bias_slot(w["g%d_bias_b" % i], ft)])
    for wv in range(4):
        for q in range(4):
            for b in range(K1 // 64):
                out.extend(F1[16 * q + 4 * wv + j, 2 * b + kk] for kk in range(2) for j in range(4))
            if gated:
                for j in range(4):
                    gate_tile(0, 16 * q + 4 * wv + j)
            for ksl in range(8):
                out.extend(F2[8 * wv + n, 8 * q + ksl] for n in range(8))
        if gated:
            for n in range(8):
                gate_tile(1, 8 * wv + n)
    return np.concatenate(out)


def np_packed(w, sh):
    """every packed array of a context made from the weights dict `w` of Shape `sh`, as read_packed hands them back (uint8), by the names of PACKED_IDS"""
    f32 = lambda a, n=None: np.concatenate([np.asarray(a, np.float32), np.zeros((n or len(a)) - len(a), np.float32)])
    opt = lambda k, n, fill: w[k] if w.get(k) is not None else np.full(n, fill, np.float32)
    out = dict(w1p=frags(w["w1"], sh.K1, sh.H1), w2p=frags(w["w2"], sh.H1, sh.H2), w3p=frags(w["w3"], sh.H2, sh.N3),
               b1=f32(w["b1"]), b2=f32(w["b2"]), b3=f32(w["b3"], sh.N3), s_mean=f32(opt("s_mean", sh.S, 0)), s_inv_std=np.float32(1) / f32(opt("s_std", sh.S, 1)),
               a_mean=f32(opt("a_mean", sh.A, 0)), a_std=f32(opt("a_std", sh.A, 1)), logstd=f32(opt("logstd", sh.A, 0)))
    if sh.fused:
        out["wfs"] = fused_stream(w, sh.K1, sh.G > 0)
    if sh.G:
        out.update(gate_wcp=frags(w["gc_w"], (sh.G + 31) // 32 * 32, sh.GC), gate_bc=f32(w["gc_b"]))
        for i, H in ((0, sh.H1), (1, sh.H2)):
            out.update({"gate_wep%d" % i: frags(w["g%d_w" % i], sh.GC, sh.GH), "gate_be%d" % i: f32(w["g%d_b" % i]),
                        "gate_wbp%d" % i: frags(w["g%d_bias_w" % i], sh.GH, H), "gate_bb%d" % i: f32(w["g%d_bias_b" % i]),
                        "gate_wsp%d" % i: frags(w["g%d_scale_w" % i], sh.GH, H), "gate_bs%d" % i: f32(w["g%d_scale_b" % i])})
    assert all(v.dtype in (np.float32, np.uint16) for v in out.values())
    return {k: np.ascontiguousarray(out[k]).reshape(-1).view(np.uint8) for k in PACKED_IDS if k in out}


@functools.lru_cache(maxsize=None)
def packed_ref(name, seed):
    """np_packed of weights(name, seed), once per shape.  Shared between the tests: never written to."""
    p = np_packed(weights(name, seed), SHAPES[name])
    for v in p.values():
        v.setflags(write=False)
    return p


# ---------------------------------------------------------------------------------------------------------------------------------- golden bytes
OPTIONAL = ("s_mean", "s_std", "a_mean", "a_std", "logstd")
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_packed_sha256.json")
GOLDEN_CASES = [n + v for n in SHAPES for v in ("", "/defaults")]      # "/defaults": created without the arrays of OPTIONAL


def hash_floats(n, salt):
    """n float32 in (-1, 1), none zero: odd multiples of 2^-24 from a 32-bit multiplicative hash of the index.  Integer arithmetic only and every value exact
    in fp32, so the bits depend on no numpy version and no random generator"""
    h = ((np.arange(1, n + 1, dtype=np.uint64) + np.uint64(0x9E3779B9 * (salt + 1) & 0xFFFFFFFF)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return (((h >> np.uint64(8)).astype(np.int64) * 2 + 1 - 2 ** 24).astype(np.float64) / 2.0 ** 24).astype(np.float32)


def golden_weights(case):
    """the weights of a golden case: hash_floats per array (distinct salts), the standard deviations 1 + |.|, SPECIAL planted in every matrix at evenly spaced
    flat positions"""
    name, _, variant = case.partition("/")
    sh = SHAPES[name]
    shapes = dict(w1=(sh.S, sh.H1), b1=(sh.H1,), w2=(sh.H1, sh.H2), b2=(sh.H2,), w3=(sh.H2, sh.A), b3=(sh.A,), s_mean=(sh.S,), s_std=(sh.S,), a_mean=(sh.A,),
                  a_std=(sh.A,), logstd=(sh.A,))
    if sh.G:
        shapes.update(gc_w=(sh.G, sh.GC), gc_b=(sh.GC,))
        for i, H in ((0, sh.H1), (1, sh.H2)):
            shapes.update({"g%d_w" % i: (sh.GC, sh.GH), "g%d_b" % i: (sh.GH,), "g%d_bias_w" % i: (sh.GH, H), "g%d_bias_b" % i: (H,),
                           "g%d_scale_w" % i: (sh.GH, H), "g%d_scale_b" % i: (H,)})
    w = {}
    for salt, k in enumerate(PLAIN_KEYS + GATE_KEYS):
        if k not in shapes or (variant == "defaults" and k in OPTIONAL):
            continue
        v = hash_floats(int(np.prod(shapes[k])), salt)
        if k in ("s_std", "a_std"):
            v = (1.0 + np.abs(v.astype(np.float64))).astype(np.float32)
        if k in MATRICES:
            every = v.size // len(SPECIAL)
            v.view(np.uint32)[every // 2 + every * np.arange(len(SPECIAL))] = np.array(SPECIAL, np.uint32)
        else:
            assert np.all(v != 0)
        w[k] = v.reshape(shapes[k])
    if sh.G:
        w["goal_dim"] = sh.G
    return w


def digest(p):
    """what the golden file holds of a dict of packed arrays: size and SHA-256 per array"""
    return {k: dict(bytes=int(v.size), sha256=hashlib.sha256(v.tobytes()).hexdigest()) for k, v in p.items()}


def check_golden(lib, case):
    """a fresh context and np_packed both give the bytes dm_policy_create gave when it still packed on the host"""
    with open(GOLDEN_FILE) as fh:
        want = json.load(fh)["cases"][case]
    sh = SHAPES[case.partition("/")[0]]
    w = golden_weights(case)
    assert len(want) == 11 + (1 if sh.fused else 0) + (14 if sh.G else 0)
    pol = Policy(w, lib_path=lib, s_clip=S_CLIP)
    got = digest(packed(pol))
    pol.close()
    mine = digest(np_packed(w, sh))
    for k in want:
        assert got[k] == want[k], "%s: %s of a fresh context is not what the golden file holds" % (case, k)
        assert mine[k] == want[k], "%s: %s of np_packed is not what the golden file holds" % (case, k)
    assert got.keys() == want.keys() == mine.keys()


def check_refresh(lib, on_gpu, name, mode):
    sh = SHAPES[name]
    wa, wb = weights(name, 1), weights(name, 2)
    side = Side(on_gpu)
    pa, pb = Policy(wa, lib_path=lib, s_clip=S_CLIP), Policy(wb, lib_path=lib, s_clip=S_CLIP)
    info = pa.info()
    assert (info["K1"], info["N3"], info["fused"], info["gated"]) == (sh.K1, sh.N3, sh.fused, sh.G > 0)
    want = packed_ref(name, 2)
    assert_same_bytes(packed(pb), want, "%s, created" % name)
    assert len(want) == 11 + (1 if sh.fused else 0) + (14 if sh.G else 0)
    if not sh.fused:
        with pytest.raises(RuntimeError, match="no fused weight stream"):
            pa.read_packed("wfs")
    if not sh.G:
        with pytest.raises(RuntimeError, match="without a gate"):
            pa.read_packed("gate_wcp")
    before = packed(pa)
    for k in want:
        assert not np.array_equal(before[k], want[k]), "%s is the same in A and B: the comparison would be vacuous" % k
    forward = mode == "device" and (on_gpu or sh.emu_forward)
    if forward:
        s = states(name)
        kw = dict(sample=True, seed=0x5EED, step=3, env_id_offset=11)
        ref_mode, ref_samp = side.forward(pb, s), side.forward(pb, s, **kw)
        a0, lp0 = side.forward(pa, s)
        assert not np.array_equal(a0, ref_mode[0]) and not np.array_equal(lp0, ref_mode[1])
    side.set(pa, wb, mode)
    assert_same_bytes(packed(pa), want, "%s / %s" % (name, mode))
    assert pa.info()["K1"] == sh.K1 and pa.info()["N3"] == sh.N3
    if forward:
        for got, ref in ((side.forward(pa, s), ref_mode), (side.forward(pa, s, **kw), ref_samp)):
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.isfinite(ref_samp[0]).all() and not np.array_equal(ref_samp[0], ref_mode[0])
    pa.close(); pb.close()


def check_partial(lib, on_gpu, name):
    """only logstd and b3 given: those two arrays become B's, every other array keeps A's bytes"""
    wa, wb = weights(name, 1), weights(name, 2)
    side = Side(on_gpu)
    pa = Policy(wa, lib_path=lib)
    a_bytes, b_bytes = packed(pa), packed_ref(name, 2)
    side.set(pa, dict(logstd=wb["logstd"], b3=wb["b3"]))
    got = packed(pa)
    assert_same_bytes(got, {k: (b_bytes[k] if k in ("logstd", "b3") else a_bytes[k]) for k in a_bytes}, name)
    assert not np.array_equal(a_bytes["b3"], b_bytes["b3"]) and not np.array_equal(a_bytes["logstd"], b_bytes["logstd"])
    # only the three layers: the fused stream follows them, everything else stays
    side.set(pa, {k: wb[k] for k in ("w1", "w2", "w3")})
    got2 = packed(pa)
    moved = ("w1p", "w2p", "w3p") + (("wfs",) if "wfs" in got2 and not SHAPES[name].G else ())
    for k in got2:
        if k in moved:
            assert np.array_equal(got2[k], b_bytes[k]), k
        elif k != "wfs":
            assert np.array_equal(got2[k], got[k]), k
    # ... and every array, a gated stream's mix of A's gate tiles and B's layers included, is what the layout makes of that mix
    assert_same_bytes(got2, np_packed({**wa, **{k: wb[k] for k in ("logstd", "b3", "w1", "w2", "w3")}}, SHAPES[name]), name + ", mixed")
    pa.close()


SPECIAL = (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF,      # NaNs: quiet, signed with a payload, signalling, all ones -> 0x7fc0, every one
           0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: to even, 0x3f80 / 0x3f82 and their negatives
           0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F800000, 0x00000001, 0x80000000)      # just above / below a tie, the largest finite (-> inf), inf, a denormal, -0
SPECIAL_BF16 = (0x7FC0, 0x7FC0, 0x7FC0, 0x7FC0, 0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F80, 0x7F80, 0x0000, 0x8000)


def check_nan_and_ties(lib, on_gpu, name, mode):
    """NaNs and exact round-to-even ties in every matrix: the bytes must be np_packed's, after a refresh and in a context created from the same arrays, and w1p
    holds the stated codes"""
    sh = SHAPES[name]
    wb = dict(weights(name, 2))
    rng = np.random.default_rng(5)
    where = {}
    for k in MATRICES:
        if k in wb:
            m = wb[k].copy()
            flat = rng.choice(m.size, size=len(SPECIAL), replace=False)
            m.reshape(-1).view(np.uint32)[flat] = np.array(SPECIAL, np.uint32)
            wb[k] = m; where[k] = flat
    side = Side(on_gpu)
    pa, pb = Policy(weights(name, 1), lib_path=lib), Policy(wb, lib_path=lib)
    want = np_packed(wb, sh)
    assert_same_bytes(packed(pb), want, name + ", created")
    w1p = want["w1p"].view(np.uint16)
    for pos, code in zip(where["w1"], SPECIAL_BF16):
        assert w1p[frag_index(pos // sh.H1, pos % sh.H1, sh.K1)] == code
    side.set(pa, wb, mode)
    assert_same_bytes(packed(pa), want, name)
    pa.close(); pb.close()


def check_refusals(lib, on_gpu):
    """width mismatch, a gate for a plain context, no gate for a gated one: non-zero with a message that names the trouble, packed bytes untouched"""
    side = Side(on_gpu)
    for name in ("small", "gated_small"):
        sh = SHAPES[name]
        wa, wb = weights(name, 1), weights(name, 2)
        pol = Policy(wa, lib_path=lib)
        before = packed(pol)
        ptr = {k: side.put(v) for k, v in arrays(wb).items()}
        fp = lambda k: C.cast(C.c_void_p(ptr[k]), C.POINTER(C.c_float)) if k in ptr else None
        lib_ = pol.lib
        lib_.dm_policy_set_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

        def call(dims, gate):
            pp = _PolicyParams(*dims, *[fp(k) for k in PLAIN_KEYS], 0.0)
            gp = None if gate is None else C.byref(_GateParams(*gate, *[fp(k) for k in GATE_KEYS]))
            rc = lib_.dm_policy_set_weights(pol.h, C.byref(pp), gp, 1, None)
            return rc, lib_.dm_last_error().decode()
        good = (sh.S, sh.H1, sh.H2, sh.A)
        gate = (sh.G, sh.GC, sh.GH) if sh.G else None
        cases = [((sh.S + 1, sh.H1, sh.H2, sh.A), gate, "state_dim"), ((sh.S, sh.H1 + 64, sh.H2, sh.A), gate, "hidden1"),
                 ((sh.S, sh.H1, sh.H2 + 64, sh.A), gate, "hidden2"), ((sh.S, sh.H1, sh.H2, sh.A + 1), gate, "action_dim")]
        if sh.G:
            cases += [(good, None, "gated context"), (good, (sh.G + 1, sh.GC, sh.GH), "goal_dim"), (good, (sh.G, sh.GC + 32, sh.GH), "gate_common"),
                      (good, (sh.G, sh.GC, sh.GH + 32), "gate_hidden")]
        else:
            cases += [(good, (3, 64, 32), "without a gate")]
        for dims, g, word in cases:
            rc, msg = call(dims, g)
            assert rc != 0 and "dm_policy_set_weights" in msg and word in msg, (dims, g, rc, msg)
            assert_same_bytes(packed(pol), before, "%s after a refused call (%s)" % (name, word))
        rc, msg = call(good, gate)                       # the same pointers with the right widths go through
        assert rc == 0, msg
        assert not np.array_equal(pol.read_packed("w1p"), before["w1p"])
        # the Python layer: a gate key for a plain context reaches the library's refusal; a wrong shape is caught in front of it
        if not sh.G:
            with pytest.raises(RuntimeError, match="without a gate"):
                pol.set_weights(dict(gc_b=np.ones(64, np.float32)))
        with pytest.raises(ValueError, match="w1 is"):
            pol.set_weights(dict(w1=np.ones((sh.S, sh.H1 + 1), np.float32)))
        pol.close()


# ---------------------------------------------------------------------------------------------------------------------------------- CPU emulator
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_create_packs_golden_bytes_emulator(emu_lib, case):
    check_golden(emu_lib, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_set_weights_equals_create_emulator(emu_lib, name, mode):
    check_refresh(emu_lib, False, name, mode)


@pytest.mark.parametrize("name", ["hum", "small", "gated_fused"])
def test_set_weights_partial_update_emulator(emu_lib, name):
    check_partial(emu_lib, False, name)


@pytest.mark.parametrize("name,mode", [("hum", "device"), ("small", "out_in"), ("gated_fused", "out_in"), ("gated_small", "host")])
def test_set_weights_nan_and_ties_emulator(emu_lib, name, mode):
    check_nan_and_ties(emu_lib, False, name, mode)


def test_set_weights_refusals_emulator(emu_lib):
    check_refusals(emu_lib, False)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU twins
@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_create_packs_golden_bytes_gpu(hip_lib, case):
    check_golden(hip_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_set_weights_equals_create_gpu(hip_lib, name, mode):
    check_refresh(hip_lib, True, name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hum", "small", "gated_fused"])
def test_set_weights_partial_update_gpu(hip_lib, name):
    check_partial(hip_lib, True, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("hum", "device"), ("small", "out_in"), ("gated_fused", "out_in"), ("gated_small", "host")])
def test_set_weights_nan_and_ties_gpu(hip_lib, name, mode):
    check_nan_and_ties(hip_lib, True, name, mode)


@pytest.mark.gpu
def test_set_weights_refusals_gpu(hip_lib):
    check_refusals(hip_lib, True)


@pytest.mark.gpu
def test_set_weights_torch_between_two_forwards_on_one_stream(hip_lib):
    """three torch.nn.Linear layers 70 -> 128 -> 64 -> 5, one SGD step, then set_weights_torch(layout="out_in") on a non-default stream between two forwards on
    that stream with no synchronisation in between: the second forward must act with the stepped parameters -- bit for bit the actions of a fresh Policy built
    from them on the host, and within 2e-3 of reference_forward(bf16=True) (the tolerance of tests/test_policy.py for this comparison)"""
    import torch
    S, H1, H2, A, n = 70, 128, 64, 5, ROWS
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(S, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU(), torch.nn.Linear(H2, A)).cuda()
    lin = [net[0], net[2], net[4]]
    logstd = torch.nn.Parameter(torch.full((A,), -2.0, device="cuda"))
    with torch.no_grad():
        for m in lin:
            m.bias.normal_(0.0, 0.1)

    def host_weights():
        w = {}
        for i, m in enumerate(lin, 1):
            w["w%d" % i] = m.weight.detach().cpu().numpy().T.copy(); w["b%d" % i] = m.bias.detach().cpu().numpy().copy()
        w["logstd"] = logstd.detach().cpu().numpy().copy()
        return w
    w_old = host_weights()
    pol = Policy(w_old, lib_path=hip_lib, s_clip=S_CLIP)
    s = (np.random.default_rng(9).normal(size=(n, S)) * 1.5).astype(np.float32)
    ts = torch.from_numpy(s).cuda()
    a1 = torch.zeros((n, A), device="cuda"); a2 = torch.zeros((n, A), device="cuda")
    opt = torch.optim.SGD(list(net.parameters()) + [logstd], lr=0.5)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        h = stream.cuda_stream
        loss = 0.01 * net(ts).sum() + logstd.sum()
        opt.zero_grad(); loss.backward(); opt.step()
        pol.forward_device(ts.data_ptr(), n, a1.data_ptr(), stream=h)
        pol.set_weights_torch(dict(w1=lin[0].weight, b1=lin[0].bias, w2=lin[1].weight, b2=lin[1].bias, w3=lin[2].weight, b3=lin[2].bias, logstd=logstd), layout="out_in")
        pol.forward_device(ts.data_ptr(), n, a2.data_ptr(), stream=h)
    torch.cuda.synchronize()
    w_new = host_weights()
    assert all(not np.array_equal(w_new[k], w_old[k]) for k in w_new)                       # the step moved every parameter
    fresh = Policy(w_new, lib_path=hip_lib, s_clip=S_CLIP)
    want, _ = Side(True).forward(fresh, s)
    old_ref, _ = reference_forward(w_old, s, s_clip=S_CLIP, bf16=True)
    new_ref, _ = reference_forward(w_new, s, s_clip=S_CLIP, bf16=True)
    assert np.abs(a1.cpu().numpy() - old_ref).max() < 2e-3                                  # the first forward still ran the old weights
    assert np.array_equal(a2.cpu().numpy(), want)
    assert np.abs(a2.cpu().numpy() - new_ref).max() < 2e-3
    assert np.abs(new_ref - old_ref).max() > 2e-2                                           # ... and the two differ by far more than the tolerance
    assert_same_bytes(packed(pol), np_packed(w_new, SHAPES["small"]), "after set_weights_torch")      # (the widths of "small"; no normalisers: the defaults)
    # the argument checks of set_weights_torch
    with pytest.raises(ValueError, match="w1 must be a contiguous float32"):
        pol.set_weights_torch(dict(w1=lin[0].weight.t()), layout="out_in")                  # right shape for in_out, but a transposed view
    with pytest.raises(ValueError, match="w1 must be a contiguous float32"):
        pol.set_weights_torch(dict(w1=lin[0].weight.double()), layout="out_in")
    with pytest.raises(ValueError, match="b1 must be a contiguous float32"):
        pol.set_weights_torch(dict(b1=lin[0].bias.detach().cpu()), layout="out_in")
    pol.close(); fresh.close()
