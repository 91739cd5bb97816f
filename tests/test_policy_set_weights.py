"""New weights into a live policy context (include/dm_hip.h dm_policy_set_weights, dm_policy_read_packed; k_policy_pack of deepmimic_amd/csrc/dm_policy.h).

The device pack must make of an fp32 array exactly what the host packers of dm_policy_create make of it.  For every shape of SHAPES -- the smallest set that
reaches every packing branch -- two contexts P_A, P_B are created from the asymmetric random weights A and B (all biases, normalisers and logstd non-zero and
different), P_A takes B through set_weights*, and then

* read_packed of EVERY array (padding included) is byte-equal between P_A and P_B -- and differed before the call;
* forward (mode, and sampled with one seed; 33 rows, so a 32-row tile is crossed) gives bit-identical actions and log-probabilities -- and differed before.

Modes: "device" (device pointers, [in, out]; every source starts 4 bytes behind a 16-byte boundary, as a torch view may), "out_in" (the same B handed over as
transposed copies with DM_WEIGHTS_OUT_IN) and "host" (numpy arrays, staged by the library).  Each runs on the CPU emulator build (device pointers are host
pointers there) and under `-m gpu`.  The emulated MFMA is slow: on the emulator the width-1024 forward runs once, on the first shape; the other 1024-wide shapes
compare bytes there and the small widths run the forward.
"""
import ctypes as C
import functools
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


def check_refresh(lib, on_gpu, name, mode):
    sh = SHAPES[name]
    wa, wb = weights(name, 1), weights(name, 2)
    side = Side(on_gpu)
    pa, pb = Policy(wa, lib_path=lib, s_clip=S_CLIP), Policy(wb, lib_path=lib, s_clip=S_CLIP)
    info = pa.info()
    assert (info["K1"], info["N3"], info["fused"], info["gated"]) == (sh.K1, sh.N3, sh.fused, sh.G > 0)
    want = packed(pb)
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
    pa, pb = Policy(wa, lib_path=lib), Policy(wb, lib_path=lib)
    a_bytes, b_bytes = packed(pa), packed(pb)
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
    pa.close(); pb.close()


SPECIAL = (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF,      # NaNs: quiet, signed with a payload, signalling, all ones -> 0x7fc0, every one
           0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: to even, 0x3f80 / 0x3f82 and their negatives
           0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F800000, 0x00000001, 0x80000000)      # just above / below a tie, the largest finite (-> inf), inf, a denormal, -0
SPECIAL_BF16 = (0x7FC0, 0x7FC0, 0x7FC0, 0x7FC0, 0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F80, 0x7F80, 0x0000, 0x8000)


def check_nan_and_ties(lib, on_gpu, name, mode):
    """NaNs and exact round-to-even ties in every matrix: the bytes must be the host packer's (P_B, created from the same arrays), and w1p holds the stated codes"""
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
    want = packed(pb)
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
    assert_same_bytes(packed(pol), packed(fresh), "after set_weights_torch")
    # the argument checks of set_weights_torch
    with pytest.raises(ValueError, match="w1 must be a contiguous float32"):
        pol.set_weights_torch(dict(w1=lin[0].weight.t()), layout="out_in")                  # right shape for in_out, but a transposed view
    with pytest.raises(ValueError, match="w1 must be a contiguous float32"):
        pol.set_weights_torch(dict(w1=lin[0].weight.double()), layout="out_in")
    with pytest.raises(ValueError, match="b1 must be a contiguous float32"):
        pol.set_weights_torch(dict(b1=lin[0].bias.detach().cpu()), layout="out_in")
    pol.close(); fresh.close()
