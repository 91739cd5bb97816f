"""PPO actor / critic minibatch gradients and the momentum step on the device (deepmimic_amd/csrc/dm_train.h, include/dm_hip.h dm_train_*, deepmimic_amd/train.py)
against the numpy statements beside the binding.  Every check runs on the emulator library through host addresses and again, marked `gpu`, through torch tensors.

Shapes: the nets (S, H1, H2, A) = (37, 64, 64, 3) and (70 of which 3 from a goal block, 128, 192, 33) -- K1 padding, N3 = 64, a non-power-of-two tile count, the
one-wave and the tiled layer kernels -- with rows n in {1, 15, 16, 17, 33, 65, 130}, and the reference's (197, 1024, 512, 36) once at n = 33.

How a device result is held to the mirror.  The matrix cores accumulate in fp32 in an order of their own, so a bf16 activation can land on the other side of a rounding
boundary than a float64 mirror of the WHOLE pass: the random-input check therefore walks the stages, each from the DEVICE's own inputs to that stage (the activations
through dm_train_read_activations, z3 and dz from the workspace):
  * a contraction of length k in fp32 differs from the float64 one by at most gamma_k sum|a||b|, gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability,
    eq. 3.5; the bound tests/test_wave_primitives.py uses for the Gram matrices); with the bias add k + 1;
  * a stage that ends in a bf16 rounding must land in [bf16(x - bound), bf16(x + bound)] (rounding is monotone);
  * the head is element-wise fp32 with every rounding point written down (the library's own exp), so from the device's z3 the mirror gives the SAME BITS: dz3 and logp
    are compared exactly, the fp64 statistics to 1e-13 relative (the mirror adds in another order; <= 130 terms of fp64 rounding are 1e-14).
On inputs where every product and sum is exact (small integers) the whole call is compared bit for bit."""
import numpy as np
import pytest

from deepmimic_amd import train as tr
from deepmimic_amd.policy import Policy, random_weights

ROWS = [1, 15, 16, 17, 33, 65, 130]
NET_A = dict(S=37, G=0, H1=64, H2=64, A=3)
NET_B = dict(S=70, G=3, H1=128, H2=192, A=33)
NET_REF = dict(S=197, G=0, H1=1024, H2=512, A=36)
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


class Emu:
    """host memory and the emulator library: a 'device array' is a numpy view whose first byte is 16-byte aligned"""
    gpu = False

    def __init__(self, lib):
        self.lib, self.stream = lib, 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        buf = np.zeros(a.size + 16, a.dtype)
        start = ((-buf.ctypes.data) % 16) // a.itemsize
        view = buf[start:start + a.size].reshape(a.shape)
        view[...] = a
        return view

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return h.copy()

    def device(self):
        return "cpu"


class Gpu:
    """torch tensors on the GPU and the HIP library, on torch's current stream"""
    gpu = True

    def __init__(self, lib):
        import torch
        self.lib, self.torch, self.stream = lib, torch, int(torch.cuda.current_stream().cuda_stream)

    def put(self, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda")
        assert t.data_ptr() % 16 == 0
        return t

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        return h.cpu().numpy()

    def device(self):
        return "cuda"


def net_weights(net, seed=1, A=None, normalisers=True):
    A = net["A"] if A is None else A
    w = random_weights(net["S"], A, H1=net["H1"], H2=net["H2"], seed=seed, init_output_scale=0.3)
    if normalisers:
        rng = np.random.default_rng(seed + 100)
        w["s_mean"] = rng.uniform(-0.5, 0.5, net["S"]).astype(np.float32); w["s_std"] = rng.uniform(0.5, 2.0, net["S"]).astype(np.float32)
        w["a_mean"] = rng.uniform(-0.2, 0.2, A).astype(np.float32); w["a_std"] = rng.uniform(0.5, 2.0, A).astype(np.float32)
        w["logstd"] = rng.uniform(-2.0, -0.5, A).astype(np.float32)
        w["b1"] = rng.uniform(-0.1, 0.1, net["H1"]).astype(np.float32); w["b2"] = rng.uniform(-0.1, 0.1, net["H2"]).astype(np.float32)
        w["b3"] = rng.uniform(-0.1, 0.1, A).astype(np.float32)
    return w


def run_grad(be, pol, net, flat, head, states, **kw):
    """one *_grad call on sentinel-filled outputs: dict(grads, stats, out, z3, dz3, dz2, dz1, s16, h1, h2 -- the activations as bf16 VALUES); `states` holds the goal columns"""
    n, G, A = states.shape[0], net["G"], pol.A
    P = tr.param_count(pol)
    nb = tr.workspace_bytes(pol, n)
    lay = tr.workspace_layout(net["H1"], net["H2"], A, n)
    assert nb == lay["bytes"] and nb % 8 == 0
    d = dict(params=be.put(flat), states=be.put(states[:, :net["S"] - G]), goals=be.put(states[:, net["S"] - G:]) if G else None,
             grads=be.put(np.full(P, np.nan, np.float32)), stats=be.put(np.full(6 if head == "actor" else 2, np.nan)), out=be.put(np.full(n, np.nan, np.float32)),
             ws=be.put(np.zeros(nb // 8)))
    common = dict(goals_ptr=be.ptr(d["goals"]) if G else 0, goal_dim=G, stream=be.stream)
    if head == "actor":
        for k in ("actions", "old_logp", "adv"):
            d[k] = be.put(np.asarray(kw[k], np.float32))
        tr.actor_grad_device(pol, be.ptr(d["params"]), be.ptr(d["states"]), n, be.ptr(d["actions"]), be.ptr(d["old_logp"]), be.ptr(d["adv"]), be.ptr(d["grads"]),
                             be.ptr(d["stats"]), be.ptr(d["ws"]), nb, kw.get("ratio_clip", 0.2), kw.get("bound_weight", 10.0), kw.get("a_bound_min"), kw.get("a_bound_max"),
                             logp_ptr=be.ptr(d["out"]), **common)
    else:
        d["targets"] = be.put(np.asarray(kw["targets"], np.float32))
        tr.value_grad_device(pol, be.ptr(d["params"]), be.ptr(d["states"]), n, be.ptr(d["targets"]), be.ptr(d["grads"]), be.ptr(d["stats"]), be.ptr(d["ws"]), nb,
                             values_ptr=be.ptr(d["out"]), **common)
    out = {k: be.get(d[k]) for k in ("grads", "stats", "out")}
    raw = np.ascontiguousarray(be.get(d["ws"])).view(np.uint8)
    for k in ("z3", "dz3", "dz2", "dz1"):
        off, dt, shape = lay[k]
        out[k] = raw[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape).copy()
    for k in ("s16", "h1", "h2"):
        out[k] = tr.bf16_value(tr.read_activations(pol, k, n))
    out["ws_bytes"] = raw.tobytes()
    return out


def blocks(net, A, flat):
    return tr.unpack_params(flat, net["S"], net["H1"], net["H2"], A)


# ---------------------------------------------------------------- 1. indexing, bit for bit

def integer_case(net, n, head, seed=0):
    """inputs on which every product and sum is exact: states with three small non-zeros per row, sparse weights in {-2 .. 2} / {-1, 0, 1}, so that h1, h2 and every dz are
    integers below 256 (exact in bf16) and every sum stays far below 2^24; sigma = 1, a_std = 2, ratio = 1 and adv, the target errors and bound_weight multiples of n, so
    that the head's divisions are exact too"""
    rng = np.random.default_rng([seed, net["S"], n])
    S, H1, H2 = net["S"], net["H1"], net["H2"]
    A = net["A"] if head == "actor" else 1
    f = np.float32
    def sparse(rows, cols, per_col, vals):
        m = np.zeros((rows, cols), f)
        for c in range(cols):
            m[rng.choice(rows, size=min(per_col, rows), replace=False), c] = rng.choice(vals, size=min(per_col, rows))
        return m
    w = dict(w1=rng.integers(-2, 3, (S, H1)).astype(f), b1=rng.integers(-1, 2, H1).astype(f), w2=sparse(H1, H2, 4, [-1, 1]), b2=rng.integers(-1, 2, H2).astype(f),
             w3=sparse(H2, A, 4, [-1, 1]), b3=rng.integers(-2, 3, A).astype(f), s_mean=np.ones(S, f), s_std=np.full(S, 2, f), a_mean=np.ones(A, f), a_std=np.full(A, 2, f),
             logstd=np.zeros(A, f))
    states = np.ones((n, S), f)                                     # (s - 1) / 2 = 0 except where set
    for i in range(n):
        states[i, rng.choice(S, size=3, replace=False)] = 1 + 2 * rng.choice([-1, 1, 2], size=3)
    states[:, S - 1] = 3                                            # the last column (of the goal block where there is one) is always live
    return w, states, A, rng


def check_indexing(be, net, n, head):
    w, states, A, rng = integer_case(net, n, head)
    flat = tr.pack_params(w)
    pol = Policy(w, lib_path=be.lib)
    fwd = tr.reference_forward_bf16(w, states)
    z3 = fwd[3]
    assert np.abs(fwd[1]).max() < 256 and np.abs(fwd[2]).max() < 256 and (z3 == np.round(z3)).all()
    m = rng.integers(-2, 3, n).astype(np.float32)
    if head == "actor":
        actions = (1 + 2 * (z3 + rng.integers(-2, 3, z3.shape))).astype(np.float32)       # u = x - mu in {-2 .. 2}
        old = tr.reference_actor_head(z3, actions, np.zeros(n), np.zeros(n), w["a_mean"], w["a_std"], w["logstd"])["logp"]
        lo = np.full(A, -np.inf, np.float32); hi = np.full(A, np.inf, np.float32)
        lo[0] = 1 + 2 * np.median(z3[:, 0]); hi[A - 1] = 1 + 2 * np.median(z3[:, A - 1])
        kw = dict(actions=actions, old_logp=old, adv=m * n, bound_weight=float(n), a_bound_min=lo, a_bound_max=hi)
    else:
        kw = dict(targets=z3[:, 0] - m * n)
    got = run_grad(be, pol, net, flat, head, states, **kw)
    ref = tr.reference_grad(w, states, head, **kw)
    for k in ("s16", "h1", "h2"):
        assert np.array_equal(got[k][:, :ref[k].shape[1]], ref[k]) and not got[k][:, ref[k].shape[1]:].any(), k
    assert np.array_equal(got["z3"][:, :A], ref["z3"]) and not got["z3"][:, A:].any()
    for k in ("dz3", "dz2", "dz1"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["grads"], ref["grads"])
    assert np.array_equal(got["out"], ref["logp"] if head == "actor" else ref["values"])
    exact = [0, 1, 2, 3, 4] if head == "actor" else [0, 1]
    assert np.array_equal(got["stats"][exact], ref["stats"][exact]), (got["stats"], ref["stats"])
    if head == "actor":
        assert abs(got["stats"][5] - ref["stats"][5]) <= 1e-13 * abs(ref["stats"][5])
        assert got["stats"][3] == 0 and got["stats"][4] == 1.0 and (ref["stats"][2] > 0 or n == 1)


@pytest.mark.parametrize("head", ["actor", "critic"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("net", [NET_A, NET_B], ids=["A", "B"])
def test_indexing_bit_for_bit(emu_lib, net, n, head):
    check_indexing(Emu(emu_lib), net, n, head)


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["actor", "critic"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("net", [NET_A, NET_B], ids=["A", "B"])
def test_indexing_bit_for_bit_gpu(hip_lib, net, n, head):
    check_indexing(Gpu(hip_lib), net, n, head)


# ---------------------------------------------------------------- 2. random inputs, stage by stage

def random_case(net, n, head, seed=0):
    A = net["A"] if head == "actor" else 1
    w = net_weights(net, seed=seed + 1, A=A)
    rng = np.random.default_rng([seed, net["S"], n, 7])
    states = (rng.standard_normal((n, net["S"])) * 1.5 + 0.2).astype(np.float32)
    if head == "actor":
        z3 = tr.reference_forward_bf16(w, states)[3]
        sg = np.exp(w["logstd"])
        actions = ((z3 + sg * rng.standard_normal(z3.shape)) * w["a_std"] + w["a_mean"]).astype(np.float32)
        lp = tr.reference_actor_head(z3, actions, np.zeros(n), np.zeros(n), w["a_mean"], w["a_std"], w["logstd"])["logp"]
        old = (lp + rng.uniform(-0.4, 0.4, n)).astype(np.float32)                  # ratios on both sides of 1 +- 0.2
        kw = dict(actions=actions, old_logp=old, adv=rng.standard_normal(n).astype(np.float32), ratio_clip=0.2, bound_weight=10.0,
                  a_bound_min=(w["a_mean"] - 0.3 * w["a_std"]).astype(np.float32), a_bound_max=(w["a_mean"] + 0.3 * w["a_std"]).astype(np.float32))
    else:
        kw = dict(targets=rng.standard_normal(n).astype(np.float32))
    return w, states, A, kw


def in_bf16_interval(bits, x, bound, what):
    lo, hi = tr.bf16_value(tr.bf16_bits((x - bound).astype(np.float32))), tr.bf16_value(tr.bf16_bits((x + bound).astype(np.float32)))
    v = tr.bf16_value(bits) if bits.dtype == np.uint16 else bits
    # (x -+ bound are rounded to float32 first: one more half ulp of fp32 on each side, far inside a bf16 step; widen by it)
    slack = 2 * U * np.abs(x)
    lo2, hi2 = tr.bf16_value(tr.bf16_bits((x - bound - slack).astype(np.float32))), tr.bf16_value(tr.bf16_bits((x + bound + slack).astype(np.float32)))
    bad = ~((v >= np.minimum(lo, lo2)) & (v <= np.maximum(hi, hi2)))
    assert not bad.any(), (what, int(bad.sum()), v[bad][:4], x[bad][:4], bound[bad][:4])


def check_stages(got, w, states, A, head, kw, s_clip=np.inf):
    f64 = np.float64
    n = states.shape[0]
    S, H1 = w["w1"].shape; H2 = w["w2"].shape[1]
    # forward: s16 is element-wise (exact); h1, h2 from the device's own inputs
    s16_ref = tr.reference_forward_bf16(w, states, s_clip)[0]
    assert np.array_equal(got["s16"][:, :S], s16_ref) and not got["s16"][:, S:].any()
    ins = dict(w1=got["s16"][:, :S], w2=got["h1"], w3=got["h2"])
    for wk, bk, hk in (("w1", "b1", "h1"), ("w2", "b2", "h2")):
        a, b = ins[wk].astype(f64), tr.bf16_round(w[wk]).astype(f64)
        pre = a @ b + w[bk]; bound = gamma(a.shape[1] + 1) * (np.abs(a) @ np.abs(b) + np.abs(w[bk]))
        in_bf16_interval(got[hk], np.maximum(pre, 0), bound, hk)           # relu is monotone and 1-Lipschitz
    a, b = got["h2"].astype(f64), tr.bf16_round(w["w3"]).astype(f64)
    z3 = a @ b + w["b3"]
    assert (np.abs(got["z3"][:, :A] - z3) <= gamma(H2 + 1) * (np.abs(a) @ np.abs(b) + np.abs(w["b3"]))).all() and not got["z3"][:, A:].any()
    # the head from the device's z3: the same bits
    if head == "actor":
        hd = tr.reference_actor_head(got["z3"], a_mean=w["a_mean"], a_std=w["a_std"], logstd=w["logstd"], **kw)
        assert np.array_equal(got["out"], hd["logp"])
    else:
        hd = tr.reference_value_head(got["z3"], **kw)
        assert np.array_equal(got["out"], hd["values"])
    assert np.array_equal(got["dz3"], hd["dz3"])
    assert np.allclose(got["stats"], hd["stats"], rtol=1e-13, atol=1e-300), (got["stats"], hd["stats"])
    # backward, each stage from the device's operands
    lay = tr.layout(S, H1, H2, A)
    grad = lambda k: got["grads"][lay[k][0]:lay[k][0] + int(np.prod(lay[k][1]))].reshape(lay[k][1])
    dz = dict(w3=tr.bf16_value(got["dz3"])[:, :A].astype(f64), w2=tr.bf16_value(got["dz2"]).astype(f64), w1=tr.bf16_value(got["dz1"]).astype(f64))
    assert not got["dz3"][:, A:].any()
    for wk, bk in (("w3", "b3"), ("w2", "b2"), ("w1", "b1")):
        a = ins[wk].astype(f64)
        assert (np.abs(grad(wk) - a.T @ dz[wk]) <= gamma(n) * (np.abs(a).T @ np.abs(dz[wk])) + 1e-300).all(), wk
        assert (np.abs(grad(bk) - dz[wk].sum(axis=0)) <= gamma(n) * np.abs(dz[wk]).sum(axis=0) + 1e-300).all(), bk
    for wk, hk, dk in (("w3", "h2", "dz2"), ("w2", "h1", "dz1")):
        b = tr.bf16_round(w[wk]).astype(f64)
        x = np.where(got[hk] != 0, dz[wk] @ b.T, 0.0); bound = np.where(got[hk] != 0, gamma(b.shape[1]) * (np.abs(dz[wk]) @ np.abs(b).T), 0.0)
        in_bf16_interval(got[dk], x, bound, dk)
    assert np.isfinite(got["grads"]).all()


def check_random(be, net, n, head):
    w, states, A, kw = random_case(net, n, head)
    pol = Policy(w, lib_path=be.lib)
    got = run_grad(be, pol, net, tr.pack_params(w), head, states, **kw)
    check_stages(got, w, states, A, head, kw)
    if head == "actor":            # the inputs reach both sides of the clip and of the bounds
        assert 0 < got["stats"][3] < 1 or n < 15
        assert got["stats"][2] > 0


RANDOM_CASES = [(NET_A, 17, "actor"), (NET_A, 130, "critic"), (NET_B, 1, "actor"), (NET_B, 33, "critic"), (NET_B, 130, "actor"), (NET_REF, 33, "actor")]
RANDOM_IDS = ["A-17-actor", "A-130-critic", "B-1-actor", "B-33-critic", "B-130-actor", "ref-33-actor"]


@pytest.mark.parametrize("net,n,head", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage(emu_lib, net, n, head):
    check_random(Emu(emu_lib), net, n, head)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n,head", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage_gpu(hip_lib, net, n, head):
    check_random(Gpu(hip_lib), net, n, head)


# ---------------------------------------------------------------- 3. consistency with the sampling net

def check_sampling_consistency(be, net, n, monkeypatch):
    """Rows sampled by dm_policy_forward_ex on the per-layer kernels, fed back: the training forward is the same kernels on the same weights, so mu is the same bits and
    logp_new - logp_old is rounding alone.  Bound per row, u = 2^-24, z the drawn noise (recovered as u_j of the mirror):
      the action's round trip  na = mu + sigma z (2 roundings), a = na std + mean (2), a - mean (1), / std (1):  |dx_j| <= u (4 |x_j| + |sigma_j z_j| + (|a_j| + |a_j - mean_j|) / std_j)
      x - mu (1), / sigma (1), and sigma itself (exp_det within 2 ulp, the sampler's expf within 2):            |u_j - z_j| <= dx_j / sigma_j + 6 u |z_j| =: d_j
      the two row sums of A + 3 terms (u_j^2 / 2 or z_j^2 / 2 + logstd_j, A ln 2pi / 2) on both sides:           2 gamma_(A + 3) (sum z_j^2 / 2 + sum |logstd_j| + A ln 2pi / 2)
    |logp_new - logp_old| <= sum_j (|z_j| d_j + d_j^2 / 2) (1 + 2 u) + the row-sum term.
    Measured on the MI355X: 8.3e-7 against a smallest bound of 7.0e-6 (A = 3, n = 17), 4.8e-6 against 3.9e-4 (A = 33, n = 65); emulator 8.3e-7 / 5.7e-6."""
    monkeypatch.setenv("DM_POLICY_LAYERED", "1")
    w = net_weights(net, seed=5)
    A, S, G = net["A"], net["S"], net["G"]
    pol = Policy(w, lib_path=be.lib)
    rng = np.random.default_rng([n, S])
    states = (rng.standard_normal((n, S)) * 1.5).astype(np.float32)
    d_s, d_g = be.put(states[:, :S - G]), (be.put(states[:, S - G:]) if G else None)
    d_a, d_lp = be.put(np.zeros((n, A), np.float32)), be.put(np.zeros(n, np.float32))
    pol.forward_device_ex(be.ptr(d_s), n, be.ptr(d_a), be.ptr(d_g) if G else 0, G, be.ptr(d_lp), sample=True, seed=11, step=3, stream=be.stream)
    actions, old = be.get(d_a), be.get(d_lp)
    adv = rng.standard_normal(n).astype(np.float32); adv[0] = 0.0
    kw = dict(actions=actions, old_logp=old, adv=adv, ratio_clip=0.2, bound_weight=10.0)
    got = run_grad(be, pol, net, tr.pack_params(w), "actor", states, **kw)
    hd = tr.reference_actor_head(got["z3"], a_mean=w["a_mean"], a_std=w["a_std"], logstd=w["logstd"], **kw)
    assert np.array_equal(got["dz3"], hd["dz3"]) and np.array_equal(got["out"], hd["logp"])
    f64 = np.float64
    sg, std, mean = np.exp(w["logstd"].astype(f64)), w["a_std"].astype(f64), w["a_mean"].astype(f64)
    x = (actions.astype(f64) - mean) / std
    z = (x - got["z3"][:, :A].astype(f64)) / sg
    dx = U * (4 * np.abs(x) + np.abs(sg * z) + (np.abs(actions) + np.abs(actions - mean)) / std)
    dj = dx / sg + 6 * U * np.abs(z)
    bound = (np.abs(z) * dj + 0.5 * dj ** 2).sum(axis=1) * (1 + 2 * U) + 2 * gamma(A + 3) * (0.5 * (z ** 2).sum(axis=1) + np.abs(w["logstd"]).sum() + 0.5 * A * np.log(2 * np.pi))
    diff = np.abs(got["out"].astype(f64) - old.astype(f64))
    print("sampling consistency: max |logp_new - logp_old| = %.3g, smallest bound %.3g (A = %d, n = %d)" % (diff.max(), bound.min(), A, n))
    assert (diff <= bound).all(), (diff.max(), bound.min())
    assert got["stats"][3] == 0.0                                  # clip_frac
    assert (hd["g"][adv != 0] != 0).all() and hd["g"][0] == 0


@pytest.mark.parametrize("net,n", [(NET_A, 17), (NET_B, 65)], ids=["A-17", "B-65"])
def test_sampling_consistency(emu_lib, net, n, monkeypatch):
    check_sampling_consistency(Emu(emu_lib), net, n, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", [(NET_A, 17), (NET_B, 65)], ids=["A-17", "B-65"])
def test_sampling_consistency_gpu(hip_lib, net, n, monkeypatch):
    check_sampling_consistency(Gpu(hip_lib), net, n, monkeypatch)


# ---------------------------------------------------------------- 4. head branches

def check_head_branches(be):
    """8 hand-built rows on net A: ratio just inside and just outside 1 - eps and 1 + eps for adv > 0 and adv < 0; column 0 with a finite lower bound at the median of mu
    (rows below and inside), column 1 unbounded (-inf, +inf), column 2 with a finite upper bound at the median (rows inside and above) and an infinite lower one.
    From the device's z3 the mirror's g, dz3 and logp are the same bits.  The statistics are fp64 sums of at most 8 float32 values (and of their exact squares): sums
    of float32 values of like size are exact in fp64 in any order, so those are compared exactly; the sum of squares (48-bit terms) to 4 ulp.  grads: the stage bounds."""
    net, n, eps = NET_A, 8, 0.2
    w = net_weights(net, seed=9)
    A = net["A"]
    pol = Policy(w, lib_path=be.lib)
    rng = np.random.default_rng(4)
    states = rng.standard_normal((n, net["S"])).astype(np.float32)
    flat = tr.pack_params(w)
    z3 = run_grad(be, pol, net, flat, "actor", states, actions=np.zeros((n, A)), old_logp=np.zeros(n), adv=np.zeros(n))["z3"]       # the device's mu
    actions = ((z3[:, :A] + np.exp(w["logstd"]) * rng.standard_normal((n, A))) * w["a_std"] + w["a_mean"]).astype(np.float32)
    lp = tr.reference_actor_head(z3, actions, np.zeros(n), np.zeros(n), w["a_mean"], w["a_std"], w["logstd"])["logp"]
    d = np.log(np.array([1 - eps, 1 - eps, 1 + eps, 1 + eps] * 2)) + np.array([3e-5, -3e-5, -3e-5, 3e-5] * 2)      # inside, outside, inside, outside
    old = (lp.astype(np.float64) - d).astype(np.float32)
    adv = np.array([1.5, 0.7, 2.0, 0.3, -1.5, -0.7, -2.0, -0.3], np.float32)
    lo = np.array([w["a_mean"][0] + w["a_std"][0] * np.median(z3[:, 0]), -np.inf, -np.inf], np.float32)
    hi = np.array([np.inf, np.inf, w["a_mean"][2] + w["a_std"][2] * np.median(z3[:, 2])], np.float32)
    kw = dict(actions=actions, old_logp=old, adv=adv, ratio_clip=eps, bound_weight=10.0, a_bound_min=lo, a_bound_max=hi)
    got = run_grad(be, pol, net, flat, "actor", states, **kw)
    hd = tr.reference_actor_head(got["z3"], a_mean=w["a_mean"], a_std=w["a_std"], logstd=w["logstd"], **kw)
    # the rows are what they were built to be
    r = hd["ratio"].astype(np.float64)
    inside = np.array([True, False, True, False] * 2)
    assert ((np.abs(r - 1) <= np.float32(eps)) == inside).all() and (np.abs(np.abs(r - 1) - eps) < 1e-4).all()
    # tf.minimum(l0, l1): the gradient flows unless the clipped branch is the smaller one: adv > 0 and ratio > 1 + eps, adv < 0 and ratio < 1 - eps
    flows = np.array([True, True, True, False, True, False, True, True])
    assert ((hd["g"] != 0) == flows).all()
    mu = got["z3"][:, :A]
    lo_n, hi_n = (lo[0] - w["a_mean"][0]) / w["a_std"][0], (hi[2] - w["a_mean"][2]) / w["a_std"][2]
    assert 0 < (mu[:, 0] < lo_n).sum() < n and 0 < (mu[:, 2] > hi_n).sum() < n
    assert np.array_equal(got["dz3"], hd["dz3"]) and np.array_equal(got["out"], hd["logp"])
    assert np.array_equal(got["stats"][[0, 1, 3, 4, 5]], hd["stats"][[0, 1, 3, 4, 5]]), (got["stats"], hd["stats"])
    assert got["stats"][3] == 0.5 and abs(got["stats"][2] - hd["stats"][2]) <= 4 * np.spacing(hd["stats"][2]) and hd["stats"][2] > 0
    check_stages(got, w, states, A, "actor", kw)
    # no bound arrays: no bound term, bound loss 0
    kw2 = dict(kw, a_bound_min=None, a_bound_max=None)
    got2 = run_grad(be, pol, net, flat, "actor", states, **kw2)
    hd2 = tr.reference_actor_head(got2["z3"], a_mean=w["a_mean"], a_std=w["a_std"], logstd=w["logstd"], **kw2)
    assert np.array_equal(got2["dz3"], hd2["dz3"]) and got2["stats"][2] == 0.0 and not np.array_equal(got2["dz3"], got["dz3"])


def test_head_branches(emu_lib):
    check_head_branches(Emu(emu_lib))


@pytest.mark.gpu
def test_head_branches_gpu(hip_lib):
    check_head_branches(Gpu(hip_lib))


# ---------------------------------------------------------------- 5. against the unrounded net

def torch_reference_grads(w, states, head, kw):
    """float64 autograd of the same loss on the fp32 masters, nothing rounded"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    p = {k: t(w[k]).requires_grad_(True) for k in tr.KEYS}
    x = (t(states) - t(w["s_mean"])) * t(np.float32(1) / w["s_std"])
    h = torch.relu(x @ p["w1"] + p["b1"]); h = torch.relu(h @ p["w2"] + p["b2"]); z3 = h @ p["w3"] + p["b3"]
    if head == "critic":
        loss = 0.5 * ((t(kw["targets"]) - z3[:, 0]) ** 2).mean()
    else:
        A = z3.shape[1]
        sg, mean, std = torch.exp(t(w["logstd"])), t(w["a_mean"]), t(w["a_std"])
        u = ((t(kw["actions"]) - mean) / std - z3) / sg
        logp = -0.5 * (u ** 2).sum(1) - 0.5 * A * np.log(2 * np.pi) - t(w["logstd"]).sum()
        ratio = torch.exp(logp - t(kw["old_logp"])); adv = t(kw["adv"])
        loss = -torch.minimum(adv * ratio, adv * torch.clamp(ratio, 1 - kw["ratio_clip"], 1 + kw["ratio_clip"])).mean()
        lo, hi = (t(kw["a_bound_min"]) - mean) / std, (t(kw["a_bound_max"]) - mean) / std
        viol = (torch.clamp(z3 - lo, max=0) ** 2).sum(1) + (torch.clamp(z3 - hi, min=0) ** 2).sum(1)
        loss = loss + kw["bound_weight"] * 0.5 * viol.mean()
    loss.backward()
    return {k: p[k].grad.numpy() for k in tr.KEYS}


# relative error ||g - g64|| / ||g64|| of each gradient block against float64 autograd on the unrounded net; bounds one notch (the next of 1, 2, 5 x 10^k) above the
# measurement, taken on the emulator, which runs the same arithmetic (DESIGN.md section 3 convention).  Measured:
#   B-130-actor    w1 6.1e-2  b1 1.9e-2  w2 2.9e-2  b2 1.9e-2  w3 2.1e-2  b3 1.6e-2
#   A-65-critic    w1 3.2e-2  b1 2.6e-2  w2 2.3e-2  b2 2.2e-2  w3 5.6e-3  b3 6.9e-3
# Nine tenths of it is the bf16 rounding of the WEIGHTS alone (a float64 net with bf16 weights and nothing else rounded is 5.9e-2 / 2.9e-2 away in w1): a rounding of
# 2^-9 moves pre-activations across zero and ratios across 1 +- eps, and a row that changes sides changes its whole contribution.
UNROUNDED = {"B-130-actor": (NET_B, 130, "actor", dict(w1=1e-1, b1=2e-2, w2=5e-2, b2=2e-2, w3=5e-2, b3=2e-2)),
             "A-65-critic": (NET_A, 65, "critic", dict(w1=5e-2, b1=5e-2, w2=5e-2, b2=5e-2, w3=1e-2, b3=1e-2))}


def check_unrounded(be, name):
    net, n, head, bounds = UNROUNDED[name]
    w, states, A, kw = random_case(net, n, head, seed=3)
    pol = Policy(w, lib_path=be.lib)
    got = run_grad(be, pol, net, tr.pack_params(w), head, states, **kw)
    ref = torch_reference_grads(w, states, head, kw)
    mine = blocks(net, A, got["grads"])
    err = {k: float(np.linalg.norm(mine[k] - ref[k]) / np.linalg.norm(ref[k])) for k in tr.KEYS}
    print("unrounded %s: " % name + "  ".join("%s %.2g" % (k, err[k]) for k in tr.KEYS))
    for k in tr.KEYS:
        assert err[k] <= bounds[k], (k, err[k], bounds[k])


@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_the_unrounded_net(emu_lib, name):
    check_unrounded(Emu(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_the_unrounded_net_gpu(hip_lib, name):
    check_unrounded(Gpu(hip_lib), name)


# ---------------------------------------------------------------- 6. the step

def run_step(be, pol, params, mom, grads, lr, mo, wd=0.0, gs=1.0):
    d = [be.put(np.asarray(a, np.float32)) for a in (params, mom, grads)]
    tr.sgd_step_device(pol, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), params.size, lr, mo, wd, gs, stream=be.stream, lib=None if pol is not None else _lib(be))
    return be.get(d[0]), be.get(d[1]), d


def _lib(be):
    from deepmimic_amd.core import load_library
    return load_library(be.lib)


def check_step(be):
    net = NET_B
    S, H1, H2, A = net["S"], net["H1"], net["H2"], net["A"]
    w = net_weights(net, seed=2)
    pol = Policy(w, lib_path=be.lib)
    flat = tr.pack_params(w); P = flat.size
    rng = np.random.default_rng(8)
    mom, grads = rng.standard_normal(P).astype(np.float32) * 0.1, rng.standard_normal(P).astype(np.float32)
    mask = tr.matrix_mask_of(S, H1, H2, A)
    lr, mo, wd, gs = 0.01, 0.9, 1e-3, 0.5
    p1, v1, dev = run_step(be, pol, flat, mom, grads, lr, mo, wd, gs)
    pe, ve = tr.reference_step(flat, mom, grads, lr, mo, wd, gs, mask)
    assert np.array_equal(p1, pe) and np.array_equal(v1, ve)                      # the kernel's bits
    p64, v64 = tr.reference_step(flat, mom, grads, lr, mo, wd, gs, mask, exact=False)
    assert (np.abs(p1 - p64) <= np.spacing(np.abs(p64))).all() and (np.abs(v1 - v64) <= np.spacing(np.abs(v64))).all()       # 1 ulp of the float64 mirror rounded once
    # biases are untouched by weight_decay, grad_scale is honoured
    p0, v0, _ = run_step(be, None, flat, mom, grads, lr, mo, 0.0, gs)
    assert np.array_equal(p0[~mask], p1[~mask]) and not np.array_equal(p0[mask], p1[mask])
    pg, vg, _ = run_step(be, None, flat, mom, grads, lr, mo, 0.0, 1.0)
    assert np.array_equal(vg, tr.reference_step(flat, mom, grads, lr, mo, 0.0, 1.0)[1]) and not np.array_equal(vg, v0)
    # exact on integer-valued inputs (lr, momentum, scale powers of two)
    ip, iv, ig = (rng.integers(-8, 9, P).astype(np.float32) for _ in range(3))
    pi_, vi_, _ = run_step(be, None, ip, iv, ig, 0.25, 0.5, 0.0, 2.0)
    assert np.array_equal(vi_, 0.5 * iv + 2 * ig) and np.array_equal(pi_, ip - 0.25 * (0.5 * iv + 2 * ig))
    # the context was refreshed: its packed arrays are byte for byte those of a fresh Policy from the new masters, and the next forward sees them
    fresh = Policy(dict(w, **blocks(net, A, p1)), lib_path=be.lib)
    for k in ("w1p", "w2p", "w3p", "b1", "b2", "b3"):
        assert np.array_equal(pol.read_packed(k), fresh.read_packed(k)), k
    states = rng.standard_normal((5, S)).astype(np.float32)
    outs = []
    for q in (pol, fresh, Policy(w, lib_path=be.lib)):
        d_s, d_a = be.put(states), be.put(np.zeros((5, A), np.float32))
        q.forward_device(be.ptr(d_s), 5, be.ptr(d_a), stream=be.stream)
        outs.append(be.get(d_a))
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


def test_step(emu_lib):
    check_step(Emu(emu_lib))


@pytest.mark.gpu
def test_step_gpu(hip_lib):
    check_step(Gpu(hip_lib))


# ---------------------------------------------------------------- 7. determinism

def check_determinism(be, net, n):
    w, states, A, kw = random_case(net, n, "actor", seed=6)
    flat = tr.pack_params(w)
    runs = []
    for _ in range(2):
        pol = Policy(w, lib_path=be.lib)
        got = run_grad(be, pol, net, flat, "actor", states, **kw)
        p, v, _ = run_step(be, pol, flat, np.zeros_like(flat), got["grads"], 1e-3, 0.9, 1e-4, 1.0)
        runs.append((got["grads"].tobytes(), got["stats"].tobytes(), got["ws_bytes"], got["out"].tobytes(), p.tobytes(), v.tobytes(), pol.read_packed("w2p").tobytes()))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("net,n", [(NET_B, 130), (NET_REF, 33)], ids=["B-130", "ref-33"])
def test_determinism(emu_lib, net, n):
    check_determinism(Emu(emu_lib), net, n)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", [(NET_B, 130), (NET_REF, 33)], ids=["B-130", "ref-33"])
def test_determinism_gpu(hip_lib, net, n):
    check_determinism(Gpu(hip_lib), net, n)


# ---------------------------------------------------------------- 8. it trains

def check_it_trains(be):
    """a critic on 256 fixed rows, targets a fixed linear map of the observations, 30 momentum steps through CriticTrainer: the loss statistic ends strictly below where it
    started.  The distance of the masters to the float64-accumulating mirror of the same recursion is printed, not gated (a bf16 rounding that lands on the other side moves
    a whole trajectory).  Measured: loss 0.726 -> 0.113, max |master - mirror| 9.5e-7, the same on the emulator and on the MI355X."""
    import torch
    net, n, steps = NET_A, 256, 30
    w = net_weights(net, seed=4, A=1)
    rng = np.random.default_rng(12)
    states = rng.standard_normal((n, net["S"])).astype(np.float32)
    targets = ((states - w["s_mean"]) / w["s_std"] @ rng.uniform(-0.3, 0.3, net["S"])).astype(np.float32)
    pol = Policy(w, lib_path=be.lib)
    dev = torch.device(be.device())
    trn = tr.CriticTrainer.from_policy(pol, w, stepsize=0.01, momentum=0.9, device=dev)
    d_s, d_t = torch.from_numpy(states).to(dev), torch.from_numpy(targets).to(dev)
    ref_w = {k: np.array(v, np.float32) for k, v in w.items()}; ref_m = np.zeros(trn.P, np.float32)
    losses, dist = [], 0.0
    for it in range(steps):
        trn.grad(d_s, d_t)
        losses.append(float(trn.stats().cpu()[0]))
        trn.step()
        g = tr.reference_grad(ref_w, states, "critic", targets=targets)["grads"]
        flat, ref_m = tr.reference_step(tr.pack_params(ref_w), ref_m, g, 0.01, 0.9)
        ref_w.update(blocks(net, 1, flat))
        dist = float(np.abs(trn.params.cpu().numpy() - flat).max())
    print("critic training: loss %.4g -> %.4g in %d steps; max |master - mirror| = %.3g" % (losses[0], losses[-1], steps, dist))
    assert losses[-1] < losses[0] and np.isfinite(losses).all()
    # the context holds the trained net: values through the sampling entry point are those of a fresh Policy from the masters
    fresh = Policy(dict(w, **blocks(net, 1, trn.params.cpu().numpy())), lib_path=be.lib)
    assert np.array_equal(pol.read_packed("w1p"), fresh.read_packed("w1p")) and np.array_equal(pol.read_packed("b3"), fresh.read_packed("b3"))


def test_it_trains(emu_lib):
    check_it_trains(Emu(emu_lib))


@pytest.mark.gpu
def test_it_trains_gpu(hip_lib):
    check_it_trains(Gpu(hip_lib))


# ---------------------------------------------------------------- 10. refusals

def check_refusals(be):
    """every refusal of include/dm_hip.h by name, nothing written: the outputs keep their sentinels"""
    net, n = NET_A, 4
    w = net_weights(net, seed=3); wc = net_weights(net, seed=3, A=1)
    A, S = net["A"], net["S"]
    actor, critic = Policy(w, lib_path=be.lib), Policy(wc, lib_path=be.lib)
    gated = Policy(random_weights(S, A, H1=64, H2=64, seed=1, gated_goal_dim=3, gate_common=32, gate_hidden=32), lib_path=be.lib)
    P, Pc = tr.param_count(actor), tr.param_count(critic)
    nb = tr.workspace_bytes(actor, n)
    f = lambda *shape: be.put(np.zeros(shape, np.float32))
    sent = lambda *shape: be.put(np.full(shape, -77.0, np.float32))
    params, states, goals, actions, vec = f(P), f(n, S), f(n, 3), f(n, A), f(n)
    grads, out, stats, ws = sent(P), sent(n), be.put(np.full(6, -77.0)), be.put(np.full(nb // 8 + 2, -77.0))
    p = be.ptr
    def actor_call(pol=actor, params_=params, n_=n, ws_=None, nb_=nb, stats_=None, goal=(0, 0), clip=0.2, bw=10.0, lo=None, hi=None, actions_=actions):
        tr.actor_grad_device(pol, p(params_) if params_ is not None else 0, p(states), n_, p(actions_) if actions_ is not None else 0, p(vec), p(vec), p(grads),
                             p(stats) if stats_ is None else stats_, p(ws) if ws_ is None else ws_, nb_, clip, bw, lo, hi, goals_ptr=goal[0], goal_dim=goal[1],
                             logp_ptr=p(out), stream=be.stream)
    def value_call(pol=critic, n_=n, nb_=nb, targets=vec):
        tr.value_grad_device(pol, p(params), p(states), n_, p(targets) if targets is not None else 0, p(grads), p(stats), p(ws), nb_, values_ptr=p(out), stream=be.stream)
    def step_call(pol=actor, P_=P, lr=0.01, mo=0.9, wd=0.0, gs=1.0, g=grads):
        tr.sgd_step_device(pol, p(params), p(grads), p(g) if g is not None else 0, P_, lr, mo, wd, gs, stream=be.stream, lib=_lib(be))
    cases = [("gated context", lambda: actor_call(pol=gated)), ("gated context", lambda: value_call(pol=gated)), ("gated context", lambda: step_call(pol=gated)),
             ("n must be >= 1", lambda: actor_call(n_=0)), ("n must be >= 1", lambda: value_call(n_=0)),
             ("null argument", lambda: actor_call(params_=None)), ("null argument", lambda: actor_call(actions_=None)), ("null argument", lambda: value_call(targets=None)),
             ("null argument", lambda: step_call(g=None)),
             ("workspace too small", lambda: actor_call(nb_=nb - 1)), ("workspace too small", lambda: value_call(nb_=16)),
             ("16-byte", lambda: actor_call(ws_=p(ws) + 8, nb_=nb)), ("8-byte aligned", lambda: actor_call(stats_=p(stats) + 4)),
             ("goal_dim must be in", lambda: actor_call(goal=(p(goals), S))), ("goal_dim must be in", lambda: actor_call(goal=(0, 3))),
             ("ratio_clip must be > 0", lambda: actor_call(clip=0.0)), ("ratio_clip must be > 0", lambda: actor_call(clip=float("nan"))),
             ("bound_weight must be >= 0", lambda: actor_call(bw=-1.0)),
             ("come together", lambda: actor_call(lo=np.zeros(A, np.float32))),
             ("the value head needs a net with one output", lambda: value_call(pol=actor)),
             ("stepsize must be finite", lambda: step_call(lr=-1.0)), ("stepsize must be finite", lambda: step_call(lr=float("inf"))),
             ("momentum must be finite", lambda: step_call(mo=float("nan"))), ("weight_decay must be finite", lambda: step_call(wd=-1e-3)),
             ("grad_scale must be finite", lambda: step_call(gs=float("inf"))),
             ("parameters", lambda: step_call(P_=P - 1)), ("P must be >= 1", lambda: step_call(pol=None, P_=0)), ("weight_decay needs the net", lambda: step_call(pol=None, wd=0.1))]
    for what, call in cases:
        with pytest.raises(RuntimeError, match=what):
            call()
    with pytest.raises(RuntimeError, match="gated context"):
        tr.param_count(gated)
    with pytest.raises(RuntimeError, match="gated context"):
        tr.workspace_bytes(gated, 4)
    with pytest.raises(RuntimeError, match="n must be >= 1"):
        tr.workspace_bytes(actor, 0)
    for name, t in dict(grads=grads, out=out, stats=stats, ws=ws).items():
        assert (be.get(t) == -77).all(), name
    assert not be.get(params).any()


def test_refusals(emu_lib):
    check_refusals(Emu(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    check_refusals(Gpu(hip_lib))
