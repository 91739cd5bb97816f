"""The PPO actor / critic minibatch updates of the GATED nets (deepmimic_amd/csrc/dm_train_gated.h, include/dm_hip.h dm_train_gated_*, deepmimic_amd/train.py
Gated*Trainer, reference_gated_*) against the numpy statements beside the binding.  Every check runs on the emulator library through host addresses and again, marked
`gpu`, through torch tensors (the Emu / Gpu back ends, gamma and the bf16-interval test of tests/test_train.py).

Shapes (S incl. G, G, H1, H2, A, GC, GH): GA = (37, 3, 64, 64, 3, 32, 32) -- one k-step everywhere, the one-wave layer kernels -- with rows in {1, 15, 16, 17, 33, 65, 130};
GB = (70, 35, 128, 192, 33, 96, 64) -- KG = 64, a three-tile GC, two k-steps in the gate, the tiled layer kernels, N3 = 64 -- with rows in {1, 33, 130}; the reference's
(200, 3, 1024, 512, 36, 128, 64) once at n = 33.

How a device result is held to the mirror: as in tests/test_train.py.  On exact inputs (small integers, sigma in {0, 1, 2}) the whole call bit for bit; on random inputs
stage by stage from the DEVICE's own operands, a contraction of length k within gamma_k sum|a||b| of the float64 one, a stage that ends in a bf16 rounding inside the bf16
interval of that (rounding is monotone)."""
import numpy as np
import pytest

from deepmimic_amd import train as tr
from deepmimic_amd.policy import Policy, random_weights
from test_train import Emu, Gpu, U, gamma, in_bf16_interval

GA = dict(S=37, G=3, H1=64, H2=64, A=3, GC=32, GH=32)
GB = dict(S=70, G=35, H1=128, H2=192, A=33, GC=96, GH=64)
GREF = dict(S=200, G=3, H1=1024, H2=512, A=36, GC=128, GH=64)
ROWS = {"GA": [1, 15, 16, 17, 33, 65, 130], "GB": [1, 33, 130]}
NETS = dict(GA=GA, GB=GB)
INDEX_CASES = [(name, n, head) for name in ("GA", "GB") for n in ROWS[name] for head in ("actor", "critic")]
INDEX_IDS = ["%s-%d-%s" % c for c in INDEX_CASES]
STAGES = ("du1", "du0", "da1", "da0", "xg", "c", "e0", "e1", "dze0", "dze1", "dzc")
PACKED = ("w1p", "b1", "w2p", "b2", "w3p", "b3", "gate_wcp", "gate_bc", "gate_wep0", "gate_be0", "gate_wbp0", "gate_bb0", "gate_wsp0", "gate_bs0",
          "gate_wep1", "gate_be1", "gate_wbp1", "gate_bb1", "gate_wsp1", "gate_bs1")          # the packed array of each entry of tr.GATED_KEYS


def dims(net, A=None):
    return net["S"], net["H1"], net["H2"], net["A"] if A is None else A, net["G"], net["GC"], net["GH"]


def gated_weights(net, seed=1, A=None):
    """random gated weights with normalisers and non-zero biases everywhere (a zero bias hides a bias gradient that lands in the wrong place less well than a random one)"""
    S, H1, H2, A, G, GC, GH = dims(net, A)
    w = random_weights(S, A, H1=H1, H2=H2, seed=seed, init_output_scale=0.3, gated_goal_dim=G, gate_common=GC, gate_hidden=GH)
    rng = np.random.default_rng(seed + 100)
    f = np.float32
    w["s_mean"] = rng.uniform(-0.5, 0.5, S).astype(f); w["s_std"] = rng.uniform(0.5, 2.0, S).astype(f)
    w["a_mean"] = rng.uniform(-0.2, 0.2, A).astype(f); w["a_std"] = rng.uniform(0.5, 2.0, A).astype(f)
    w["logstd"] = rng.uniform(-2.0, -0.5, A).astype(f)
    for k in tr.GATED_KEYS[1::2]:
        w[k] = rng.uniform(-0.1, 0.1, w[k].shape).astype(f)
    return w


def run_gated(be, pol, net, flat, head, states, split=True, **kw):
    """one dm_train_gated_*_grad call on sentinel-filled outputs: dict(grads, stats, out, every workspace piece, s16 / h1 / h2 as bf16 VALUES, sigma / beta); `states` holds
    the goal columns, split: they go in as the goal block (goal_dim = G), else inside the state rows (goal_dim = 0)"""
    n, G, A = states.shape[0], net["G"] if split else 0, pol.A
    P = tr.gated_param_count(pol)
    nb = tr.gated_workspace_bytes(pol, n)
    lay = tr.gated_workspace_layout(net["H1"], net["H2"], A, net["G"], net["GC"], net["GH"], n)
    assert nb == lay["bytes"] and nb % 16 == 0 and P == flat.size
    d = dict(params=be.put(flat), states=be.put(states[:, :net["S"] - G]), goals=be.put(states[:, net["S"] - G:]) if G else None,
             grads=be.put(np.full(P, np.nan, np.float32)), stats=be.put(np.full(6 if head == "actor" else 2, np.nan)), out=be.put(np.full(n, np.nan, np.float32)),
             ws=be.put(np.zeros(nb // 8)))
    common = dict(goals_ptr=be.ptr(d["goals"]) if G else 0, goal_dim=G, stream=be.stream, gated=True)
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
    for k in ("z3", "dz3", "dz2", "dz1") + STAGES:
        off, dt, shape = lay[k]
        out[k] = raw[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape).copy()
    for k in tr.GATED_READ:
        a = tr.read_gated(pol, k, n)
        out[k] = tr.bf16_value(a) if a.dtype == np.uint16 else a
    out["ws_bytes"] = raw.tobytes()
    return out


def grad_blocks(net, A, flat):
    return tr.unpack_gated_params(flat, *dims(net, A))


# ---------------------------------------------------------------- 1. exact inputs, bit for bit

def integer_case(net, n, head, seed=0):
    """Inputs on which every product and sum is exact, in the manner of tests/test_train.py integer_case: states with three small non-zeros per row and a live last column
    (which lies in the goal block), small integer weights, so that xg, c, e_i, beta_i, h_i and every gradient stage are small integers or half-integers.  The sigma
    projection has ONE entry of +-128 per column and a bias in {-128, 0, 128}: its pre-activation is 128 times an integer, so sigma is exactly 1 (0), 2 (>= 128) or 0
    (<= -128) on device, emulator and numpy alike (dm_policy.h gate_sigma).  Head inputs as there: a_std = 2, ratio = 1, adv / target errors / bound_weight multiples of n."""
    S, H1, H2, A, G, GC, GH = dims(net, None if head == "actor" else 1)
    rng = np.random.default_rng([seed, S, n, 21])
    f = np.float32
    def sparse(rows, cols, per_col, vals):
        m = np.zeros((rows, cols), f)
        for c in range(cols):
            m[rng.choice(rows, size=min(per_col, rows), replace=False), c] = rng.choice(vals, size=min(per_col, rows))
        return m
    w = dict(w1=rng.integers(-1, 2, (S, H1)).astype(f), b1=rng.integers(-1, 2, H1).astype(f), w2=sparse(H1, H2, 2, [-1, 1]), b2=rng.integers(-1, 2, H2).astype(f),
             w3=sparse(H2, A, H2 if A == 1 else 6, [-1, 1]), b3=rng.integers(-2, 3, A).astype(f), s_mean=np.ones(S, f), s_std=np.full(S, 2, f), a_mean=np.ones(A, f), a_std=np.full(A, 2, f),
             logstd=np.zeros(A, f), goal_dim=G, gc_w=sparse(G, GC, 2, [-1, 1]), gc_b=rng.integers(0, 2, GC).astype(f))
    for i, H in ((0, H1), (1, H2)):
        w.update({"g%d_w" % i: sparse(GC, GH, 2, [-1, 1]), "g%d_b" % i: rng.integers(0, 2, GH).astype(f),
                  "g%d_bias_w" % i: sparse(GH, H, 1, [-1, 1]), "g%d_bias_b" % i: rng.integers(-1, 2, H).astype(f),
                  "g%d_scale_w" % i: sparse(GH, H, 1, [-128, 128]), "g%d_scale_b" % i: rng.choice([-128, 0, 0, 0, 128], size=H).astype(f)})
    states = np.ones((n, S), f)                                     # (s - 1) / 2 = 0 except where set
    for i in range(n):
        states[i, rng.choice(S, size=3, replace=False)] = 1 + 2 * rng.choice([-1, 1, 2], size=3)
    states[:, S - 1] = 3
    return w, states, A, rng


def check_indexing(be, net, n, head):
    w, states, A, rng = integer_case(net, n, head)
    flat = tr.pack_gated_params(w)
    pol = Policy(w, lib_path=be.lib)
    fwd = tr.reference_gated_forward_bf16(w, states)
    z3 = fwd["z3"]
    assert np.abs(fwd["h1"]).max() < 256 and np.abs(fwd["h2"]).max() < 256 and (z3 == np.round(z3)).all()
    sig = np.concatenate([fwd["sigma0"].ravel(), fwd["sigma1"].ravel()])
    assert set(np.unique(sig)) == {0.0, 1.0, 2.0}                  # the case reaches all three, and nothing else
    m = rng.integers(-2, 3, n).astype(np.float32); m[0] = 2          # (row 0 always sends a gradient: n = 1)
    if head == "actor":
        actions = (1 + 2 * (z3 + rng.integers(-2, 3, z3.shape))).astype(np.float32)
        old = tr.reference_actor_head(z3, actions, np.zeros(n), np.zeros(n), w["a_mean"], w["a_std"], w["logstd"])["logp"]
        lo = np.full(A, -np.inf, np.float32); hi = np.full(A, np.inf, np.float32)
        lo[0] = 1 + 2 * np.median(z3[:, 0]); hi[A - 1] = 1 + 2 * np.median(z3[:, A - 1])
        kw = dict(actions=actions, old_logp=old, adv=m * n, bound_weight=float(n), a_bound_min=lo, a_bound_max=hi)
    else:
        kw = dict(targets=z3[:, 0] - m * n)
    ref = tr.reference_gated_grad(w, states, head, **kw)
    for i in (0, 1):                                                # every dp u 0.5 is exact in bf16
        x = ref["dp%d" % i].astype(np.float64) * ref["u%d" % i] * 0.5
        assert np.array_equal(tr.bf16_round(x.astype(np.float32)).astype(np.float64), x), i
    got = run_gated(be, pol, net, flat, head, states, **kw)
    for k in ("s16", "h1", "h2"):
        assert np.array_equal(got[k][:, :ref[k].shape[1]], ref[k]) and not got[k][:, ref[k].shape[1]:].any(), k
    for k in ("sigma0", "beta0", "sigma1", "beta1"):
        assert np.array_equal(got[k], ref[k]), k
    G = net["G"]
    assert np.array_equal(tr.bf16_value(got["xg"])[:, :G], ref["xg"]) and not got["xg"][:, G:].any()
    assert np.array_equal(got["z3"][:, :A], ref["z3"]) and not got["z3"][:, A:].any()
    assert np.array_equal(got["dz3"], ref["dz3"])
    for k, rk in [("dz2", "dp1"), ("dz1", "dp0")] + [(k, k) for k in STAGES[:4] + STAGES[5:]]:
        assert np.array_equal(tr.bf16_value(got[k]), ref[rk]), k
    mine = grad_blocks(net, A, got["grads"])
    for k in tr.GATED_KEYS:
        assert np.array_equal(mine[k], ref["grads"][k]), k
        assert mine[k].any() or n == 1, k                           # an array that was never written would be NaN; one that was written as zeros proves nothing
    assert np.isfinite(got["grads"]).all()
    assert np.array_equal(got["out"], ref["logp"] if head == "actor" else ref["values"])
    exact = [0, 1, 2, 3, 4] if head == "actor" else [0, 1]
    assert np.array_equal(got["stats"][exact], ref["stats"][exact]), (got["stats"], ref["stats"])
    if head == "actor":
        assert abs(got["stats"][5] - ref["stats"][5]) <= 1e-13 * abs(ref["stats"][5])


@pytest.mark.parametrize("name,n,head", INDEX_CASES, ids=INDEX_IDS)
def test_exact_inputs_bit_for_bit(emu_lib, name, n, head):
    check_indexing(Emu(emu_lib), NETS[name], n, head)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,head", INDEX_CASES, ids=INDEX_IDS)
def test_exact_inputs_bit_for_bit_gpu(hip_lib, name, n, head):
    check_indexing(Gpu(hip_lib), NETS[name], n, head)


# ---------------------------------------------------------------- 2. random inputs, stage by stage

def random_case(net, n, head, seed=0):
    A = net["A"] if head == "actor" else 1
    w = gated_weights(net, seed=seed + 1, A=A)
    rng = np.random.default_rng([seed, net["S"], n, 7])
    states = (rng.standard_normal((n, net["S"])) * 1.5 + 0.2).astype(np.float32)
    if head == "actor":
        z3 = tr.reference_gated_forward_bf16(w, states)["z3"]
        sg = np.exp(w["logstd"])
        actions = ((z3 + sg * rng.standard_normal(z3.shape)) * w["a_std"] + w["a_mean"]).astype(np.float32)
        lp = tr.reference_actor_head(z3, actions, np.zeros(n), np.zeros(n), w["a_mean"], w["a_std"], w["logstd"])["logp"]
        old = (lp + rng.uniform(-0.4, 0.4, n)).astype(np.float32)
        kw = dict(actions=actions, old_logp=old, adv=rng.standard_normal(n).astype(np.float32), ratio_clip=0.2, bound_weight=10.0,
                  a_bound_min=(w["a_mean"] - 0.3 * w["a_std"]).astype(np.float32), a_bound_max=(w["a_mean"] + 0.3 * w["a_std"]).astype(np.float32))
    else:
        kw = dict(targets=rng.standard_normal(n).astype(np.float32))
    return w, states, A, kw


def check_stages(got, w, states, A, head, kw):
    """every stage from the device's own operands (module docstring); W: the RNE bf16 of a master, what both passes multiply by"""
    f64 = np.float64
    n = states.shape[0]
    S, H1, H2, _, G, GC, GH = tr.gated_dims(w)
    W = lambda k: tr.bf16_round(w[k]).astype(f64)
    val = lambda k: tr.bf16_value(got[k]).astype(f64)
    # ---- forward
    assert np.array_equal(got["s16"][:, :S], tr.reference_gated_forward_bf16(w, states)["s16"]) and not got["s16"][:, S:].any()
    xg, c, e = val("xg"), val("c"), [val("e0"), val("e1")]
    assert np.array_equal(xg[:, :G], got["s16"][:, S - G:S]) and not xg[:, G:].any()
    def lin(a, wk, bk):                                     # the float64 contraction with its bias and the fp32 accumulation bound gamma_(k + 1) sum|a||b|
        b = W(wk)
        return a @ b + w[bk], gamma(a.shape[1] + 1) * (np.abs(a) @ np.abs(b) + np.abs(w[bk]))
    pre, bound = lin(xg[:, :G], "gc_w", "gc_b")
    in_bf16_interval(got["c"], np.maximum(pre, 0), bound, "c")
    ins = [got["s16"][:, :S].astype(f64), got["h1"].astype(f64), got["h2"].astype(f64)]
    u64, ub = [None, None], [None, None]
    for i in (0, 1):
        pre, bound = lin(c, "g%d_w" % i, "g%d_b" % i)
        in_bf16_interval(got["e%d" % i], np.maximum(pre, 0), bound, "e%d" % i)
        beta, bb = lin(e[i], "g%d_bias_w" % i, "g%d_bias_b" % i)
        assert (np.abs(got["beta%d" % i] - beta) <= bb + 1e-300).all(), "beta%d" % i
        z, bz = lin(e[i], "g%d_scale_w" % i, "g%d_scale_b" % i)
        sg = got["sigma%d" % i].astype(f64)
        sig64 = lambda t: 2.0 / (1.0 + np.exp(-t))
        ulp4 = 4 * np.spacing(got["sigma%d" % i]).astype(f64)     # expf is the platform's
        assert ((sg >= sig64(z - bz) - ulp4) & (sg <= sig64(z + bz) + ulp4)).all(), "sigma%d" % i
        u64[i], ub[i] = lin(ins[i], "w%d" % (i + 1), "b%d" % (i + 1))
        p = sg * u64[i] + got["beta%d" % i]
        in_bf16_interval(got["h%d" % (i + 1)], np.maximum(p, 0), np.abs(sg) * ub[i], "h%d" % (i + 1))          # relu is monotone and 1-Lipschitz
    z3, b3 = lin(ins[2], "w3", "b3")
    assert (np.abs(got["z3"][:, :A] - z3) <= b3).all() and not got["z3"][:, A:].any()
    # ---- the head from the device's z3: the same bits
    if head == "actor":
        hd = tr.reference_actor_head(got["z3"], a_mean=w["a_mean"], a_std=w["a_std"], logstd=w["logstd"], **kw)
        assert np.array_equal(got["out"], hd["logp"])
    else:
        hd = tr.reference_value_head(got["z3"], **kw)
        assert np.array_equal(got["out"], hd["values"])
    assert np.array_equal(got["dz3"], hd["dz3"]) and not got["dz3"][:, A:].any()
    assert np.allclose(got["stats"], hd["stats"], rtol=1e-13, atol=1e-300), (got["stats"], hd["stats"])
    # ---- backward
    dz3 = val("dz3")[:, :A]
    dp, du, da, dze, dzc = [val("dz1"), val("dz2")], [val("du0"), val("du1")], [val("da0"), val("da1")], [val("dze0"), val("dze1")], val("dzc")
    def back(what, h, *pairs):                               # bf16((sum over the pairs of dz W^T) . [h != 0]) in its interval
        x = sum(dz @ W(k).T for dz, k in pairs)
        bound = gamma(sum(dz.shape[1] for dz, _ in pairs)) * sum(np.abs(dz) @ np.abs(W(k)).T for dz, k in pairs)
        in_bf16_interval(got[what], np.where(h != 0, x, 0.0), np.where(h != 0, bound, 0.0), what)
    back("dz2", got["h2"], (dz3, "w3"))
    back("dz1", got["h1"], (du[1], "w2"))
    for i in (0, 1):
        sg32 = got["sigma%d" % i]
        du_ref, _ = tr.reference_gate_split(tr.bf16_value(got["dz%d" % (i + 1)]), np.zeros_like(sg32), sg32)
        assert np.array_equal(du[i], du_ref), "du%d" % i     # exact from the device's dp and sigma
        sg = sg32.astype(f64); ds = sg * (1.0 - 0.5 * sg)
        x = (dp[i] * u64[i]) * ds
        in_bf16_interval(got["da%d" % i], x, ub[i] * np.abs(dp[i] * ds) + 6 * U * np.abs(x), "da%d" % i)          # 3 ulp of fp32: the product, t and ds, the last product
        back("dze%d" % i, e[i], (dp[i], "g%d_bias_w" % i), (da[i], "g%d_scale_w" % i))
    back("dzc", c, (dze[0], "g0_w"), (dze[1], "g1_w"))
    mine = tr.unpack_gated_params(got["grads"], S, H1, H2, A, G, GC, GH)
    pairs = dict(w3=(ins[2], dz3), w2=(ins[1], du[1]), w1=(ins[0], du[0]), gc_w=(xg[:, :G], dzc))
    for i in (0, 1):
        pairs.update({"g%d_bias_w" % i: (e[i], dp[i]), "g%d_scale_w" % i: (e[i], da[i]), "g%d_w" % i: (c, dze[i])})
    assert len(pairs) == 10
    for wk, (a, dz) in pairs.items():
        bk = tr.GATED_KEYS[tr.GATED_KEYS.index(wk) + 1]
        assert (np.abs(mine[wk] - a.T @ dz) <= gamma(n) * (np.abs(a).T @ np.abs(dz)) + 1e-300).all(), wk
        assert (np.abs(mine[bk] - dz.sum(axis=0)) <= gamma(n) * np.abs(dz).sum(axis=0) + 1e-300).all(), bk
    assert np.isfinite(got["grads"]).all()


def check_random(be, net, n, head):
    w, states, A, kw = random_case(net, n, head)
    pol = Policy(w, lib_path=be.lib)
    got = run_gated(be, pol, net, tr.pack_gated_params(w), head, states, **kw)
    check_stages(got, w, states, A, head, kw)
    for k, v in grad_blocks(net, A, got["grads"]).items():
        assert v.any(), k


RANDOM_CASES = [(GA, 17, "actor"), (GA, 130, "critic"), (GB, 1, "actor"), (GB, 33, "critic"), (GB, 130, "actor"), (GREF, 33, "actor")]
RANDOM_IDS = ["GA-17-actor", "GA-130-critic", "GB-1-actor", "GB-33-critic", "GB-130-actor", "ref-33-actor"]


@pytest.mark.parametrize("net,n,head", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage(emu_lib, net, n, head):
    check_random(Emu(emu_lib), net, n, head)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n,head", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage_gpu(hip_lib, net, n, head):
    check_random(Gpu(hip_lib), net, n, head)


# ---------------------------------------------------------------- 3. the algebra against autograd (CPU only)

def torch_gated_grads(w, states, head, kw):
    """float64 autograd of the gated net on the fp32 masters, nothing rounded: PPO surrogate + bound loss, or 0.5 MSE"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    p = {k: t(w[k]).requires_grad_(True) for k in tr.GATED_KEYS}
    S, G = w["w1"].shape[0], int(w["goal_dim"])
    x = (t(states) - t(w["s_mean"])) * t(np.float32(1) / w["s_std"])
    c = torch.relu(x[:, S - G:] @ p["gc_w"] + p["gc_b"])
    h = x
    for i in (0, 1):
        e = torch.relu(c @ p["g%d_w" % i] + p["g%d_b" % i])
        beta = e @ p["g%d_bias_w" % i] + p["g%d_bias_b" % i]
        sigma = 2 * torch.sigmoid(e @ p["g%d_scale_w" % i] + p["g%d_scale_b" % i])
        h = torch.relu(sigma * (h @ p["w%d" % (i + 1)] + p["b%d" % (i + 1)]) + beta)
    z3 = h @ p["w3"] + p["b3"]
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
    return {k: p[k].grad.numpy() for k in tr.GATED_KEYS}


def rel_to_largest(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("net,n,head", [(GA, 17, "actor"), (GB, 33, "critic"), (GB, 33, "actor")], ids=["GA-17-actor", "GB-33-critic", "GB-33-actor"])
def test_algebra_against_autograd(net, n, head):
    """reference_gated_grad(rounded=False) IS the gradient of the loss: to 1e-9 of each array's largest entry against float64 autograd of the net written out above"""
    w, states, A, kw = random_case(net, n, head, seed=3)
    mine = tr.reference_gated_grad(w, states, head, rounded=False, **kw)["grads"]
    ref = torch_gated_grads(w, states, head, kw)
    for k in tr.GATED_KEYS:
        assert np.abs(ref[k]).max() > 0 and rel_to_largest(mine[k], ref[k]) <= 1e-9, (k, rel_to_largest(mine[k], ref[k]))


# ---------------------------------------------------------------- 4. against the unrounded net

UNROUNDED = {"GB-130-actor": (GB, 130, "actor"), "GA-65-critic": (GA, 65, "critic")}


def check_unrounded(be, name):
    """The device gradients against float64 autograd of the unrounded net, per array, relative to the array's largest entry.  The tolerance is not a device figure: the
    numpy mirror (rounded=True: the device's rounding points, float64 contractions) is held against the same autograd on the same inputs here, and the device is allowed
    twice the mirror's deviation -- the fp32 accumulation order is the only source of error the device has and the mirror has not.  Mirror deviations measured on the CPU
    (the device's own are printed):
      GB-130-actor   w1 6.4e-2 b1 1.7e-2 w2 1.7e-2 b2 9.9e-3 w3 2.2e-2 b3 2.0e-2 gc_w 9.6e-2 gc_b 4.4e-2 g0_w 4.6e-2 g0_b 2.0e-2 g0_bias_w 3.1e-2 g0_bias_b 2.0e-2
                     g0_scale_w 2.0e-2 g0_scale_b 1.4e-2 g1_w 4.9e-2 g1_b 2.2e-2 g1_bias_w 1.4e-2 g1_bias_b 1.4e-2 g1_scale_w 1.9e-2 g1_scale_b 1.3e-2
      GA-65-critic   w1 2.7e-2 b1 1.6e-2 w2 1.0e-1 b2 4.6e-2 w3 4.2e-3 b3 4.1e-3 gc_w 3.9e-2 gc_b 4.3e-2 g0_w 4.1e-2 g0_b 4.6e-2 g0_bias_w 2.2e-2 g0_bias_b 1.7e-2
                     g0_scale_w 1.8e-2 g0_scale_b 3.5e-2 g1_w 1.6e-1 g1_b 6.2e-2 g1_bias_w 3.3e-2 g1_bias_b 4.7e-2 g1_scale_w 4.0e-3 g1_scale_b 5.9e-3
    The emulator and the MI355X deviate by the same figures to the two digits printed: the bf16 rounding points, which the mirror shares, are all of it."""
    net, n, head = UNROUNDED[name]
    w, states, A, kw = random_case(net, n, head, seed=3)
    ref = torch_gated_grads(w, states, head, kw)
    mirror = tr.reference_gated_grad(w, states, head, **kw)["grads"]
    pol = Policy(w, lib_path=be.lib)
    mine = grad_blocks(net, A, run_gated(be, pol, net, tr.pack_gated_params(w), head, states, **kw)["grads"])
    err_m = {k: rel_to_largest(mirror[k], ref[k]) for k in tr.GATED_KEYS}
    err_d = {k: rel_to_largest(mine[k], ref[k]) for k in tr.GATED_KEYS}
    print("unrounded %s mirror: " % name + " ".join("%s %.2g" % (k, err_m[k]) for k in tr.GATED_KEYS))
    print("unrounded %s device: " % name + " ".join("%s %.2g" % (k, err_d[k]) for k in tr.GATED_KEYS))
    for k in tr.GATED_KEYS:
        assert err_d[k] <= 2 * err_m[k], (k, err_d[k], err_m[k])


@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_the_unrounded_net(emu_lib, name):
    check_unrounded(Emu(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_the_unrounded_net_gpu(hip_lib, name):
    check_unrounded(Gpu(hip_lib), name)


# ---------------------------------------------------------------- 5. consistency with the sampling net

def check_sampling_consistency(be, net, n, monkeypatch):
    """Rows sampled by dm_policy_forward_ex on the per-layer gated route, fed back at the masters that sampled: the training forward is the same kernels on the same weights,
    so mu is the same bits, logp_new - logp_old is rounding alone and the mean ratio is 1.  The per-row bound is the one tests/test_train.py check_sampling_consistency
    derives for the plain net (the head is the same code); the goal goes in once as a block and once inside the state rows."""
    monkeypatch.setenv("DM_POLICY_LAYERED", "1")
    w = gated_weights(net, seed=5)
    S, A, G = net["S"], net["A"], net["G"]
    pol = Policy(w, lib_path=be.lib)
    rng = np.random.default_rng([n, S, 3])
    states = (rng.standard_normal((n, S)) * 1.5).astype(np.float32)
    d_s, d_g = be.put(states[:, :S - G]), be.put(states[:, S - G:])
    d_a, d_lp = be.put(np.zeros((n, A), np.float32)), be.put(np.zeros(n, np.float32))
    pol.forward_device_ex(be.ptr(d_s), n, be.ptr(d_a), be.ptr(d_g), G, be.ptr(d_lp), sample=True, seed=11, step=3, stream=be.stream)
    actions, old = be.get(d_a), be.get(d_lp)
    adv = rng.standard_normal(n).astype(np.float32); adv[0] = 0.0
    kw = dict(actions=actions, old_logp=old, adv=adv, ratio_clip=0.2, bound_weight=10.0)
    flat = tr.pack_gated_params(w)
    got = run_gated(be, pol, net, flat, "actor", states, **kw)
    inside = run_gated(be, pol, net, flat, "actor", states, split=False, **kw)
    assert np.array_equal(got["grads"], inside["grads"]) and np.array_equal(got["out"], inside["out"])
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
    print("gated sampling consistency: max |logp_new - logp_old| = %.3g, smallest bound %.3g (A = %d, n = %d)" % (diff.max(), bound.min(), A, n))
    assert (diff <= bound).all(), (diff.max(), bound.min())
    assert got["stats"][3] == 0.0 and abs(got["stats"][4] - 1.0) <= np.expm1(bound.max())       # clip_frac, mean ratio
    assert (hd["g"][adv != 0] != 0).all() and hd["g"][0] == 0


@pytest.mark.parametrize("net,n", [(GA, 17), (GB, 65)], ids=["GA-17", "GB-65"])
def test_sampling_consistency(emu_lib, net, n, monkeypatch):
    check_sampling_consistency(Emu(emu_lib), net, n, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", [(GA, 17), (GB, 65)], ids=["GA-17", "GB-65"])
def test_sampling_consistency_gpu(hip_lib, net, n, monkeypatch):
    check_sampling_consistency(Gpu(hip_lib), net, n, monkeypatch)


# ---------------------------------------------------------------- 6. the step

def run_step(be, pol, params, mom, grads, lr, mo, wd=0.0, gs=1.0):
    d = [be.put(np.asarray(a, np.float32)) for a in (params, mom, grads)]
    tr.gated_sgd_step_device(pol, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), params.size, lr, mo, wd, gs, stream=be.stream)
    return be.get(d[0]), be.get(d[1])


def check_step(be):
    net = GB
    w = gated_weights(net, seed=2)
    pol = Policy(w, lib_path=be.lib)
    flat = tr.pack_gated_params(w); P = flat.size
    rng = np.random.default_rng(8)
    mom, grads = rng.standard_normal(P).astype(np.float32) * 0.1, rng.standard_normal(P).astype(np.float32)
    mask = tr.gated_matrix_mask_of(*dims(net))
    lay = tr.gated_layout(*dims(net))
    assert mask.sum() == sum(int(np.prod(lay[k][1])) for k in tr.GATED_KEYS if len(lay[k][1]) == 2) and sum(len(lay[k][1]) == 2 for k in tr.GATED_KEYS) == 10
    lr, mo, wd, gs = 0.01, 0.9, 1e-3, 0.5
    p1, v1 = run_step(be, pol, flat, mom, grads, lr, mo, wd, gs)
    pe, ve = tr.reference_step(flat, mom, grads, lr, mo, wd, gs, mask)
    assert np.array_equal(p1, pe) and np.array_equal(v1, ve)                      # the kernel's bits, the decay on the ten matrices and on no vector
    p0, _ = run_step(be, Policy(w, lib_path=be.lib), flat, mom, grads, lr, mo, 0.0, gs)
    new, plain = grad_blocks(net, None, p1), grad_blocks(net, None, p0)
    for k in tr.GATED_KEYS:
        assert np.array_equal(new[k], plain[k]) == (new[k].ndim == 1), k
    # the context was refreshed, gate included: all twenty packed arrays are byte for byte those of a fresh Policy from the new masters
    fresh = Policy(dict(w, **new), lib_path=be.lib)
    stale = Policy(w, lib_path=be.lib)
    for k in PACKED:
        assert np.array_equal(pol.read_packed(k), fresh.read_packed(k)), k
        assert not np.array_equal(pol.read_packed(k), stale.read_packed(k)), k


def test_step(emu_lib):
    check_step(Emu(emu_lib))


@pytest.mark.gpu
def test_step_gpu(hip_lib):
    check_step(Gpu(hip_lib))


# ---------------------------------------------------------------- 7. determinism

def check_determinism(be, net, n):
    w, states, A, kw = random_case(net, n, "actor", seed=6)
    flat = tr.pack_gated_params(w)
    runs = []
    for _ in range(2):
        pol = Policy(w, lib_path=be.lib)
        got = run_gated(be, pol, net, flat, "actor", states, **kw)
        runs.append((got["grads"].tobytes(), got["stats"].tobytes(), got["ws_bytes"], got["out"].tobytes()))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("net,n", [(GB, 130), (GREF, 33)], ids=["GB-130", "ref-33"])
def test_determinism(emu_lib, net, n):
    check_determinism(Emu(emu_lib), net, n)


@pytest.mark.gpu
@pytest.mark.parametrize("net,n", [(GB, 130), (GREF, 33)], ids=["GB-130", "ref-33"])
def test_determinism_gpu(hip_lib, net, n):
    check_determinism(Gpu(hip_lib), net, n)


# ---------------------------------------------------------------- 8. it trains

def check_it_trains(be):
    """A gated critic (heads.Critic) on 256 fixed rows whose targets depend on the goal columns only through a product with an observation column -- what a gate is for --
    30 momentum steps through GatedCriticTrainer on the critic's own context: the loss statistic ends below where it started, the gate's masters have moved, and the
    critic evaluates with the trained weights."""
    import torch
    from deepmimic_amd.heads import Critic
    net, n, steps = GA, 256, 30
    w = gated_weights(net, seed=4, A=1)
    S, G = net["S"], net["G"]
    rng = np.random.default_rng(12)
    states = rng.standard_normal((n, S)).astype(np.float32)
    x = (states - w["s_mean"]) / w["s_std"]
    targets = (x[:, S - G:] @ np.array([0.8, -0.6, 0.5])[:G] * x[:, 0]).astype(np.float32)
    critic = Critic(w, lib_path=be.lib)
    dev = torch.device(be.device())
    trn = tr.GatedCriticTrainer.from_policy(critic.net, w, stepsize=0.01, momentum=0.9, device=dev)
    before = {k: v.clone() for k, v in trn.views().items()}
    d_s, d_t = torch.from_numpy(states).to(dev), torch.from_numpy(targets).to(dev)
    losses = []
    for it in range(steps):
        trn.grad(d_s, d_t)
        losses.append(float(trn.stats().cpu()[0]))
        trn.step()
    print("gated critic training: loss %.4g -> %.4g in %d steps" % (losses[0], losses[-1], steps))
    assert losses[-1] < losses[0] and np.isfinite(losses).all()
    after = trn.views()
    for k in tr.GATED_KEYS[6:]:
        assert not torch.equal(before[k], after[k]), k
    fresh = Policy(dict(w, **{k: v.cpu().numpy() for k, v in after.items()}), lib_path=be.lib)
    for k in ("w1p", "b3", "gate_wcp", "gate_wsp1", "gate_bs0"):
        assert np.array_equal(critic.net.read_packed(k), fresh.read_packed(k)), k


def test_it_trains(emu_lib):
    check_it_trains(Emu(emu_lib))


@pytest.mark.gpu
def test_it_trains_gpu(hip_lib):
    check_it_trains(Gpu(hip_lib))


# ---------------------------------------------------------------- 9. refusals

def check_refusals(be):
    """every refusal of the gated entry points by name, nothing written: the outputs keep their sentinels; and the plain entry points still refuse the gated context"""
    net, n = GA, 4
    S, H1, H2, A, G, GC, GH = dims(net)
    w, wc = gated_weights(net, seed=3), gated_weights(net, seed=3, A=1)
    actor, critic = Policy(w, lib_path=be.lib), Policy(wc, lib_path=be.lib)
    plain = Policy({k: w[k] for k in tr.KEYS + ("s_mean", "s_std", "a_mean", "a_std", "logstd")}, lib_path=be.lib)
    P = tr.gated_param_count(actor)
    nb = tr.gated_workspace_bytes(actor, n)
    assert P == tr.gated_layout(*dims(net))["P"] and tr.gated_param_count(critic) == tr.gated_layout(*dims(net, 1))["P"]
    f = lambda *shape: be.put(np.zeros(shape, np.float32))
    sent = lambda *shape: be.put(np.full(shape, -77.0, np.float32))
    params, states, goals, actions, vec = f(P), f(n, S), f(n, G), f(n, A), f(n)
    grads, out, stats, ws = sent(P), sent(n), be.put(np.full(6, -77.0)), be.put(np.full(nb // 8 + 2, -77.0))
    p = be.ptr
    def actor_call(pol=actor, params_=params, n_=n, ws_=None, nb_=nb, stats_=None, goal=(0, 0), clip=0.2, bw=10.0, lo=None, hi=None, actions_=actions, gated=True):
        tr.actor_grad_device(pol, p(params_) if params_ is not None else 0, p(states), n_, p(actions_) if actions_ is not None else 0, p(vec), p(vec), p(grads),
                             p(stats) if stats_ is None else stats_, p(ws) if ws_ is None else ws_, nb_, clip, bw, lo, hi, goals_ptr=goal[0], goal_dim=goal[1],
                             logp_ptr=p(out), stream=be.stream, gated=gated)
    def value_call(pol=critic, n_=n, nb_=nb, targets=vec, gated=True):
        tr.value_grad_device(pol, p(params), p(states), n_, p(targets) if targets is not None else 0, p(grads), p(stats), p(ws), nb_, values_ptr=p(out), stream=be.stream,
                             gated=gated)
    def step_call(pol=actor, P_=P, lr=0.01, mo=0.9, wd=0.0, gs=1.0, g=grads):
        tr.gated_sgd_step_device(pol, p(params), p(grads), p(g) if g is not None else 0, P_, lr, mo, wd, gs, stream=be.stream)
    cases = [("plain context", lambda: actor_call(pol=plain)), ("plain context", lambda: value_call(pol=plain)), ("plain context", lambda: step_call(pol=plain)),
             ("plain context", lambda: tr.gated_param_count(plain)), ("plain context", lambda: tr.gated_workspace_bytes(plain, 4)),
             ("plain context", lambda: tr.read_gated(plain, "h1", 1)),
             ("n must be >= 1", lambda: actor_call(n_=0)), ("n must be >= 1", lambda: value_call(n_=0)), ("n must be >= 1", lambda: tr.gated_workspace_bytes(actor, 0)),
             ("null argument", lambda: actor_call(params_=None)), ("null argument", lambda: actor_call(actions_=None)), ("null argument", lambda: value_call(targets=None)),
             ("null argument", lambda: step_call(g=None)),
             ("workspace too small", lambda: actor_call(nb_=nb - 1)), ("workspace too small", lambda: value_call(nb_=tr.workspace_layout(H1, H2, 1, n)["bytes"])),
             ("16-byte", lambda: actor_call(ws_=p(ws) + 8, nb_=nb)), ("8-byte aligned", lambda: actor_call(stats_=p(stats) + 4)),
             ("goal_dim must be in", lambda: actor_call(goal=(p(goals), S))), ("goal_dim must be in", lambda: actor_call(goal=(0, G))),
             ("the gate's goal_dim", lambda: actor_call(goal=(p(goals), G - 1))), ("the gate's goal_dim", lambda: value_call_goal(G + 1)),
             ("ratio_clip must be > 0", lambda: actor_call(clip=0.0)), ("ratio_clip must be > 0", lambda: actor_call(clip=float("nan"))),
             ("bound_weight must be >= 0", lambda: actor_call(bw=-1.0)),
             ("come together", lambda: actor_call(lo=np.zeros(A, np.float32))),
             ("the value head needs a net with one output", lambda: value_call(pol=actor)),
             ("stepsize must be finite", lambda: step_call(lr=-1.0)), ("stepsize must be finite", lambda: step_call(lr=float("inf"))),
             ("momentum must be finite", lambda: step_call(mo=float("nan"))), ("weight_decay must be finite", lambda: step_call(wd=-1e-3)),
             ("grad_scale must be finite", lambda: step_call(gs=float("inf"))),
             ("parameters", lambda: step_call(P_=P - 1)), ("parameters", lambda: step_call(P_=P + 1)), ("P must be >= 1", lambda: step_call(P_=0)),
             ("null net", lambda: step_call(pol=type("NoNet", (), dict(lib=actor.lib, h=None))())),
             # the plain entry points keep refusing the gated context
             ("gated context", lambda: actor_call(gated=False)), ("gated context", lambda: value_call(gated=False)), ("gated context", lambda: tr.param_count(actor)),
             ("gated context", lambda: tr.workspace_bytes(actor, 4)), ("gated context", lambda: tr.read_activations(actor, "h1", 1)),
             ("gated context", lambda: tr.sgd_step_device(actor, p(params), p(grads), p(grads), P, 0.01, 0.9, stream=be.stream))]
    def value_call_goal(goal_dim):
        tr.value_grad_device(critic, p(params), p(states), n, p(vec), p(grads), p(stats), p(ws), nb, goals_ptr=p(goals), goal_dim=goal_dim, values_ptr=p(out),
                             stream=be.stream, gated=True)
    for what, call in cases:
        with pytest.raises(RuntimeError, match=what):
            call()
    for name, t in dict(grads=grads, out=out, stats=stats, ws=ws).items():
        assert (be.get(t) == -77).all(), name
    assert not be.get(params).any()


def test_refusals(emu_lib):
    check_refusals(Emu(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    check_refusals(Gpu(hip_lib))
