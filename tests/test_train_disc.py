"""The AMP discriminator minibatch update on the device, gradient penalty included (deepmimic_amd/csrc/dm_train.h dm_train_disc_grad, include/dm_hip.h,
deepmimic_amd/train.py DiscTrainer / reference_disc_grad).  Every check runs on the emulator library through host addresses and again, marked `gpu`, through torch tensors,
with the helpers and the conventions of tests/test_train.py (the fp32-contraction bound gamma_k sum|a||b|, the [bf16(x - bound), bf16(x + bound)] interval, stages taken
from the DEVICE's own inputs).

Shapes: the nets (S, H1, H2) = (37, 64, 64) and (70, 128, 192) with one output -- K1 padding on both, a non-power-of-two tile count on the second -- at
(n_expert, n_agent) in {(1, 1), (15, 17), (16, 16), (17, 15), (33, 65), (65, 33), (130, 1)}: the expert / agent boundary inside a 16- and a 32-row tile, on a tile edge,
one side a single row; the reference's widths (226 -> 1024 -> 512 -> 1) once at (33, 31)."""
import numpy as np
import pytest

from deepmimic_amd import heads
from deepmimic_amd import train as tr
from deepmimic_amd.policy import Policy, random_weights
from test_train import Emu, Gpu, U, blocks, gamma, in_bf16_interval, net_weights

NET_A = dict(S=37, G=0, H1=64, H2=64, A=1)
NET_B = dict(S=70, G=0, H1=128, H2=192, A=1)
NET_REF = dict(S=226, G=0, H1=1024, H2=512, A=1)
PAIRS = [(1, 1), (15, 17), (16, 16), (17, 15), (33, 65), (65, 33), (130, 1)]
LS_STAGES, PEN_STAGES = ("z3", "dz3", "dz2", "dz1"), ("g2", "g1", "a", "t1", "t2", "sq")
SIG = tr.DISC_STATS.index("prob_agent")
NOT_SIG = [i for i in range(8) if i != SIG]


def run_disc(be, pol, net, flat, expert, agent, gp, lr, sentinel=np.nan):
    """one dm_train_disc_grad call on sentinel-filled outputs and a zeroed workspace: dict(grads, stats, logits, every workspace stage, s16 / h1 / h2 as bf16 VALUES)"""
    ne, na = expert.shape[0], agent.shape[0]
    n = ne + na
    P = tr.param_count(pol)
    nb = tr.disc_workspace_bytes(pol, ne, na)
    lay = tr.disc_workspace_layout(net["S"], net["H1"], net["H2"], ne, na)
    assert nb == lay["bytes"] and nb % 16 == 0
    d = dict(params=be.put(flat), expert=be.put(np.asarray(expert, np.float32)), agent=be.put(np.asarray(agent, np.float32)), grads=be.put(np.full(P, sentinel, np.float32)),
             stats=be.put(np.full(8, np.nan)), logits=be.put(np.full(n, np.nan, np.float32)), ws=be.put(np.zeros(nb // 8)))
    tr.disc_grad_device(pol, be.ptr(d["params"]), be.ptr(d["expert"]), ne, be.ptr(d["agent"]), na, be.ptr(d["grads"]), be.ptr(d["stats"]), be.ptr(d["ws"]), nb, gp, lr,
                        logits_ptr=be.ptr(d["logits"]), stream=be.stream)
    out = {k: be.get(d[k]) for k in ("grads", "stats", "logits")}
    raw = np.ascontiguousarray(be.get(d["ws"])).view(np.uint8)
    for k in LS_STAGES + PEN_STAGES:
        off, dt, shape = lay[k]
        out[k] = raw[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape).copy()
    for k in ("s16", "h1", "h2"):
        out[k] = tr.bf16_value(tr.read_activations(pol, k, n))
    out["ws_bytes"] = raw.tobytes()
    return out


def disc_weights(net, seed):
    return net_weights(net, seed=seed, A=1)


def random_obs(net, ne, na, seed=0):
    rng = np.random.default_rng([seed, net["S"], ne, na])
    return ((rng.standard_normal((ne, net["S"])) * 1.5 + 0.3).astype(np.float32), (rng.standard_normal((na, net["S"])) * 1.5 - 0.1).astype(np.float32))


# ---------------------------------------------------------------- the stages, each from the device's own inputs

def check_disc_stages(got, w, expert, agent, gp, lr, forward=True):
    """Every stage of one call held to float64 arithmetic on the DEVICE's inputs to that stage.  Bounds: a contraction of length k in fp32 gamma_k sum|a||b| (with the bias
    add k + 1); a stage stored in bf16 lies in the bf16 interval of its bound; element-wise stages (s16, the head from z3, g2 from h2) are exact; a gradient element is
    fl(ls + pen) then one fmaf: the two contraction bounds plus 2u (|ls| + |pen| + |reg|) for the two final roundings; the fp64 statistics to 1e-13 relative.
    sq (fp32 sums of 32 squares of fp32 gx = gx64 + d, |d| <= b): |sq - sum gx64^2| <= sum (2 |gx64| b + b^2) + gamma_34 sum (|gx64| + b)^2."""
    f64 = np.float64
    ne, na = expert.shape[0], agent.shape[0]
    n = ne + na
    S, H1 = w["w1"].shape; H2 = w["w2"].shape[1]; K1 = (S + 63) // 64 * 64
    W1, W2, w3 = (tr.bf16_round(w[k]).astype(f64) for k in ("w1", "w2", "w3"))
    obs = np.concatenate([expert, agent])
    if forward:
        s16_ref = tr.reference_forward_bf16(w, obs)[0]
        assert np.array_equal(got["s16"][:, :S], s16_ref) and not got["s16"][:, S:].any()
        for a, b, bias, hk in ((got["s16"][:, :S].astype(f64), W1, w["b1"], "h1"), (got["h1"].astype(f64), W2, w["b2"], "h2")):
            in_bf16_interval(got[hk], np.maximum(a @ b + bias, 0), gamma(a.shape[1] + 1) * (np.abs(a) @ np.abs(b) + np.abs(bias)), hk)
    h2 = got["h2"].astype(f64)
    z3 = h2 @ w3 + w["b3"]
    assert (np.abs(got["z3"][:, :1] - z3) <= gamma(H2 + 1) * (np.abs(h2) @ np.abs(w3) + np.abs(w["b3"]))).all() and not got["z3"][:, 1:].any()
    # the head from the device's z3: the same bits
    hd = tr.reference_disc_head(got["z3"], ne, na)
    assert np.array_equal(got["dz3"], hd["dz3"]) and np.array_equal(got["logits"], hd["logits"]) and not got["dz3"][:, 1:].any()
    assert np.allclose(got["stats"][:5], hd["stats"], rtol=1e-13, atol=1e-300), (got["stats"], hd["stats"])
    # the least-squares backward pass
    ins = dict(w1=got["s16"][:, :S].astype(f64), w2=got["h1"].astype(f64), w3=h2)
    dz = dict(w3=tr.bf16_value(got["dz3"])[:, :1].astype(f64), w2=tr.bf16_value(got["dz2"]).astype(f64), w1=tr.bf16_value(got["dz1"]).astype(f64))
    for b, hk, src, dk in ((w3, "h2", "w3", "dz2"), (W2, "h1", "w2", "dz1")):
        live = got[hk] != 0
        in_bf16_interval(got[dk], np.where(live, dz[src] @ b.T, 0.0), np.where(live, gamma(b.shape[1]) * (np.abs(dz[src]) @ np.abs(b).T), 0.0), dk)
    ls = {k: ins[k].T @ dz[k] for k in ("w1", "w2", "w3")}
    err = {k: gamma(n) * (np.abs(ins[k]).T @ np.abs(dz[k])) for k in ("w1", "w2", "w3")}
    pen = {k: np.zeros_like(v) for k, v in ls.items()}
    if gp > 0:
        h1e, h2e = got["h1"][:ne], got["h2"][:ne]
        assert np.array_equal(got["g2"], tr.bf16_bits(np.where(h2e != 0, w3[:, 0][None, :], 0.0).astype(np.float32)))
        g2 = tr.bf16_value(got["g2"]).astype(f64)
        in_bf16_interval(got["g1"], np.where(h1e != 0, g2 @ W2.T, 0.0), np.where(h1e != 0, gamma(H2) * (np.abs(g2) @ np.abs(W2).T), 0.0), "g1")
        g1 = tr.bf16_value(got["g1"]).astype(f64)
        gx = np.zeros((ne, K1)); gb = np.zeros((ne, K1))
        gx[:, :S] = g1 @ W1.T; gb[:, :S] = gamma(H1) * (np.abs(g1) @ np.abs(W1).T)
        blk = lambda v: v.reshape(ne, K1 // 32, 32).sum(axis=2)
        sq_bound = blk(2 * np.abs(gx) * gb + gb ** 2) + gamma(34) * blk((np.abs(gx) + gb) ** 2)
        assert (np.abs(got["sq"] - blk(gx ** 2)) <= sq_bound + 1e-300).all(), "sq"
        scale = float(np.float32(gp) / np.float32(ne))
        in_bf16_interval(got["a"], gx * scale, gb * scale + U * np.abs(gx * scale), "a")
        assert not got["a"][:, S:].any()
        a = tr.bf16_value(got["a"])[:, :S].astype(f64)
        in_bf16_interval(got["t1"], np.where(h1e != 0, a @ W1, 0.0), np.where(h1e != 0, gamma(K1) * (np.abs(a) @ np.abs(W1)), 0.0), "t1")
        t1 = tr.bf16_value(got["t1"]).astype(f64)
        in_bf16_interval(got["t2"], np.where(h2e != 0, t1 @ W2, 0.0), np.where(h2e != 0, gamma(H1) * (np.abs(t1) @ np.abs(W2)), 0.0), "t2")
        t2 = tr.bf16_value(got["t2"]).astype(f64)
        pen = dict(w1=a.T @ g1, w2=t1.T @ g2, w3=t2.sum(axis=0)[:, None])
        for k, v in dict(w1=np.abs(a).T @ np.abs(g1), w2=np.abs(t1).T @ np.abs(g2), w3=np.abs(t2).sum(axis=0)[:, None]).items():
            err[k] = err[k] + gamma(ne) * v
        assert abs(got["stats"][5] - 0.5 * got["sq"].astype(f64).sum() / ne) <= 1e-13 * got["stats"][5]
    else:
        assert got["stats"][5] == 0.0
    reg = dict(w1=0.0, w2=0.0, w3=float(np.float32(lr)) * np.asarray(w["w3"], f64).reshape(-1, 1))
    mine = blocks(dict(S=S, H1=H1, H2=H2), 1, got["grads"])
    for k in ("w1", "w2", "w3"):
        want = ls[k] + pen[k] + reg[k]
        bound = err[k] + 2 * U * (np.abs(ls[k]) + np.abs(pen[k]) + np.abs(reg[k])) + 1e-300
        assert (np.abs(mine[k] - want) <= bound).all(), (k, float(np.abs(mine[k] - want).max()))
    for k, bk in (("w1", "b1"), ("w2", "b2"), ("w3", "b3")):
        assert (np.abs(mine[bk] - dz[k].sum(axis=0)) <= gamma(n) * np.abs(dz[k]).sum(axis=0) + 1e-300).all(), bk
    sq = {k: (np.asarray(w[k], f64) ** 2).sum() for k in ("w1", "w2", "w3")}
    assert np.allclose(got["stats"][6:], [0.5 * sq["w3"], 0.5 * (sq["w1"] + sq["w2"] + sq["w3"])], rtol=1e-13, atol=0)
    assert np.isfinite(got["grads"]).all() and np.isfinite(got["stats"]).all()


# ---------------------------------------------------------------- 1. indexing, bit for bit

def integer_disc_case(net, ne, na, seed=0):
    """Inputs on which every product and sum is exact, in the manner of test_train.integer_case, W1 included (gx contracts over H1): observations with three small
    non-zeros per row, sparse weights in {-1, 0, 1}, integer biases, (s - 1) / 2 as the normaliser.  grad_penalty = n_e, so that a = gx exactly; logit_reg = 0.25."""
    rng = np.random.default_rng([seed, net["S"], ne, na])
    S, H1, H2 = net["S"], net["H1"], net["H2"]
    f = np.float32
    def sparse(rows, cols, per_col):
        m = np.zeros((rows, cols), f)
        for c in range(cols):
            m[rng.choice(rows, size=min(per_col, rows), replace=False), c] = rng.choice([-1, 1], size=min(per_col, rows))
        return m
    w = dict(w1=sparse(S, H1, 4), b1=rng.integers(-1, 2, H1).astype(f), w2=sparse(H1, H2, 3), b2=rng.integers(-1, 2, H2).astype(f), w3=sparse(H2, 1, 3),
             b3=rng.integers(-2, 3, 1).astype(f), s_mean=np.ones(S, f), s_std=np.full(S, 2, f))
    obs = np.ones((ne + na, S), f)
    for i in range(ne + na):
        obs[i, rng.choice(S, size=3, replace=False)] = 1 + 2 * rng.choice([-1, 1, 2], size=3)
    obs[:, S - 1] = 3
    return w, obs[:ne], obs[ne:]


def check_disc_indexing(be, net, ne, na):
    w, expert, agent = integer_disc_case(net, ne, na)
    gp, lr = float(ne), 0.25
    pol = Policy(w, lib_path=be.lib)
    ref = tr.reference_disc_grad(w, expert, agent, gp, lr)
    # the precondition: every stage value is an integer below 256 (exact in bf16); the least-squares dz stages are such integers over 2 n_side, exact where n_side is a
    # power of two (|e| < 256, so 0.5 e / n_side is a bf16 value and every sum of them an fp32 one)
    small_int = lambda v: (v == np.round(v)).all() and np.abs(v).max() < 256
    for k in ("h1", "h2", "z3", "gx"):
        assert small_int(ref[k]), k
    for k in ("g2", "g1", "a", "t1", "t2"):
        assert small_int(tr.bf16_value(ref[k])), k
    assert (ref["sq"] == np.round(ref["sq"])).all() and np.abs(ref["sq"]).max() < 2 ** 24
    exact_division = (ne & (ne - 1)) == 0 and (na & (na - 1)) == 0
    if exact_division:
        for k in ("dz3", "dz2", "dz1"):
            assert small_int(tr.bf16_value(ref[k]) * (2 * max(ne, na))), k
    got = run_disc(be, pol, net, tr.pack_params(w), expert, agent, gp, lr)
    S = net["S"]
    # the stages ahead of the division by n_side (and the whole penalty path: grad_penalty / n_e = 1) are exact for every (n_e, n_a)
    for k in ("s16", "h1", "h2"):
        assert np.array_equal(got[k][:, :ref[k].shape[1]], ref[k]) and not got[k][:, ref[k].shape[1]:].any(), k
    assert np.array_equal(got["z3"][:, :1], ref["z3"]) and not got["z3"][:, 1:].any()
    assert np.array_equal(got["logits"], ref["logits"]) and np.array_equal(got["dz3"], ref["dz3"])
    for k in PEN_STAGES:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["stats"][NOT_SIG], ref["stats"][NOT_SIG]), (got["stats"], ref["stats"])
    assert abs(got["stats"][SIG] - ref["stats"][SIG]) <= 1e-13 * abs(ref["stats"][SIG])
    assert ref["stats"][5] > 0 and ref["sq"].any()
    if exact_division:
        for k in ("dz2", "dz1"):
            assert np.array_equal(got[k], ref[k]), k
        assert np.array_equal(got["grads"], ref["grads"])
    else:
        check_disc_stages(got, w, expert, agent, gp, lr, forward=False)


@pytest.mark.parametrize("ne,na", PAIRS)
@pytest.mark.parametrize("net", [NET_A, NET_B], ids=["A", "B"])
def test_indexing_bit_for_bit(emu_lib, net, ne, na):
    check_disc_indexing(Emu(emu_lib), net, ne, na)


@pytest.mark.gpu
@pytest.mark.parametrize("ne,na", PAIRS)
@pytest.mark.parametrize("net", [NET_A, NET_B], ids=["A", "B"])
def test_indexing_bit_for_bit_gpu(hip_lib, net, ne, na):
    check_disc_indexing(Gpu(hip_lib), net, ne, na)


# ---------------------------------------------------------------- 2. random inputs, stage by stage

def check_disc_random(be, net, ne, na):
    w = disc_weights(net, seed=ne + 2)
    expert, agent = random_obs(net, ne, na)
    pol = Policy(w, lib_path=be.lib)
    got = run_disc(be, pol, net, tr.pack_params(w), expert, agent, 10.0, 0.05)
    check_disc_stages(got, w, expert, agent, 10.0, 0.05)
    assert got["stats"][5] > 0 and got["sq"].any()


RANDOM_CASES = [(NET_A, 1, 1), (NET_A, 17, 15), (NET_A, 130, 1), (NET_B, 15, 17), (NET_B, 16, 16), (NET_B, 33, 65), (NET_B, 65, 33), (NET_REF, 33, 31)]
RANDOM_IDS = ["A-1-1", "A-17-15", "A-130-1", "B-15-17", "B-16-16", "B-33-65", "B-65-33", "ref-33-31"]


@pytest.mark.parametrize("net,ne,na", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage(emu_lib, net, ne, na):
    check_disc_random(Emu(emu_lib), net, ne, na)


@pytest.mark.gpu
@pytest.mark.parametrize("net,ne,na", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_inputs_stage_by_stage_gpu(hip_lib, net, ne, na):
    check_disc_random(Gpu(hip_lib), net, ne, na)


# ---------------------------------------------------------------- 3. against float64 autograd of the reference's loss on the unrounded masters

def torch_disc_reference(w, expert, agent, gp, lr):
    """the reference's loss (learning/amp_agent.py:134-207, 251-257) in float64 on the fp32 masters, the penalty by autograd.grad(create_graph=True) with respect to the
    normalised expert input: ({key: gradient}, the penalty statistic)"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    p = {k: t(w[k]).requires_grad_(True) for k in tr.KEYS}
    net = lambda x: (torch.relu(torch.relu(x @ p["w1"] + p["b1"]) @ p["w2"] + p["b2"]) @ p["w3"] + p["b3"])[:, 0]
    norm = lambda o: (t(o) - t(w["s_mean"])) * t(np.float32(1) / w["s_std"])
    xe = norm(expert).requires_grad_(True)
    ye, ya = net(xe), net(norm(agent))
    loss = 0.5 * ((0.5 * (ye - 1) ** 2).mean() + (0.5 * (ya + 1) ** 2).mean())
    gx, = torch.autograd.grad(ye.sum(), xe, create_graph=True)
    penalty = 0.5 * (gx ** 2).sum(dim=1).mean()
    loss = loss + gp * penalty + lr * 0.5 * (p["w3"] ** 2).sum()
    loss.backward()
    return {k: p[k].grad.numpy() for k in tr.KEYS}, float(penalty.detach())


# relative error ||g - g64|| / ||g64|| of each gradient block and of the penalty statistic against float64 autograd on the unrounded net, NET_B at (16, 16); bounds one
# notch (the next of 1, 2, 5 x 10^k) above the measurement on the emulator (the convention of tests/test_train.py).  Measured:
#   gp 10, lr 0.05   w1 2.8e-2  b1 4.3e-2  w2 1.9e-2  b2 2.7e-2  w3 9.5e-3  b3 8.9e-3  penalty 8.3e-4
#   gp 0, lr 0       w1 3.9e-2  b1 4.3e-2  w2 2.3e-2  b2 2.7e-2  w3 6.0e-3  b3 8.9e-3  (no penalty: the statistic is exactly 0)
# As in tests/test_train.py most of it is the bf16 rounding of the weights, which moves pre-activations across zero.
UNROUNDED = {"on": (10.0, 0.05, dict(w1=5e-2, b1=5e-2, w2=2e-2, b2=5e-2, w3=1e-2, b3=1e-2, penalty=1e-3)),
             "off": (0.0, 0.0, dict(w1=5e-2, b1=5e-2, w2=5e-2, b2=5e-2, w3=1e-2, b3=1e-2, penalty=0.0))}


def check_disc_unrounded(be, name):
    gp, lr, bounds = UNROUNDED[name]
    net, ne, na = NET_B, 16, 16
    w = disc_weights(net, seed=4)
    expert, agent = random_obs(net, ne, na, seed=3)
    flat = tr.pack_params(w)
    pol = Policy(w, lib_path=be.lib)
    got = run_disc(be, pol, net, flat, expert, agent, gp, lr)
    ref, ref_pen = torch_disc_reference(w, expert, agent, gp, lr)
    mine = blocks(net, 1, got["grads"])
    err = {k: float(np.linalg.norm(mine[k] - ref[k]) / np.linalg.norm(ref[k])) for k in tr.KEYS}
    err["penalty"] = abs(got["stats"][5] - ref_pen) / ref_pen if gp > 0 else 0.0
    print("unrounded disc %s: " % name + "  ".join("%s %.2g" % (k, v) for k, v in err.items()))
    for k, v in err.items():
        assert v <= bounds[k], (k, v, bounds[k])
    if gp == 0 and lr == 0:
        # n_e = n_a: 0.5 / n_side = 1 / n, so the call is dm_train_value_grad on the concatenated rows with targets +-1, bit for bit
        from test_train import run_grad
        val = run_grad(be, Policy(w, lib_path=be.lib), net, flat, "critic", np.concatenate([expert, agent]), targets=np.concatenate([np.ones(ne), -np.ones(na)]))
        assert got["grads"].tobytes() == val["grads"].tobytes()
        for k in LS_STAGES:
            assert np.array_equal(got[k], val[k]), k
        assert np.array_equal(got["logits"], val["out"]) and got["stats"][5] == 0.0
        assert abs(got["stats"][0] - val["stats"][0]) <= 1e-13 * val["stats"][0]          # 0.5 (0.5 sum_e / 16 + 0.5 sum_a / 16) = 0.5 sum / 32, in another order


@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_float64_autograd(emu_lib, name):
    check_disc_unrounded(Emu(emu_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNROUNDED))
def test_against_float64_autograd_gpu(hip_lib, name):
    check_disc_unrounded(Gpu(hip_lib), name)


# ---------------------------------------------------------------- 4. term isolation

def check_term_isolation(be):
    net, ne, na = NET_A, 17, 15
    w = disc_weights(net, seed=6)
    # an expert row whose h2 is all zero: biases <= 0 and row 3 at the normaliser's mean (x = 0, so h1 = relu(b1) = 0 and h2 = relu(b2) = 0)
    w["b1"] = -np.abs(w["b1"]); w["b2"] = -np.abs(w["b2"])
    expert, agent = random_obs(net, ne, na, seed=1)
    expert[3] = w["s_mean"]
    flat = tr.pack_params(w)
    run = lambda gp, lr: run_disc(be, Policy(w, lib_path=be.lib), net, flat, expert, agent, gp, lr)
    both, reg_only, pen_only, none = run(10.0, 0.05), run(0.0, 0.05), run(10.0, 0.0), run(0.0, 0.0)
    g = {k: blocks(net, 1, v["grads"]) for k, v in dict(both=both, reg_only=reg_only, pen_only=pen_only, none=none).items()}
    # grad_penalty = 0: no penalty statistic, the least-squares part of the penalty-on call (its dz stages, its b gradients, and w1 / w2 without the penalty's add)
    assert reg_only["stats"][5] == 0.0 and none["stats"][5] == 0.0 and both["stats"][5] > 0
    for k in LS_STAGES:
        assert np.array_equal(both[k], reg_only[k]) and np.array_equal(both[k], none[k]), k
    for k in (0, 1, 2, 3, 4, 6, 7):
        assert both["stats"][k] == reg_only["stats"][k] == pen_only["stats"][k] == none["stats"][k]
    # the penalty leaves the bias gradients bit-identical
    for k in ("b1", "b2", "b3"):
        assert g["both"][k].tobytes() == g["reg_only"][k].tobytes() == g["pen_only"][k].tobytes() == g["none"][k].tobytes(), k
    for k in ("w1", "w2"):
        assert g["reg_only"][k].tobytes() == g["none"][k].tobytes() and not np.array_equal(g["both"][k], g["none"][k]), k
    # logit_reg changes the w3 block alone
    for k in ("w1", "b1", "w2", "b2", "b3"):
        assert g["both"][k].tobytes() == g["pen_only"][k].tobytes(), k
    assert not np.array_equal(g["both"]["w3"], g["pen_only"]["w3"]) and not np.array_equal(g["reg_only"]["w3"], g["none"]["w3"])
    w3 = np.asarray(w["w3"], np.float32).reshape(-1, 1)
    assert np.array_equal(g["both"]["w3"], tr.fma32(np.float32(0.05), w3, g["pen_only"]["w3"]))
    assert np.array_equal(g["reg_only"]["w3"], tr.fma32(np.float32(0.05), w3, g["none"]["w3"]))
    for k in PEN_STAGES:
        assert np.array_equal(both[k], pen_only[k]), k
    # the dead expert row: nothing in any penalty stage, and the statistic is the other rows' alone
    assert not both["h2"][3].any() and both["h2"][:ne].any(axis=1).sum() == ne - 1
    for k in PEN_STAGES:
        assert not both[k][3].any(), k
    others = np.delete(both["sq"], 3, axis=0).astype(np.float64)
    assert abs(both["stats"][5] - 0.5 * others.sum() / ne) <= 1e-13 * both["stats"][5]
    check_disc_stages(both, w, expert, agent, 10.0, 0.05)
    check_disc_stages(reg_only, w, expert, agent, 0.0, 0.05)


def test_term_isolation(emu_lib):
    check_term_isolation(Emu(emu_lib))


@pytest.mark.gpu
def test_term_isolation_gpu(hip_lib):
    check_term_isolation(Gpu(hip_lib))


# ---------------------------------------------------------------- 5. determinism

def check_disc_determinism(be, net, ne, na):
    w = disc_weights(net, seed=8)
    expert, agent = random_obs(net, ne, na, seed=2)
    flat = tr.pack_params(w)
    runs = []
    for _ in range(2):
        got = run_disc(be, Policy(w, lib_path=be.lib), net, flat, expert, agent, 10.0, 0.05)
        runs.append((got["grads"].tobytes(), got["stats"].tobytes(), got["ws_bytes"], got["logits"].tobytes()))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("net,ne,na", [(NET_B, 65, 33), (NET_REF, 33, 31)], ids=["B-65-33", "ref-33-31"])
def test_determinism(emu_lib, net, ne, na):
    check_disc_determinism(Emu(emu_lib), net, ne, na)


@pytest.mark.gpu
@pytest.mark.parametrize("net,ne,na", [(NET_B, 65, 33), (NET_REF, 33, 31)], ids=["B-65-33", "ref-33-31"])
def test_determinism_gpu(hip_lib, net, ne, na):
    check_disc_determinism(Gpu(hip_lib), net, ne, na)


# ---------------------------------------------------------------- 6. it trains

def check_disc_trains(be):
    """Two separable Gaussian clusters (expert around +c, agent around -c, c a fixed direction), 40 grad + step calls through DiscTrainer on the context of a
    heads.Discriminator with weight decay, penalty and regulariser on: both accuracies end above 0.9 and the penalty statistic stays finite.  Afterwards the
    discriminator's own evaluation returns exactly the logits a fresh grad call reports: the net that scores IS the net that was trained."""
    import torch
    net, n, steps = NET_A, 64, 40
    S = net["S"]
    w = net_weights(net, seed=11, A=1, normalisers=False)
    rng = np.random.default_rng(21)
    c = rng.standard_normal(S).astype(np.float32); c *= 2.0 / np.linalg.norm(c)
    expert = (c + 0.3 * rng.standard_normal((n, S))).astype(np.float32); agent = (-c + 0.3 * rng.standard_normal((n, S))).astype(np.float32)
    disc = heads.Discriminator(w, lib_path=be.lib)
    dev = torch.device(be.device())
    trn = tr.DiscTrainer.from_policy(disc.net, w, stepsize=0.01, momentum=0.9, weight_decay=1e-4, device=dev)
    d_e, d_a = torch.from_numpy(expert).to(dev), torch.from_numpy(agent).to(dev)
    hist = []
    for _ in range(steps):
        trn.grad(d_e, d_a, grad_penalty=10.0, logit_reg=0.05)
        hist.append(trn.stats().cpu().numpy().copy())
        trn.step()
    logits = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    trn.grad(d_e, d_a, grad_penalty=10.0, logit_reg=0.05, logits_out=logits)
    last = trn.stats().cpu().numpy()
    hist = np.array(hist)
    print("disc training: acc_expert %.3f -> %.3f, acc_agent %.3f -> %.3f, penalty %.3g -> %.3g, loss %.4g" % (hist[0, 1], last[1], hist[0, 2], last[2], hist[0, 5], last[5],
                                                                                                               float(trn.loss().cpu())))
    assert last[1] > 0.9 and last[2] > 0.9 and np.isfinite(hist[:, 5]).all() and np.isfinite(last).all()
    assert float(trn.loss().cpu()) == last[0] + 1e-4 * last[7] + 0.05 * last[6] + 10.0 * last[5]
    both = np.concatenate([expert, agent])
    logits_of = lambda d: d.eval_torch(torch.from_numpy(both).to(dev), raw=True)[1].cpu().numpy() if be.gpu else d.eval_host(both)[1]
    y = logits_of(disc)
    assert np.array_equal(y, logits.cpu().numpy())
    assert not np.array_equal(y, logits_of(heads.Discriminator(w, lib_path=be.lib)))


def test_it_trains(emu_lib):
    check_disc_trains(Emu(emu_lib))


@pytest.mark.gpu
def test_it_trains_gpu(hip_lib):
    check_disc_trains(Gpu(hip_lib))


# ---------------------------------------------------------------- 7. refusals

def check_disc_refusals(be):
    """every refusal of include/dm_hip.h by name, nothing written: the outputs keep their sentinels"""
    net, ne, na = NET_A, 4, 3
    S = net["S"]
    disc = Policy(net_weights(net, seed=3, A=1), lib_path=be.lib)
    actor = Policy(net_weights(net, seed=3, A=3), lib_path=be.lib)
    gated = Policy(random_weights(S, 1, H1=64, H2=64, seed=1, gated_goal_dim=3, gate_common=32, gate_hidden=32), lib_path=be.lib)
    P = tr.param_count(disc)
    nb = tr.disc_workspace_bytes(disc, ne, na)
    f = lambda *shape: be.put(np.zeros(shape, np.float32))
    params, expert, agent = f(P), f(ne, S), f(na, S)
    grads, logits = be.put(np.full(P, -77.0, np.float32)), be.put(np.full(ne + na, -77.0, np.float32))
    stats, ws = be.put(np.full(8, -77.0)), be.put(np.full(nb // 8 + 2, -77.0))
    p = be.ptr
    def call(pol=disc, params_=params, expert_=expert, agent_=agent, ne_=ne, na_=na, grads_=grads, stats_=None, ws_=None, nb_=nb, gp=10.0, lr=0.05):
        ptr = lambda t: p(t) if t is not None else 0
        tr.disc_grad_device(pol, ptr(params_), ptr(expert_), ne_, ptr(agent_), na_, ptr(grads_), p(stats) if stats_ is None else stats_, p(ws) if ws_ is None else ws_, nb_,
                            gp, lr, logits_ptr=p(logits), stream=be.stream)
    big = 20_000_000
    cases = [("gated context", lambda: call(pol=gated)), ("a net with one output", lambda: call(pol=actor)),
             ("n_expert and n_agent must be >= 1", lambda: call(ne_=0)), ("n_expert and n_agent must be >= 1", lambda: call(na_=0)),
             ("n_expert and n_agent must be >= 1", lambda: call(na_=-2)),
             ("grad_penalty must be finite and >= 0", lambda: call(gp=-1.0)), ("grad_penalty must be finite and >= 0", lambda: call(gp=float("inf"))),
             ("grad_penalty must be finite and >= 0", lambda: call(gp=float("nan"))),
             ("logit_reg must be finite and >= 0", lambda: call(lr=-0.05)), ("logit_reg must be finite and >= 0", lambda: call(lr=float("nan"))),
             ("null argument", lambda: call(params_=None)), ("null argument", lambda: call(expert_=None)), ("null argument", lambda: call(agent_=None)),
             ("null argument", lambda: call(grads_=None)), ("null argument", lambda: call(stats_=0)), ("null argument", lambda: call(ws_=0)),
             ("workspace too small", lambda: call(nb_=nb - 1)), ("workspace too small", lambda: call(nb_=tr.workspace_bytes(disc, ne + na))),
             ("16-byte", lambda: call(ws_=p(ws) + 8)), ("8-byte aligned", lambda: call(stats_=p(stats) + 4)),
             ("too many rows", lambda: call(ne_=big, na_=big)), ("too many rows", lambda: call(ne_=2 ** 31 - 1, na_=2 ** 31 - 1))]
    for what, fn in cases:
        with pytest.raises(RuntimeError, match=what):
            fn()
    for what, fn in [("gated context", lambda: tr.disc_workspace_bytes(gated, 4, 4)), ("a net with one output", lambda: tr.disc_workspace_bytes(actor, 4, 4)),
                     ("must be >= 1", lambda: tr.disc_workspace_bytes(disc, 0, 4)), ("too many rows", lambda: tr.disc_workspace_bytes(disc, big, big))]:
        with pytest.raises(RuntimeError, match=what):
            fn()
    for name, t in dict(grads=grads, logits=logits, stats=stats, ws=ws).items():
        assert (be.get(t) == -77).all(), name
    assert not be.get(params).any()


def test_refusals(emu_lib):
    check_disc_refusals(Emu(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    check_disc_refusals(Gpu(hip_lib))


# ---------------------------------------------------------------- 8. the collective takes the trainer

def test_all_reduce_accepts_the_trainer(emu_lib, tmp_path):
    """dist.all_reduce_gradients on a DiscTrainer as on the other trainers: a group of one rank (gloo) sums the gradient view in place and leaves its bytes"""
    import torch
    import torch.distributed as td
    from deepmimic_amd.dist import all_reduce_gradients
    net = NET_A
    w = disc_weights(net, seed=5)
    expert, agent = random_obs(net, 5, 7)
    disc = heads.Discriminator(w, lib_path=emu_lib)
    trn = tr.DiscTrainer.from_policy(disc.net, w, stepsize=0.01, device="cpu")
    trn.grad(torch.from_numpy(expert), torch.from_numpy(agent))
    before = trn.grads.clone()
    created = not td.is_initialized()
    if created:
        td.init_process_group("gloo", store=td.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        out = all_reduce_gradients(trn)
    finally:
        if created:
            td.destroy_process_group()
    assert out is trn.grads and torch.equal(out, before) and bool(before.any())
    trn.step(grad_scale=1.0)
    assert trn.STATS == tr.DISC_STATS and float(trn.stat("grad_penalty")) == float(trn.stats()[5]) > 0
