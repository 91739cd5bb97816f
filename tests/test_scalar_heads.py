"""The scalar heads of the device nets (include/dm_hip.h dm_policy_eval_scalar, deepmimic_amd/heads.py; kernels: the HEAD = 1 instantiations of
k_policy_fused and k_policy_layer<2, ..> in deepmimic_amd/csrc/dm_policy.h): critic value and AMP style reward in the launch that evaluates the net.

Every check runs on the emulator and, under `-m gpu`, on the device through raw device pointers, with the fixtures and helpers of test_policy_kernels.py.

(1) exact, every route: the integer networks of test_policy_kernels.py / test_policy_gated.py (exact in bf16, sums exact in fp32) with an output layer in
    multiples of 1/8 that reads four hidden units bounded by the observation clip, so that y lies on the 1/8 grid in [-1, 3]: raw output, value head and
    style head (scale 2, lerp 0.5, task rewards in multiples of 1/64: every operation exact in fp32) equal the float64 reference BIT FOR BIT;
(2) the raw output equals, bit for bit, the mode action of an actor (Policy, A = 1, identity action normaliser) on random weights at 1024 / 512;
(3) terminate override, clip bounds, NaN rows, row_mask with fill, and sentinels on both sides of the outputs;
(4) the style head's general arithmetic within its rounding bound;
(5) random weights against the numpy reference with the bounds of test_policy.py::test_policy_gpu_matches_reference;
(6) set_weights on a scalar context == a fresh context, bit for bit;
(8) closed loop on the GPU: TorchVecEnv(amp_heading_zombie) -> style reward -> critic (terminal observations under row_mask = done) -> TD(lambda).
"""
import numpy as np
import pytest

from deepmimic_amd import heads
from deepmimic_amd.heads import Critic, Discriminator
from deepmimic_amd.policy import GATE_KEYS, Policy, random_weights
from test_policy_kernels import (FUSED_8_2, FUSED_12_2, LAYERED, S_CLIP, TILE64_TILE64, WAVE_WAVE, Row, actor_f64, check_reference, integer_inputs, integer_net,
                                 set_env, split, xavier_net)
from test_policy_gated import GRow, check_gated_reference, gated_actor_f64, integer_gated_net

# (S, G) as the issue lists them; A = 1 throughout: N3 = 32, so the one-launch ids are FUSED_8_2 / FUSED_12_2
SCALAR_ROWS = {
    "s197": Row(197, 0, 1, FUSED_8_2, 256, 32, note="fused, K1 = 256"),
    "s227_g7": Row(227, 7, 1, FUSED_8_2, 256, 32, note="fused, K1 = 256, goal block"),
    "s300_g50": Row(300, 50, 1, FUSED_12_2, 384, 32, note="fused, K1 = 384, the goal split across the column passes"),
    "s400": Row(400, 0, 1, TILE64_TILE64, 448, 32, note="not compiled as one launch: per layer"),
    "h64": Row(40, 6, 1, WAVE_WAVE, 64, 32, H1=64, H2=64, note="the one-wave route"),
    "layered": Row(227, 7, 1, TILE64_TILE64, 256, 32, env=(LAYERED,), note="DM_POLICY_LAYERED=1"),
}
GATED_ROWS = {n: GRow(r.S, r.G, 1, r.path, r.K1, r.N3, H1=r.H1, H2=r.H2, env=r.env) for n, r in SCALAR_ROWS.items() if r.G}
ROWS_EMU = (1, 31, 32, 33, 200)
ROWS_GPU = ROWS_EMU + (4097,)
PAD, SENT = 64, np.float32(-12345.5)
PLAIN_NET_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3", "s_mean", "s_std")


# ---------------------------------------------------------------------------------------------------------------------------------- running a call
class Run:
    """one head on one library; the outputs carry PAD sentinel rows IN FRONT OF row 0 and BEHIND row n, which must survive"""

    def __init__(self, head, gpu):
        self.head, self.gpu = head, gpu

    def __call__(self, s, g=None, raw=True, **rows):
        n = s.shape[0]
        out = np.full(n + 2 * PAD, SENT, np.float32); y = np.full(n + 2 * PAD, SENT, np.float32)
        arrs = dict(s=np.ascontiguousarray(s, np.float32), out=out, y=y)
        if g is not None:
            arrs["g"] = np.ascontiguousarray(g, np.float32)
        for k, v in rows.items():
            if k != "fill" and v is not None:
                arrs[k] = np.ascontiguousarray(v, np.float32 if k == "task_reward" else np.int32)
        if self.gpu:
            import torch
            dev = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
            torch.cuda.synchronize()
            ptr = lambda k: dev[k].data_ptr() if k in dev else 0
        else:
            dev = arrs
            ptr = lambda k: dev[k].ctypes.data if k in dev else 0
        kw = {k + "_ptr": ptr(k) for k in ("terminate", "task_reward") if k in rows}
        self.head.eval_device(ptr("s"), n, ptr("out") + 4 * PAD, ptr("g"), 0 if g is None else g.shape[1], (ptr("y") + 4 * PAD) if raw else 0, ptr("row_mask"),
                              rows.get("fill", 0.0), 0, **kw)
        if self.gpu:
            torch.cuda.synchronize()
            out, y = dev["out"].cpu().numpy(), dev["y"].cpu().numpy()
        for a in (out, y):
            assert (a[:PAD] == SENT).all() and (a[PAD + n:] == SENT).all(), "rows outside [0, n) were written"
        if not raw:
            assert (y == SENT).all()
        assert not (out[PAD:PAD + n] == SENT).any(), "an output row of [0, n) was not written"
        return out[PAD:PAD + n], y[PAD:PAD + n]

    def close(self):
        self.head.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------- (1) the integer network
def scalar_integer_net(row, gated, inst, seed):
    """The integer network of the actor tests with a one-column output layer on the 1/8 grid.  Four hidden units of each layer are re-wired into chains
    input column k -> h1 unit i -> h2 unit j (weights +1, biases 0; gated: sigma = 1 and beta = 0 for them), so h2_j = relu(x_k) lies in [0, 6] by the
    observation clip; w3 = (+1, -1, +1, -1) / 8 on the four h2 units (random positions: other k-steps and lanes per case), 0 elsewhere, b3 = 1:
    y = 1 + (h2_a - h2_b + h2_c - h2_d) / 8 lies in [-0.5, 2.5].  The other hidden units keep the actor tests' weights, so the preconditions there hold."""
    w = integer_gated_net(row, seed) if gated else integer_net(row, inst, seed)
    rng = np.random.default_rng(seed + 17)
    S, H1, H2 = row.S, row.H1, row.H2
    ks = rng.choice(S, 4, replace=False); i1 = rng.choice(H1, 4, replace=False); j2 = rng.choice(H2, 4, replace=False)
    w["w1"][:, i1] = 0; w["w1"][ks, i1] = 1; w["b1"][i1] = 0
    w["w2"][:, j2] = 0; w["w2"][i1, j2] = 1; w["b2"][j2] = 0
    if gated:
        for i, idx in ((0, i1), (1, j2)):
            for k in ("g%d_bias_w", "g%d_scale_w"):
                w[k % i][:, idx] = 0
            w["g%d_bias_b" % i][idx] = 0; w["g%d_scale_b" % i][idx] = 0          # beta = 0, sigma = 2 sigmoid(0) = 1 exactly
    w3 = np.zeros((H2, 1), np.float32); w3[j2, 0] = np.array([1, -1, 1, -1], np.float32) / 8
    w["w3"] = w3; w["b3"] = np.array([1.0], np.float32)
    for k in ("a_mean", "a_std", "logstd"):
        w.pop(k, None)
    return w


def check_scalar_reference(ref, y, r, scale, tag):
    """preconditions of the exact check, on the float64 reference alone"""
    assert np.array_equal(8 * y, np.rint(8 * y)) and y.min() >= -1 and y.max() <= 3, (tag, y.min(), y.max())
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64)) and np.array_equal(r, r.astype(np.float32).astype(np.float64)), tag
    if y.size >= 31:
        assert ((r > 0) & (r < scale)).mean() >= 0.25, (tag, ((r > 0) & (r < scale)).mean())      # a head that always returns 0 (or scale) does not pass
        assert np.unique(y).size >= 3, tag


def check_exact(name, gated, lib, gpu, monkeypatch, counts):
    row = (GATED_ROWS if gated else SCALAR_ROWS)[name]
    set_env(monkeypatch, row.env)
    for inst in (("w2",) if gated else ("w2", "w1")):
        w = scalar_integer_net(row, gated, inst, seed=sum(map(ord, name)) + (1 if gated else 0))
        crit = Run(Critic(w, lo=-0.25, hi=2.0, lib_path=lib, s_clip=S_CLIP), gpu)
        free = Run(Critic(w, lib_path=lib, s_clip=S_CLIP), gpu)
        disc = None if gated else Run(Discriminator(w, reward_scale=2.0, task_reward_lerp=0.5, lib_path=lib, s_clip=S_CLIP), gpu)
        assert crit.head.info()["path"] == -1 and crit.head.info()["net"]["gated"] == gated
        for M in counts:
            tag = "%s/%s/%s/M=%d" % (name, "gated" if gated else "plain", inst, M)
            cat = integer_inputs(row, w, M, seed=M)
            wa = dict(w, a_mean=np.zeros(1, np.float32), a_std=np.ones(1, np.float32))
            # the hidden layers' preconditions are the actor tests' own; their integer test of the output is given 8 y (y itself: check_scalar_reference)
            ref = (gated_actor_f64 if gated else actor_f64)(wa, cat, S_CLIP)
            (check_gated_reference if gated else check_reference)(dict(ref, m=8 * ref["m"], a=8 * ref["m"]), tag)
            y = ref["m"][:, 0]
            task = np.random.default_rng(M).integers(0, 65, M) / 64.0
            r = heads.reference_style_reward(y, 2.0, 0.5, task)
            check_scalar_reference(ref, y, r, 2.0, tag)                      # before the kernel is looked at
            s, g = split(row, cat)
            v, raw = free(s, g)
            info = free.head.info()
            assert info["path"] == row.path and info["rows"] == M and info["kind"] == heads.VALUE and not info["masked"], (tag, info)
            assert info["net"]["path"] == -1                                # dm_policy_info reports forward calls only
            assert same_bits(raw, y), (tag, np.abs(raw - y).max())
            assert same_bits(v, y), tag
            v, raw = crit(s, g)
            assert same_bits(v, heads.reference_value(y, -0.25, 2.0)) and same_bits(raw, y), tag
            if disc is not None:
                rr, raw = disc(s, g, task_reward=task)
                assert disc.head.info()["kind"] == heads.STYLE
                assert same_bits(raw, y) and same_bits(rr, r), (tag, np.abs(rr - r).max())
                rr, _ = disc(s, g, raw=False)
                assert same_bits(rr, heads.reference_style_reward(y, 2.0)), tag
        for x in (crit, free, disc):
            if x is not None:
                x.close()


@pytest.mark.parametrize("name", sorted(SCALAR_ROWS))
def test_exact_every_route_emulator(emu_lib, monkeypatch, name):
    check_exact(name, False, emu_lib, False, monkeypatch, ROWS_EMU)


@pytest.mark.parametrize("name", sorted(GATED_ROWS))
def test_exact_every_route_gated_emulator(emu_lib, monkeypatch, name):
    check_exact(name, True, emu_lib, False, monkeypatch, ROWS_EMU)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCALAR_ROWS))
def test_exact_every_route_gpu(hip_lib, monkeypatch, name):
    check_exact(name, False, hip_lib, True, monkeypatch, ROWS_GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GATED_ROWS))
def test_exact_every_route_gated_gpu(hip_lib, monkeypatch, name):
    check_exact(name, True, hip_lib, True, monkeypatch, ROWS_GPU)


# ---------------------------------------------------------------------------------------------------------------------------------- (2) the actor's layer 3
def random_scalar_net(S, G=0, seed=1, H1=1024, H2=512, scale=0.2):
    """Xavier weights, non-zero biases, an observation normaliser; the output layer wide enough for y to spread over the heads' interesting range"""
    w = random_weights(S, 1, H1, H2, seed=seed, init_output_scale=scale, gated_goal_dim=G)
    x = xavier_net(S, 1, H1, H2, seed=seed)
    for k in ("b1", "b2", "s_mean", "s_std"):
        w[k] = x[k]
    w["b3"] = np.array([0.4], np.float32)
    for k in ("a_mean", "a_std", "logstd"):
        w.pop(k, None)
    return w


def check_equals_actor(lib, gpu, monkeypatch, gated, layered, M):
    S, G = 227, 7
    set_env(monkeypatch, (LAYERED,) if layered else ())
    w = random_scalar_net(S, G if gated else 0)
    x = (1.5 * np.random.default_rng(4).normal(size=(M, S))).astype(np.float32)
    run = Run(Critic(w, lib_path=lib, s_clip=5.0), gpu)
    _, raw = run(x)
    assert run.head.info()["path"] == (TILE64_TILE64 if layered else FUSED_8_2)
    run.close()
    from test_policy_kernels import Runner
    actor = Runner(dict(w, logstd=np.zeros(1, np.float32)), lib, gpu, s_clip=5.0)
    a, _, _ = actor(x)
    assert actor.pol.info()["path"] == (TILE64_TILE64 if layered else FUSED_8_2)
    actor.close()
    assert a.std() > 0.05 and same_bits(raw, a[:, 0]), np.abs(raw - a[:, 0]).max()


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("layered", [False, True])
def test_raw_output_is_the_actors_mode_action_emulator(emu_lib, monkeypatch, gated, layered):
    check_equals_actor(emu_lib, False, monkeypatch, gated, layered, 45)


@pytest.mark.gpu
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("layered", [False, True])
def test_raw_output_is_the_actors_mode_action_gpu(hip_lib, monkeypatch, gated, layered):
    check_equals_actor(hip_lib, True, monkeypatch, gated, layered, 333)


# ---------------------------------------------------------------------------------------------------------------------------------- (3) end-of-path rules, mask
def check_rules_and_mask(lib, gpu, monkeypatch, layered):
    S, M = 197, 100
    set_env(monkeypatch, (LAYERED,) if layered else ())
    w = random_scalar_net(S)
    rng = np.random.default_rng(8)
    x = (1.5 * rng.normal(size=(M, S))).astype(np.float32)
    free = Run(Critic(w, lib_path=lib), gpu)
    v0, y0 = free(x)
    assert same_bits(v0, y0) and y0.std() > 0.05                                     # infinite bounds do not clip
    # terminate 0 / 1 / 2 -> v, val_fail, val_succ exactly; finite bounds clip
    lo, hi = np.float32(np.quantile(y0, 0.3)), np.float32(np.quantile(y0, 0.7))
    term = rng.integers(0, 3, M).astype(np.int32)
    crit = Run(Critic(w, lo=float(lo), hi=float(hi), val_fail=-3.5, val_succ=41.25, lib_path=lib), gpu)
    v, y = crit(x, terminate=term)
    assert same_bits(y, y0)
    want = np.where(term == 1, np.float32(-3.5), np.where(term == 2, np.float32(41.25), np.minimum(np.maximum(y0, lo), hi)))
    assert same_bits(v, want) and (y0 < lo).any() and (y0 > hi).any() and {0, 1, 2} <= set(term)
    assert same_bits(v, heads.reference_value(y0, lo, hi, term, -3.5, 41.25))
    v, _ = crit(x)
    assert same_bits(v, np.minimum(np.maximum(y0, lo), hi))
    # a NaN observation row (no observation clip: the row's own value is unspecified) does not leak into a neighbour
    xn = x.copy(); xn[5, 3] = np.nan; xn[40, S - 1] = np.nan
    vn, yn = free(xn)
    keep = np.setdiff1d(np.arange(M), [5, 40])
    assert same_bits(vn[keep], v0[keep]) and same_bits(yn[keep], y0[keep])
    # row_mask: tile 1 (rows 32 .. 63) all off -> fill in both outputs; mixed tiles compute their rows bit-equal to the unmasked call
    mask = (rng.random(M) < 0.5).astype(np.int32); mask[32:64] = 0; mask[0] = 1; mask[M - 1] = 0; mask[64:80] = 0
    fill = np.float32(-77.5)
    vm, ym = crit(x, terminate=term, row_mask=mask, fill=float(fill))
    assert crit.head.info()["masked"]
    on = mask != 0
    assert same_bits(vm[on], want[on]) and same_bits(ym[on], y0[on])
    assert (vm[~on] == fill).all() and (ym[~on] == fill).all()
    assert same_bits(vm, heads.reference_value(y0, lo, hi, term, -3.5, 41.25, mask, fill))
    # everything off, and one single row on
    vm, ym = crit(x, row_mask=np.zeros(M, np.int32), fill=float(fill))
    assert (vm == fill).all() and (ym == fill).all()
    one = np.zeros(M, np.int32); one[M - 1] = 1
    vm, ym = crit(x, row_mask=one, fill=0.0)
    assert vm[M - 1] == np.minimum(np.maximum(y0, lo), hi)[M - 1] and ym[M - 1] == y0[M - 1] and not vm[:M - 1].any() and not ym[:M - 1].any()
    # the style head under a mask
    disc = Run(Discriminator(w, reward_scale=2.0, lib_path=lib), gpu)
    r0, _ = disc(x)
    rm, ym = disc(x, row_mask=mask, fill=float(fill))
    assert same_bits(rm[on], r0[on]) and (rm[~on] == fill).all() and same_bits(ym[on], y0[on])
    for r in (free, crit, disc):
        r.close()


@pytest.mark.parametrize("layered", [False, True])
def test_end_of_path_rules_and_row_mask_emulator(emu_lib, monkeypatch, layered):
    check_rules_and_mask(emu_lib, False, monkeypatch, layered)


@pytest.mark.gpu
@pytest.mark.parametrize("layered", [False, True])
def test_end_of_path_rules_and_row_mask_gpu(hip_lib, monkeypatch, layered):
    check_rules_and_mask(hip_lib, True, monkeypatch, layered)


def test_refusals(emu_lib):
    w = random_weights(45, 3, 64, 64, seed=1)
    with pytest.raises(ValueError, match="one output"):
        Critic(w, lib_path=emu_lib)
    # the C-ABI itself refuses a context with action_dim != 1
    import ctypes as C
    pol = Policy(w, lib_path=emu_lib)
    x = np.zeros((4, 45), np.float32); out = np.zeros(4, np.float32)
    head = heads._ScalarHead(heads.VALUE, -np.inf, np.inf, 0, 0, None, 0, 0, None, None, 0)
    pol.lib.dm_policy_eval_scalar.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert pol.lib.dm_policy_eval_scalar(pol.h, x.ctypes.data, None, 0, 4, C.byref(head), out.ctypes.data, None, None) != 0
    assert b"action_dim" in pol.lib.dm_last_error()
    pol.close()
    w1 = random_scalar_net(45, H1=64, H2=64)
    d = Discriminator(w1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="task_reward_lerp"):
        d.eval_host(x, task_reward=np.zeros(4, np.float32))
    d.close()
    c = Critic(w1, lo=1.0, hi=0.0, lib_path=emu_lib)
    with pytest.raises(RuntimeError, match="lo <= hi"):
        c.eval_host(x)
    c.close()
    with pytest.raises(ValueError, match="plain"):
        Discriminator(random_scalar_net(45, 6, H1=64, H2=64), lib_path=emu_lib)


# ---------------------------------------------------------------------------------------------------------------------------------- (4) general arithmetic
def check_style_arithmetic(lib, gpu, M):
    """r = fma(lerp, task, (1 - lerp) * (scale * max(0, fma(-d / 4, d, 1)))) with d = 1 - y has SIX fp32 roundings (d; the fma; the product with scale; 1 - lerp;
    its product with r; the last fma -- d / 4 is exact).  Each is at most 2^-24 relative to its own result.  Where the reward is not clamped |d| < 2, so the
    rounding of d (<= 2^-24 |d|) moves 1 - d^2 / 4 by <= |d| / 2 * 2^-24 |d| <= 2 * 2^-24 and, with the fma's own 2^-24, the scaled and blended term
    (1 - lerp) * scale * (.) = 0.6 (.) by <= 1.8 * 2^-24; the three roundings of the blend's factors add <= 3 * 0.6 * 2^-24 (each relative to a term
    <= 0.6), the last fma 2^-24 |r|: in all below 4.6 * 2^-24 max(1, |r|), inside the bound of 6 roundings x 2^-24 x max(1, |r|) that is asserted.
    The reference is float64 on the device's own raw y, with the float32 values of lerp and scale the call passes."""
    S = 226
    w = random_scalar_net(S, scale=0.3)
    x = (1.5 * np.random.default_rng(12).normal(size=(M, S))).astype(np.float32)
    task = np.random.default_rng(13).random(M).astype(np.float32)
    run = Run(Discriminator(w, reward_scale=2.0, task_reward_lerp=0.7, lib_path=lib), gpu)
    r, y = run(x, task_reward=task)
    run.close()
    want = heads.reference_style_reward(y.astype(np.float64), 2.0, float(np.float32(0.7)), task.astype(np.float64))
    err = np.abs(r.astype(np.float64) - want); bound = 6 * 2.0 ** -24 * np.maximum(1.0, np.abs(want))
    style = heads.reference_style_reward(y.astype(np.float64), 2.0)
    print("STYLE_ARITHMETIC M=%d max err / bound %.3f, rows with 0 < style < scale: %.2f" % (M, (err / bound).max(), ((style > 0) & (style < 2)).mean()))
    assert ((style > 0) & (style < 2)).mean() > 0.25 and (style == 0).any()
    assert (err <= bound).all(), (err / bound).max()


def test_style_reward_arithmetic_emulator(emu_lib):
    check_style_arithmetic(emu_lib, False, 200)


@pytest.mark.gpu
def test_style_reward_arithmetic_gpu(hip_lib):
    check_style_arithmetic(hip_lib, True, 4097)


# ---------------------------------------------------------------------------------------------------------------------------------- (5) random weights
def check_random(lib, gpu, monkeypatch, S, G, gated, M, H1=1024, H2=512):
    """bounds of tests/test_policy.py::test_policy_gpu_matches_reference: 2e-3 of the range against the bf16 statement, 2e-2 against fp32"""
    from test_policy import make
    set_env(monkeypatch, ())
    w = make(S, 1, H1, H2, 11)
    if gated:
        gw = random_weights(S, 1, H1, H2, seed=12, gated_goal_dim=G)
        w.update({k: gw[k] for k in GATE_KEYS + ("goal_dim",)})
    for k in ("a_mean", "a_std", "logstd"):
        w.pop(k, None)
    cat = (np.random.default_rng(2).normal(size=(M, S)) * 1.5 + 0.3).astype(np.float32)
    run = Run(Critic(w, lib_path=lib, s_clip=10.0), gpu)
    s, g = (cat, None) if not G else (cat[:, :S - G], cat[:, S - G:])
    _, y = run(s, g)
    run.close()
    want_bf = heads.reference_forward(w, cat, s_clip=10.0, bf16=True); want_32 = heads.reference_forward(w, cat, s_clip=10.0, bf16=False)
    scale = np.abs(want_32).max()
    assert np.abs(y - want_bf).max() < 2e-3 * scale, (np.abs(y - want_bf).max(), scale)
    assert np.abs(y - want_32).max() < 2e-2 * scale, (np.abs(y - want_32).max(), scale)


def test_random_weights_match_the_numpy_reference_emulator(emu_lib, monkeypatch):
    check_random(emu_lib, False, monkeypatch, 45, 6, True, 37, 64, 128)
    check_random(emu_lib, False, monkeypatch, 226, 0, False, 37)


@pytest.mark.gpu
@pytest.mark.parametrize("S,G,gated", [(197, 0, False), (200, 3, True), (226, 0, False)], ids=["critic", "gated_critic_heading", "discriminator"])
def test_random_weights_match_the_numpy_reference_gpu(hip_lib, monkeypatch, S, G, gated):
    """the humanoid's critic (197), its gated critic in the heading scene (197 + 3) and its AMP discriminator (amp_obs of 226)"""
    for M in (200, 4097):
        check_random(hip_lib, True, monkeypatch, S, G, gated, M)


# ---------------------------------------------------------------------------------------------------------------------------------- (6) weights refresh
def check_refresh(lib, gpu, gated):
    S, G = 200, 3
    old, new = random_scalar_net(S, G if gated else 0, seed=1), random_scalar_net(S, G if gated else 0, seed=2)
    x = (1.5 * np.random.default_rng(4).normal(size=(70, S))).astype(np.float32)
    live = Run(Critic(old, lo=-0.1, hi=0.9, lib_path=lib, s_clip=5.0), gpu)
    v_old, _ = live(x)
    assert set(live.head.weight_shapes()) == set(k for k in new if k != "goal_dim") and live.head.weight_shapes()["w3"] == (512, 1)
    live.head.set_weights({k: v for k, v in new.items() if k != "goal_dim"})
    v_live, y_live = live(x)
    fresh = Run(Critic(new, lo=-0.1, hi=0.9, lib_path=lib, s_clip=5.0), gpu)
    v_new, y_new = fresh(x)
    assert same_bits(v_live, v_new) and same_bits(y_live, y_new) and not same_bits(v_old, v_new)
    live.close(); fresh.close()


@pytest.mark.parametrize("gated", [False, True])
def test_set_weights_equals_a_fresh_context_emulator(emu_lib, gated):
    check_refresh(emu_lib, False, gated)


@pytest.mark.gpu
@pytest.mark.parametrize("gated", [False, True])
def test_set_weights_equals_a_fresh_context_gpu(hip_lib, gated):
    check_refresh(hip_lib, True, gated)


# ---------------------------------------------------------------------------------------------------------------------------------- (8) closed loop
@pytest.mark.gpu
def test_closed_loop_style_reward_critic_and_returns_gpu(hip_lib):
    """64 envs of amp_heading_zombie, 8 steps: style reward from info["amp_obs"], gated critic on obs and on terminal_obs under row_mask = done, TD(lambda):
    all three equal the numpy references fed the device's own outputs, and the masked critic equals an unmasked one where done is set"""
    import torch
    from deepmimic_amd import model, returns
    from deepmimic_amd.vec_env import TorchVecEnv
    from test_td_returns import numpy_recursion
    T, N = 8, 64
    env = TorchVecEnv(model.load_asset("amp_heading_zombie"), N, seed=3, lib_path=hip_lib, amp_obs=True)
    env.env.set_time_limits(0.1, 0.2)
    S, G, AMP = env.obs_dim, env.goal_dim, env.env.amp_size
    assert G > 0 and AMP > 0
    critic = Critic(random_scalar_net(S + G, G, seed=5, scale=1.0), lo=-2.0, hi=2.0, val_fail=0.0, val_succ=20.0, lib_path=hip_lib)
    disc = Discriminator(random_scalar_net(AMP, seed=6, scale=0.5), reward_scale=2.0, task_reward_lerp=0.5, lib_path=hip_lib)
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    obs_all, goal_all = torch.zeros((T + 1, N, S), **f32), torch.zeros((T + 1, N, G), **f32)
    tobs, tgoal = torch.zeros((T, N, S), **f32), torch.zeros((T, N, G), **f32)
    rewards, logits, task = torch.zeros((T, N), **f32), torch.zeros((T, N), **f32), torch.zeros((T, N), **f32)
    terminate, done, valid = torch.zeros((T, N), **i32), torch.zeros((T, N), **i32), torch.zeros((T, N), **i32)
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    obs = env.reset()
    goal = torch.from_numpy(env.env.query_goal()).to(obs.device)          # the goal of the reset state (step hands it out as info["goal"] from then on)
    for t in range(T):
        obs_all[t], goal_all[t] = obs, goal
        acts = 0.6 * torch.randn((N, env.act_dim), generator=gen, **f32)
        obs, r, d, info = env.step(acts)
        goal = info["goal"]
        task[t] = r
        rewards[t], logits[t] = disc.eval_torch(info["amp_obs"], task_reward=r, raw=True)
        terminate[t], done[t], valid[t] = info["terminate"], d.to(torch.int32), info["valid"]
        tobs[t], tgoal[t] = info["terminal_obs"], info["terminal_goal"]
    obs_all[T], goal_all[T] = obs, goal
    ret, mask = returns.critic_returns_torch(critic, obs_all, goal_all, tobs, tgoal, terminate, done, valid, rewards, 0.95, 0.95, lib_path=hip_lib)
    values, values_raw = critic.eval_torch(obs_all, goal_all, raw=True)
    tv_masked, tv_masked_raw = critic.eval_torch(tobs, tgoal, row_mask=done, fill=0.0, raw=True)
    tv_full, tv_full_raw = critic.eval_torch(tobs, tgoal, raw=True)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in dict(rewards=rewards, logits=logits, task=task, values=values, vraw=values_raw, tvm=tv_masked, tvmraw=tv_masked_raw, tvf=tv_full,
                                             tvfraw=tv_full_raw, terminate=terminate, done=done, valid=valid, ret=ret, mask=mask).items()}
    dn = h["done"] != 0
    assert dn.sum() >= N and (~dn).any() and np.isfinite(h["values"]).all() and h["values"].std() > 0
    # style reward: the numpy statement on the device's logits (exact here: scale 2 and lerp 0.5 are powers of two -- up to the fp32 roundings of test (4))
    want_r = heads.reference_style_reward(h["logits"].astype(np.float64), 2.0, 0.5, h["task"].astype(np.float64))
    assert (np.abs(h["rewards"] - want_r) <= 6 * 2.0 ** -24 * np.maximum(1.0, np.abs(want_r))).all()
    # critic values: the numpy statement of the value head on the device's own net output, on obs and on the terminal observations
    assert np.isfinite(h["vraw"]).all() and np.isfinite(h["tvfraw"]).all() and h["vraw"].std() > 0
    assert same_bits(h["values"], heads.reference_value(h["vraw"], -2.0, 2.0))
    assert same_bits(h["tvf"], heads.reference_value(h["tvfraw"], -2.0, 2.0))
    # ... under row_mask = done: the statement with the mask on the UNMASKED call's net output, fill (0) in value and raw output elsewhere
    assert same_bits(h["tvm"], heads.reference_value(h["tvfraw"], -2.0, 2.0, row_mask=h["done"], fill=0.0))
    assert same_bits(h["tvmraw"], np.where(dn, h["tvfraw"], np.float32(0.0)))
    assert same_bits(h["tvm"][dn], h["tvf"][dn]) and not h["tvm"][~dn].any()
    print("CLOSED_LOOP done rows %d of %d, values clipped %.3f, |raw| max %.3f" % (dn.sum(), dn.size, (np.abs(h["vraw"]) > 2).mean(), np.abs(h["vraw"]).max()))
    want, wmask = numpy_recursion(h["rewards"], h["values"], h["tvm"], h["terminate"], h["done"], h["valid"], 0.95, 0.95, 0.0, 20.0)
    assert same_bits(h["ret"], want) and np.array_equal(h["mask"], wmask)
    critic.close(); disc.close(); env.close()
