"""Adam, global-norm gradient clipping and the non-finite guard of the device trainers (deepmimic_amd/csrc/dm_optim.h, include/dm_hip.h dm_train_opt_step,
deepmimic_amd/train.py) against the numpy statements beside the binding: reference_grad_norm, reference_opt_begin, reference_adam_step, reference_step.  Every check runs
on the emulator library through host addresses and again, marked `gpu`, through torch tensors.

The step is element-wise fp64 with every rounding point written down, and the norm is an fp64 sum in one fixed order that the mirror walks too: params, m, v, the eight
state words and the norm pass's partials are compared BIT FOR BIT.  Sizes: P in {1, 255, 256, 257} (the edges of a workgroup), 1024 / 255 * 1024 + 1 / 256 * 1024 + 1
(1, 256 and 257 partials of the norm pass: 257 is the first count at which a folding thread owns two) and 4096 * 256 + 1, the first P at which a thread of the step
kernel takes a second trip -- that one on the GPU only: a million fibers per launch take the emulator 13 s per case."""
import numpy as np
import pytest

from deepmimic_amd import train as tr
from deepmimic_amd.policy import Policy
from test_train import NET_A, NET_B, Emu, Gpu, _lib, blocks, net_weights

F = np.float32
EDGES = [1, 255, 256, 257, 1024, 255 * 1024 + 1, 256 * 1024 + 1, 4096 * 256 + 1]
PLAIN_PACKED = ("w1p", "w2p", "w3p", "b1", "b2", "b3")
ADAM = dict(kind="adam", stepsize=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_grad_norm=None, skip_nonfinite=False)
MOM = dict(ADAM, kind="momentum", stepsize=0.01)
ST = {k: i for i, k in enumerate(tr.OPT_STATE)}


class Run:
    """the device arrays of one optimiser -- params, m, v, grads, state, workspace -- and steps on them; pol None: the step alone"""

    def __init__(self, be, pol, params, m=None, v=None, state=None):
        self.be, self.pol, self.P = be, pol, int(np.size(params))
        z = np.zeros(self.P, F)
        self.nb = tr.opt_workspace_bytes(self.P, _lib(be))
        self.lay = tr.opt_workspace_layout(self.P)
        assert self.nb == self.lay["bytes"] and self.nb % 16 == 0
        self.d = dict(params=be.put(np.asarray(params, F)), m=be.put(z if m is None else np.asarray(m, F)), v=be.put(z if v is None else np.asarray(v, F)), grads=be.put(z),
                      state=be.put(np.zeros(8) if state is None else np.asarray(state, np.float64)), ws=be.put(np.zeros(self.nb // 8)))

    def load(self, name, a):
        h = self.d[name]
        if self.be.gpu:
            h.copy_(self.be.torch.from_numpy(np.ascontiguousarray(a)))
        else:
            h[...] = a

    def step(self, grads, cfg):
        be, d = self.be, self.d
        self.load("grads", np.asarray(grads, F))
        tr.opt_step_device(self.pol, be.ptr(d["params"]), be.ptr(d["m"]), be.ptr(d["v"]) if cfg["kind"] == "adam" else 0, be.ptr(d["grads"]), self.P, be.ptr(d["state"]),
                           be.ptr(d["ws"]), self.nb, stream=be.stream, lib=_lib(be), **cfg)
        return self

    def get(self, *names):
        out = tuple(self.be.get(self.d[k]) for k in names)
        return out if len(out) > 1 else out[0]

    def partials(self):
        raw = np.ascontiguousarray(self.get("ws")).view(np.uint8)
        piece = lambda k: raw[self.lay[k][0]:self.lay[k][0] + 8 * self.lay["groups"]].view(np.float64).copy()
        return piece("sum"), piece("count")

    def packed(self, names):
        return [self.pol.read_packed(k).tobytes() for k in names]


def same(a, b):
    """bit for bit, except that a NaN equals a NaN (the device and numpy need not agree on a NaN's payload)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all()) and np.array_equal(np.signbit(a[a == a]), np.signbit(b[b == b]))


def test_the_library_has_the_entry_points(emu_lib, tmp_path):
    """the symbols are there (asserted, not skipped), train._OptCfg is what a C compiler makes of dm_train_opt_cfg, and the workspace is the exported layout"""
    import ctypes
    import os
    import subprocess
    lib = _lib(Emu(emu_lib))
    assert hasattr(lib, "dm_train_opt_step") and hasattr(lib, "dm_train_opt_workspace_bytes")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [name for name, _ in tr._OptCfg._fields_]
    src = tmp_path / "cfg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm_hip.h"\nint main(void){ printf("%d %d %zu' + " %zu" * len(fields) + '\\n", DM_OPT_MOMENTUM, DM_OPT_ADAM, '
                   "sizeof(dm_train_opt_cfg), " + ", ".join("offsetof(dm_train_opt_cfg, %s)" % f for f in fields) + "); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "cfg")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "cfg")]).split()]
    assert got == [tr.OPT_KINDS["momentum"], tr.OPT_KINDS["adam"], ctypes.sizeof(tr._OptCfg)] + [getattr(tr._OptCfg, f).offset for f in fields]
    for P in (1, 1024, 1025):
        assert tr.opt_workspace_bytes(P, lib) == tr.opt_workspace_layout(P)["bytes"] == 32 + 16 * ((P + 1023) // 1024)
    for P in (0, -1, 2 ** 40 + 1):
        with pytest.raises(RuntimeError, match="dm_train_opt_workspace_bytes: P must be in"):
            tr.opt_workspace_bytes(P, lib)


@pytest.mark.gpu
def test_the_library_has_the_entry_points_gpu(hip_lib):
    lib = _lib(Gpu(hip_lib))
    assert hasattr(lib, "dm_train_opt_step") and hasattr(lib, "dm_train_opt_workspace_bytes")


# ---------------------------------------------------------------- 1. bits at the index edges, no net

def check_edges(be, P, kind):
    """three steps from a zero state with clipping (active: the norm of P standard normals against max_grad_norm 0.5) and the guard on, so that all three kernels run"""
    rng = np.random.default_rng([P, kind == "adam"])
    cfg = dict(ADAM if kind == "adam" else MOM, max_grad_norm=0.5, skip_nonfinite=True, grad_scale=0.75)
    w = rng.standard_normal(P).astype(F)
    m0 = (0.1 * rng.standard_normal(P)).astype(F); v0 = (0.01 * rng.random(P)).astype(F)
    run = Run(be, None, w, m0, v0)
    rw, rm, rv, rs = w, m0, v0, np.zeros(8)
    for it in range(3):
        g = rng.standard_normal(P).astype(F)
        run.step(g, cfg)
        rw, rm, rv, rs = tr.reference_opt_step(rs, cfg, rw, rm, rv, g)
        dw, dm, dv, ds = run.get("params", "m", "v", "state")
        assert np.array_equal(ds, rs), (it, ds, rs)
        assert np.array_equal(dw, rw) and np.array_equal(dm, rm) and np.array_equal(dv, rv), it
        assert rs[ST["t"]] == it + 1 and rs[ST["skipped"]] == 0 and rs[ST["scale"]] <= 1.0
        p1 = p2 = 1.0
        for _ in range(it + 1):
            p1 *= float(F(cfg["beta1"])); p2 *= float(F(cfg["beta2"]))
        assert ds[ST["pow1"]] == p1 and ds[ST["pow2"]] == p2
    assert rs[ST["scale"]] < 1.0 or P < 4
    total, count, norm, (gs, gc) = tr.reference_grad_norm(g, grad_scale=cfg["grad_scale"])
    ps, pc = run.partials()
    assert np.array_equal(ps, gs) and np.array_equal(pc, gc) and count == 0 and ps.size == (P + 1023) // 1024
    if kind == "momentum":
        assert np.array_equal(dv, v0)                       # MOMENTUM never touches v


@pytest.mark.parametrize("kind", ["momentum", "adam"])
@pytest.mark.parametrize("P", EDGES[:-1])
def test_edges_bit_for_bit(emu_lib, P, kind):
    check_edges(Emu(emu_lib), P, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["momentum", "adam"])
@pytest.mark.parametrize("P", EDGES)
def test_edges_bit_for_bit_gpu(hip_lib, P, kind):
    check_edges(Gpu(hip_lib), P, kind)


def check_against_torch_adam(be, P=4097):
    """One step from zero moments against torch.optim.Adam in float64 on the CPU, fed the gradient the kernel forms (s g, s from the state's scale) and the float32
    values of the betas and eps.  The device stores m' and v' in fp32: 2^-24 relative each, v' under a square root, so the update is within
    (2^-24 + 2^-25)(1 + O(2^-24)) < 2^-22 relative of torch's, and w' is rounded once: |w' - w_torch| <= 0.5 ulp(w') + stepsize |update| 2^-22."""
    import torch
    rng = np.random.default_rng(5)
    cfg = dict(ADAM, stepsize=1e-2, max_grad_norm=1.0, grad_scale=0.5)
    w, g = rng.standard_normal(P).astype(F), rng.standard_normal(P).astype(F)
    run = Run(be, None, w).step(g, cfg)
    dw, ds = run.get("params", "state")
    s = np.float64(F(cfg["grad_scale"] * ds[ST["scale"]]))
    p = torch.tensor(w.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=cfg["stepsize"], betas=(float(F(cfg["beta1"])), float(F(cfg["beta2"]))), eps=float(F(cfg["eps"])))
    p.grad = torch.tensor(s * g.astype(np.float64))
    opt.step()
    ref = p.detach().numpy()
    upd = np.abs(ref - w.astype(np.float64))
    ulp = np.maximum(np.spacing(np.abs(dw)), np.spacing(np.abs(ref.astype(F)))).astype(np.float64)
    err = np.abs(dw.astype(np.float64) - ref)
    print("adam against torch float64: max err / bound = %.3g" % (err / (0.5 * ulp + upd * 2.0 ** -22)).max())
    assert (err <= 0.5 * ulp + upd * 2.0 ** -22).all() and ds[ST["scale"]] < 1.0 and upd.min() > 0


def test_adam_against_torch(emu_lib):
    check_against_torch_adam(Emu(emu_lib))


@pytest.mark.gpu
def test_adam_against_torch_gpu(hip_lib):
    check_against_torch_adam(Gpu(hip_lib))


# ---------------------------------------------------------------- 2. the old step is a special case

def check_old_step_plain(be):
    net = NET_B
    w = net_weights(net, seed=2)
    flat = tr.pack_params(w); P = flat.size
    rng = np.random.default_rng(8)
    mom, grads = rng.standard_normal(P).astype(F) * 0.1, rng.standard_normal(P).astype(F)
    lr, mo, wd, gs = 0.01, 0.9, 1e-3, 0.5
    old_pol, new_pol = Policy(w, lib_path=be.lib), Policy(w, lib_path=be.lib)
    d = [be.put(a) for a in (flat, mom, grads)]
    tr.sgd_step_device(old_pol, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), P, lr, mo, wd, gs, stream=be.stream)
    run = Run(be, new_pol, flat, mom).step(grads, dict(MOM, stepsize=lr, beta1=mo, weight_decay=wd, grad_scale=gs))
    assert be.get(d[0]).tobytes() == run.get("params").tobytes() and be.get(d[1]).tobytes() == run.get("m").tobytes()
    assert [old_pol.read_packed(k).tobytes() for k in PLAIN_PACKED] == run.packed(PLAIN_PACKED)
    assert run.packed(PLAIN_PACKED) != [Policy(w, lib_path=be.lib).read_packed(k).tobytes() for k in PLAIN_PACKED]
    st = run.get("state")
    assert list(st) == [1.0, float(F(mo)), float(F(0.999)), 0.0, 0.0, 1.0, 0.0, 0.0]                # no norm pass: words 4 and 6 are 0


def check_old_step_gated(be):
    from test_train_gated import GA, PACKED, dims, gated_weights
    w = gated_weights(GA, seed=2)
    flat = tr.pack_gated_params(w); P = flat.size
    rng = np.random.default_rng(9)
    mom, grads = rng.standard_normal(P).astype(F) * 0.1, rng.standard_normal(P).astype(F)
    lr, mo, wd, gs = 0.01, 0.9, 1e-3, 0.5
    old_pol, new_pol = Policy(w, lib_path=be.lib), Policy(w, lib_path=be.lib)
    d = [be.put(a) for a in (flat, mom, grads)]
    tr.gated_sgd_step_device(old_pol, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), P, lr, mo, wd, gs, stream=be.stream)
    run = Run(be, new_pol, flat, mom).step(grads, dict(MOM, stepsize=lr, beta1=mo, weight_decay=wd, grad_scale=gs))
    assert be.get(d[0]).tobytes() == run.get("params").tobytes() and be.get(d[1]).tobytes() == run.get("m").tobytes()
    assert [old_pol.read_packed(k).tobytes() for k in PACKED] == run.packed(PACKED)


def test_old_step_is_a_special_case(emu_lib):
    check_old_step_plain(Emu(emu_lib)); check_old_step_gated(Emu(emu_lib))


@pytest.mark.gpu
def test_old_step_is_a_special_case_gpu(hip_lib):
    check_old_step_plain(Gpu(hip_lib)); check_old_step_gated(Gpu(hip_lib))


# ---------------------------------------------------------------- 3. the norm

def check_norm(be):
    from fractions import Fraction
    cfg = dict(MOM, stepsize=0.0, skip_nonfinite=True, grad_scale=-0.5)
    # entries +-2^k: every square and every partial sum is exact in fp64, whatever the order
    rng = np.random.default_rng(3)
    P = 3 * 1024 + 77
    g = (rng.choice([-1.0, 1.0], P) * 2.0 ** rng.integers(-3, 4, P)).astype(F)
    run = Run(be, None, np.zeros(P, F)).step(g, cfg)
    exact = sum(Fraction(float(x)) ** 2 for x in g)
    ps, pc = run.partials()
    assert sum(Fraction(float(x)) for x in ps) == exact and not pc.any()
    assert run.get("state")[ST["norm"]] == 0.5 * np.sqrt(np.float64(float(exact))) and float(exact) == exact
    # a perfect square: 2304 entries +-2, sum 96^2, norm 0.5 * 96
    g2 = (2.0 * rng.choice([-1.0, 1.0], 2304)).astype(F)
    assert Run(be, None, np.zeros(2304, F)).step(g2, cfg).get("state")[ST["norm"]] == 48.0
    # random gradients: the mirror's bits; float64 numpy within P 2^-53 relative (each of the P - 1 additions rounds once, the squares are exact)
    for P in (1000, 70001):
        g = rng.standard_normal(P).astype(F)
        a = Run(be, None, np.zeros(P, F)).step(g, cfg)
        b = Run(be, None, np.zeros(P, F)).step(g, cfg)
        total, count, norm, (gs, gc) = tr.reference_grad_norm(g, grad_scale=cfg["grad_scale"])
        st = a.get("state")
        assert st[ST["norm"]] == norm and st[ST["nonfinite"]] == 0 and np.array_equal(a.partials()[0], gs)
        ref = 0.5 * np.linalg.norm(g.astype(np.float64))
        assert abs(norm - ref) <= P * 2.0 ** -53 * ref
        assert a.get("state").tobytes() == b.get("state").tobytes() and a.get("ws").tobytes() == b.get("ws").tobytes()


def test_norm(emu_lib):
    check_norm(Emu(emu_lib))


@pytest.mark.gpu
def test_norm_gpu(hip_lib):
    check_norm(Gpu(hip_lib))


# ---------------------------------------------------------------- 4. the clip

def check_clip(be, kind):
    net = NET_B
    S, H1, H2, A = net["S"], net["H1"], net["H2"], net["A"]
    w = net_weights(net, seed=2)
    flat = tr.pack_params(w); P = flat.size
    mask = tr.matrix_mask_of(S, H1, H2, A)
    rng = np.random.default_rng(14)
    m0, v0, g = (0.1 * rng.standard_normal(P)).astype(F), (0.01 * rng.random(P)).astype(F), rng.standard_normal(P).astype(F)
    base = dict(ADAM if kind == "adam" else MOM, weight_decay=1e-3, grad_scale=0.5)
    norm = tr.reference_grad_norm(g, grad_scale=base["grad_scale"])[2]
    for what, mx in (("below", 2.0 * norm), ("above", 0.5 * norm), ("at", norm)):
        cfg = dict(base, max_grad_norm=mx)
        run = Run(be, Policy(w, lib_path=be.lib), flat, m0, v0).step(g, cfg)
        dw, dm, dv, ds = run.get("params", "m", "v", "state")
        rw, rm, rv, rs = tr.reference_opt_step(np.zeros(8), cfg, flat, m0, v0, g, mask)
        assert np.array_equal(ds, rs) and ds[ST["norm"]] == norm, what
        assert (ds[ST["scale"]] == 1.0) == (what == "below") and (what != "at" or ds[ST["scale"]] == mx / (mx + 1e-6) < 1.0)
        assert np.array_equal(dw, rw) and np.array_equal(dm, rm) and np.array_equal(dv, rv), what
        # the same arrays as an unclipped step whose grad_scale is the mirror's s
        s = tr.reference_opt_begin(np.zeros(8), cfg, *tr.reference_grad_norm(g, grad_scale=cfg["grad_scale"])[:2])[1]["s"]
        pre = Run(be, Policy(w, lib_path=be.lib), flat, m0, v0).step(g, dict(base, grad_scale=float(s)))
        assert pre.get("params").tobytes() == dw.tobytes() and pre.get("m").tobytes() == dm.tobytes() and pre.get("v").tobytes() == dv.tobytes(), what
        assert pre.packed(PLAIN_PACKED) == run.packed(PLAIN_PACKED)
        # the decay reaches the matrices and no bias
        nod = Run(be, Policy(w, lib_path=be.lib), flat, m0, v0).step(g, dict(cfg, weight_decay=0.0))
        assert np.array_equal(nod.get("params")[~mask], dw[~mask]) and np.array_equal(nod.get("m")[~mask], dm[~mask]) and not np.array_equal(nod.get("m")[mask], dm[mask])


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_clip(emu_lib, kind):
    check_clip(Emu(emu_lib), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_clip_gpu(hip_lib, kind):
    check_clip(Gpu(hip_lib), kind)


# ---------------------------------------------------------------- 5. the guard

def check_guard(be, kind):
    net = NET_A
    w = net_weights(net, seed=3)
    flat = tr.pack_params(w); P = flat.size
    lay = tr.layout(net["S"], net["H1"], net["H2"], net["A"])
    rng = np.random.default_rng(15)
    g1, g2, g3 = (rng.standard_normal(P).astype(F) for _ in range(3))
    cfg = dict(ADAM if kind == "adam" else MOM, weight_decay=1e-3, max_grad_norm=10.0, skip_nonfinite=True)
    clean = Run(be, Policy(w, lib_path=be.lib), flat).step(g1, cfg).step(g3, cfg)
    names = ("params", "m", "v")
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0,), (P - 1,), (lay["b2"][0] + 5,), (0, lay["b1"][0], P - 1)):
            run = Run(be, Policy(w, lib_path=be.lib), flat).step(g1, cfg)
            before, st0, packed0 = [a.tobytes() for a in run.get(*names)], run.get("state"), run.packed(PLAIN_PACKED)
            gb = g2.copy(); gb[list(at)] = bad
            run.step(gb, cfg)
            st1 = run.get("state")
            assert [a.tobytes() for a in run.get(*names)] == before and run.packed(PLAIN_PACKED) == packed0, (bad, at)
            assert st1[:3].tobytes() == st0[:3].tobytes() and st1[ST["skipped"]] == st0[ST["skipped"]] + 1 == 1 and st1[ST["nonfinite"]] == len(at), (bad, at, st1)
            run.step(g3, cfg)
            st2, ref = run.get("state"), clean.get("state")
            assert [a.tobytes() for a in run.get(*names)] == [a.tobytes() for a in clean.get(*names)] and run.packed(PLAIN_PACKED) == clean.packed(PLAIN_PACKED), (bad, at)
            assert st2[ST["skipped"]] == 1 and ref[ST["skipped"]] == 0 and np.delete(st2, ST["skipped"]).tobytes() == np.delete(ref, ST["skipped"]).tobytes()
            assert st2[ST["t"]] == 2 and st2[ST["nonfinite"]] == 0
    # the guard off: the non-finite value spreads as the arithmetic says (a NaN norm: s = NaN, every element; an infinite norm: scale 0 and 0 * inf = NaN in that element)
    mask = tr.matrix_mask_of(net["S"], net["H1"], net["H2"], net["A"])
    for bad in (np.nan, np.inf):
        off = dict(cfg, skip_nonfinite=False)
        gb = g2.copy(); gb[7] = bad
        run = Run(be, Policy(w, lib_path=be.lib), flat).step(g1, off)
        r = tr.reference_opt_step(np.zeros(8), off, flat, np.zeros(P, F), np.zeros(P, F), g1, mask)
        run.step(gb, off)
        r = tr.reference_opt_step(r[3], off, r[0], r[1], r[2], gb, mask)
        dw, dm, dv, ds = run.get("params", "m", "v", "state")
        assert same(dw, r[0]) and same(dm, r[1]) and same(dv, r[2]) and same(ds, r[3]), bad
        assert np.isnan(dw[7]) and np.isnan(dw).all() == (bad != bad) and ds[ST["nonfinite"]] == 1 and ds[ST["skipped"]] == 0 and ds[ST["t"]] == 2


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_guard(emu_lib, kind):
    check_guard(Emu(emu_lib), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_guard_gpu(hip_lib, kind):
    check_guard(Gpu(hip_lib), kind)


# ---------------------------------------------------------------- 6. gated and discriminator contexts

def check_contexts(be):
    from deepmimic_amd import heads
    from test_train_gated import GA, PACKED, dims, gated_weights, grad_blocks
    cfg = dict(ADAM, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
    rng = np.random.default_rng(16)
    # the smallest gated net: the decay on its ten matrices, all twenty packed arrays refreshed
    w = gated_weights(GA, seed=4)
    flat = tr.pack_gated_params(w); P = flat.size
    mask = tr.gated_matrix_mask_of(*dims(GA))
    lay = tr.gated_layout(*dims(GA))
    assert sum(len(lay[k][1]) == 2 for k in tr.GATED_KEYS) == 10
    g = rng.standard_normal(P).astype(F)
    pol = Policy(w, lib_path=be.lib)
    run = Run(be, pol, flat).step(g, cfg)
    r = tr.reference_opt_step(np.zeros(8), cfg, flat, np.zeros(P, F), np.zeros(P, F), g, mask)
    for got, ref in zip(run.get("params", "m", "v", "state"), r):
        assert np.array_equal(got, ref)
    nod = Run(be, Policy(w, lib_path=be.lib), flat).step(g, dict(cfg, weight_decay=0.0))
    new, plain = grad_blocks(GA, None, run.get("m")), grad_blocks(GA, None, nod.get("m"))
    for k in tr.GATED_KEYS:
        assert np.array_equal(new[k], plain[k]) == (new[k].ndim == 1), k
    fresh, stale = Policy(dict(w, **grad_blocks(GA, None, run.get("params"))), lib_path=be.lib), Policy(w, lib_path=be.lib)
    for k in PACKED:
        assert np.array_equal(pol.read_packed(k), fresh.read_packed(k)) and not np.array_equal(pol.read_packed(k), stale.read_packed(k)), k
    with pytest.raises(RuntimeError, match="dm_train_opt_step: P is .*dm_train_gated_param_count"):
        Run(be, pol, flat[:-1]).step(g[:-1], cfg)
    # a discriminator's context: a plain net with one output, the decay on its three matrices
    net = dict(NET_A, A=1)
    wd_ = net_weights(net, seed=11, A=1, normalisers=False)
    disc = heads.Discriminator(wd_, lib_path=be.lib)
    flat = tr.pack_params(wd_); P = flat.size
    mask = tr.matrix_mask_of(net["S"], net["H1"], net["H2"], 1)
    g = rng.standard_normal(P).astype(F)
    run = Run(be, disc.net, flat).step(g, cfg)
    r = tr.reference_opt_step(np.zeros(8), cfg, flat, np.zeros(P, F), np.zeros(P, F), g, mask)
    for got, ref in zip(run.get("params", "m", "v", "state"), r):
        assert np.array_equal(got, ref)
    nod = Run(be, heads.Discriminator(wd_, lib_path=be.lib).net, flat).step(g, dict(cfg, weight_decay=0.0))
    assert np.array_equal(nod.get("m")[~mask], run.get("m")[~mask]) and (nod.get("m")[mask] != run.get("m")[mask]).mean() > 0.9
    fresh = Policy(dict(wd_, **blocks(net, 1, run.get("params"))), lib_path=be.lib)
    assert run.packed(PLAIN_PACKED) == [fresh.read_packed(k).tobytes() for k in PLAIN_PACKED]


def test_gated_and_discriminator_contexts(emu_lib):
    check_contexts(Emu(emu_lib))


@pytest.mark.gpu
def test_gated_and_discriminator_contexts_gpu(hip_lib):
    check_contexts(Gpu(hip_lib))


# ---------------------------------------------------------------- 7. it trains

def check_critic_trains(be):
    """the critic case of test_train.py check_it_trains through CriticTrainer(optimizer="adam"), clipping and the guard on: 30 steps, the loss ends below where it began"""
    import torch
    net, n, steps = NET_A, 256, 30
    w = net_weights(net, seed=4, A=1)
    rng = np.random.default_rng(12)
    states = rng.standard_normal((n, net["S"])).astype(F)
    targets = ((states - w["s_mean"]) / w["s_std"] @ rng.uniform(-0.3, 0.3, net["S"])).astype(F)
    pol = Policy(w, lib_path=be.lib)
    dev = torch.device(be.device())
    trn = tr.CriticTrainer.from_policy(pol, w, stepsize=1e-3, device=dev, optimizer="adam", max_grad_norm=5.0, skip_nonfinite=True)
    assert tuple(trn.buf.shape) == (4, trn.P) and trn.opt_state.dtype == torch.float64 and tuple(trn.opt_state.shape) == (8,)
    d_s, d_t = torch.from_numpy(states).to(dev), torch.from_numpy(targets).to(dev)
    losses, norms = [], []
    for it in range(steps):
        trn.grad(d_s, d_t)
        losses.append(float(trn.stats().cpu()[0]))
        trn.step()
        norms.append(float(trn.grad_norm().cpu()))
    print("critic training with adam: loss %.4g -> %.4g in %d steps; gradient norm %.3g -> %.3g, last scale %.3g" % (losses[0], losses[-1], steps, norms[0], norms[-1],
                                                                                                              float(trn.grad_scale_applied().cpu())))
    assert losses[-1] < losses[0] and np.isfinite(losses).all() and np.isfinite(trn.buf.cpu().numpy()).all()
    assert float(trn.skipped().cpu()) == 0 and float(trn.opt_state.cpu()[0]) == steps
    fresh = Policy(dict(w, **blocks(net, 1, trn.params.cpu().numpy())), lib_path=be.lib)
    assert np.array_equal(pol.read_packed("w1p"), fresh.read_packed("w1p")) and np.array_equal(pol.read_packed("b3"), fresh.read_packed("b3"))
    # the defaults keep the old path: [3, P], no state
    old = tr.CriticTrainer.from_policy(Policy(w, lib_path=be.lib), w, stepsize=0.01, device=dev)
    assert tuple(old.buf.shape) == (3, old.P) and old.opt_state is None
    with pytest.raises(RuntimeError, match="keeps no optimiser state"):
        old.grad_norm()


def check_disc_trains(be):
    """the two clusters of test_train_disc.py check_disc_trains through DiscTrainer(optimizer="adam") for 30 steps: the loss ends below where it began, everything finite"""
    import torch
    from deepmimic_amd import heads
    net, n, steps = dict(NET_A, A=1), 64, 30
    S = net["S"]
    w = net_weights(net, seed=11, A=1, normalisers=False)
    rng = np.random.default_rng(21)
    c = rng.standard_normal(S).astype(F); c *= 2.0 / np.linalg.norm(c)
    expert = (c + 0.3 * rng.standard_normal((n, S))).astype(F); agent = (-c + 0.3 * rng.standard_normal((n, S))).astype(F)
    disc = heads.Discriminator(w, lib_path=be.lib)
    dev = torch.device(be.device())
    trn = tr.DiscTrainer.from_policy(disc.net, w, stepsize=1e-3, weight_decay=1e-4, device=dev, optimizer="adam", max_grad_norm=10.0, skip_nonfinite=True)
    d_e, d_a = torch.from_numpy(expert).to(dev), torch.from_numpy(agent).to(dev)
    losses = []
    for _ in range(steps):
        trn.grad(d_e, d_a, grad_penalty=10.0, logit_reg=0.05)
        losses.append(float(trn.loss().cpu()))
        trn.step()
    print("disc training with adam: loss %.4g -> %.4g in %d steps, skipped %g" % (losses[0], losses[-1], steps, float(trn.skipped().cpu())))
    assert losses[-1] < losses[0] and np.isfinite(losses).all() and np.isfinite(trn.buf.cpu().numpy()).all()


def test_it_trains(emu_lib):
    check_critic_trains(Emu(emu_lib)); check_disc_trains(Emu(emu_lib))


@pytest.mark.gpu
def test_it_trains_gpu(hip_lib):
    check_critic_trains(Gpu(hip_lib)); check_disc_trains(Gpu(hip_lib))


# ---------------------------------------------------------------- 8. resume

def check_resume(be):
    import torch
    net, n = NET_A, 32
    w = net_weights(net, seed=6, A=1)
    rng = np.random.default_rng(18)
    dev = torch.device(be.device())
    states = torch.from_numpy(rng.standard_normal((n, net["S"])).astype(F)).to(dev); targets = torch.from_numpy(rng.standard_normal(n).astype(F)).to(dev)
    make = lambda: tr.CriticTrainer.from_policy(Policy(w, lib_path=be.lib), w, stepsize=1e-3, weight_decay=1e-4, device=dev, optimizer="adam", max_grad_norm=0.5)
    whole = make()
    for it in range(3):
        if it == 2:
            saved = (whole.buf.clone(), whole.opt_state.clone())
        whole.grad(states, targets); whole.step()
    resumed = make()
    resumed.buf.copy_(saved[0]); resumed.opt_state.copy_(saved[1]); resumed.sync()
    resumed.grad(states, targets); resumed.step()
    assert resumed.buf.cpu().numpy().tobytes() == whole.buf.cpu().numpy().tobytes() and resumed.opt_state.cpu().numpy().tobytes() == whole.opt_state.cpu().numpy().tobytes()
    assert float(resumed.opt_state.cpu()[0]) == 3
    assert [resumed.policy.read_packed(k).tobytes() for k in PLAIN_PACKED] == [whole.policy.read_packed(k).tobytes() for k in PLAIN_PACKED]


def test_resume(emu_lib):
    check_resume(Emu(emu_lib))


@pytest.mark.gpu
def test_resume_gpu(hip_lib):
    check_resume(Gpu(hip_lib))


# ---------------------------------------------------------------- 10. refusals

def check_refusals(be):
    """every refusal of include/dm_hip.h by name, nothing written: every array keeps its sentinel"""
    net = NET_A
    w = net_weights(net, seed=3)
    pol = Policy(w, lib_path=be.lib)
    P = tr.param_count(pol)
    nb = tr.opt_workspace_bytes(P, _lib(be))
    sent = lambda: be.put(np.full(P, -77.0, F))
    params, m, v, grads = sent(), sent(), sent(), sent()
    state, ws = be.put(np.full(9, -77.0)), be.put(np.full(nb // 8 + 2, -77.0))
    p = be.ptr
    packed0 = [pol.read_packed(k).tobytes() for k in PLAIN_PACKED]

    def call(pol_=pol, P_=P, nb_=nb, ws_=None, state_=None, null=None, **kw):
        a = dict(params=p(params), m=p(m), v=p(v), grads=p(grads), state=p(state) if state_ is None else state_, ws=p(ws) if ws_ is None else ws_)
        if null:
            a[null] = 0
        cfg = dict(ADAM, **kw)
        tr.opt_step_device(pol_, a["params"], a["m"], a["v"], a["grads"], P_, a["state"], a["ws"], nb_, stream=be.stream, lib=_lib(be), **cfg)

    nan, inf = float("nan"), float("inf")
    cases = [("null argument", dict(null="params")), ("null argument", dict(null="m")), ("null argument", dict(null="grads")), ("null argument", dict(null="state")),
             ("null argument", dict(null="ws")), ("kind must be DM_OPT_MOMENTUM or DM_OPT_ADAM", dict(kind=2)), ("kind must be", dict(kind=-1)),
             ("ADAM needs v_dev", dict(null="v")),
             ("beta1 and beta2 must be in", dict(beta1=1.0)), ("beta1 and beta2 must be in", dict(beta1=-0.1)), ("beta1 and beta2 must be in", dict(beta2=1.0)),
             ("beta1 and beta2 must be in", dict(beta2=nan)), ("beta1 and beta2 must be in", dict(beta2=1.0 - 1e-12)),
             ("momentum must be finite", dict(kind="momentum", beta1=-0.5)), ("momentum must be finite", dict(kind="momentum", beta1=inf)),
             ("eps must be finite and > 0", dict(eps=0.0)), ("eps must be finite and > 0", dict(eps=-1e-8)), ("eps must be finite and > 0", dict(eps=1e-60)),
             ("stepsize must be finite", dict(stepsize=-1.0)), ("stepsize must be finite", dict(stepsize=inf)),
             ("weight_decay must be finite", dict(weight_decay=-1e-3)), ("weight_decay must be finite", dict(weight_decay=nan)),
             ("grad_scale must be finite", dict(grad_scale=inf)), ("max_grad_norm must not be NaN", dict(max_grad_norm=nan)),
             ("P must be in", dict(pol_=None, P_=0)), ("the net has .* parameters \\(dm_train_param_count\\)", dict(P_=P - 1)),
             ("weight_decay needs the net", dict(pol_=None, weight_decay=0.1)),
             ("state must be 8-byte aligned", dict(state_=p(state) + 4)),
             ("workspace too small", dict(nb_=nb - 1)), ("workspace must be 16-byte aligned", dict(ws_=p(ws) + 8))]
    for what, kw in cases:
        with pytest.raises(RuntimeError, match="dm_train_opt_step: .*" + what):
            call(**kw)
    with pytest.raises(RuntimeError, match="dm_train_opt_step: null argument"):
        lib = _lib(be)
        tr.check(lib, lib.dm_train_opt_step(pol.h, None, p(params), p(m), p(v), p(grads), P, p(state), p(ws), nb, None))
    for name, t in dict(params=params, m=m, v=v, grads=grads, state=state, ws=ws).items():
        assert (be.get(t) == -77).all(), name
    assert [pol.read_packed(k).tobytes() for k in PLAIN_PACKED] == packed0
    # the trainers' own argument
    with pytest.raises(ValueError, match="optimizer must be"):
        tr.CriticTrainer.from_policy(Policy(net_weights(net, seed=3, A=1), lib_path=be.lib), net_weights(net, seed=3, A=1), stepsize=0.1, device=be.device(), optimizer="sgd")


def test_refusals(emu_lib):
    check_refusals(Emu(emu_lib))


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    check_refusals(Gpu(hip_lib))
