"""The gated actor of the AMP task policies (learning/nets/fc_2layers_gated_1024units.py; deepmimic_amd/csrc/dm_policy.h GateDev, k_policy_gate and the
GATED epilogues; include/dm_hip.h dm_policy_create_gated) in the manner of tests/test_policy_kernels.py, whose helpers it borrows.

GATED_PATHS is the ledger: one row per (shape, environment switches) with the (path id, gated) the library must report: the four k_policy_fused<.., true>
instantiations, the per-layer kernel kinds by the existing switches, other widths.  Every row runs on the emulator and under `-m gpu` through raw device pointers:

(a) exact: integer-valued networks extended to the gate -- integer c, e_i, beta_i of magnitude <= 256, scale pre-activations that are multiples of 128 (0 or
    of magnitude >= 128), so sigma (float64, rounded to fp32) is exactly 0, 1 or 2 and every gated activation an integer exact in bf16.  The result does not
    depend on summation order, MFMA order or fma contraction: actions equal the float64 statement BIT FOR BIT.  The precondition is asserted on the
    reference alone before the kernel is looked at.
(b) neutral gate (scale and bias projections zero: sigma = 1, beta = 0) == the plain actor on the same w1 .. w3 on the same path id, bit for bit;
(c) on random weights fused == per-layer with 64-row and with 128-row tiles bit for bit, one-wave to 1e-5 (the bounds the plain paths are held to);
(d) random Xavier weights against the bf16-point and the float64 statement (bound: see RANDOM_BOUND);
(e) sampling, coin, flags, logp, null pointers: check_sampling of test_policy_kernels.py; non-finite observations and goals.
"""
from dataclasses import dataclass, field

import numpy as np
import pytest

from deepmimic_amd.policy import GATE_KEYS, Policy, random_weights, reference_forward
from test_policy_kernels import (FUSED_8_2, FUSED_8_4, FUSED_12_2, FUSED_12_4, HALF_LOG_2PI, LAYERED, ONE_WAVE, ROWS_EMU, ROWS_GPU, S_CLIP, TILE128, TILE64_TILE64, TILE64_WAVE, TILE128_TILE128,
                                 WAVE_WAVE, Runner, check_sampling, integer_inputs, set_env)

GC, GH = 128, 64


@dataclass(frozen=True)
class GRow:
    """S counts the G goal columns; inside: the goal travels in the last columns of states_dev (goal_dim = 0) instead of its own block"""
    S: int
    G: int
    A: int
    path: int
    K1: int
    N3: int
    H1: int = 1024
    H2: int = 512
    env: tuple = ()
    inside: bool = False
    note: str = field(default="", compare=False)


GATED_PATHS = {
    # one launch: k_policy_fused<8 | 12, 2 | 4, true>
    "hum_a36": GRow(200, 3, 36, FUSED_8_4, 256, 64, note="humanoid 197 + 3 (heading), A = 36: the shipped shape"),
    "hum_a28": GRow(200, 3, 28, FUSED_8_2, 256, 32, note="N3 = 32"),
    "dog": GRow(350, 3, 58, FUSED_12_4, 384, 64, note="dog 347 + 3"),
    "dog_a28": GRow(352, 5, 28, FUSED_12_2, 384, 32),
    "split": GRow(300, 50, 28, FUSED_12_2, 384, 32, note="S - G = 250: the state / goal boundary inside a 4-column group; G = 50 is two k-steps of the gate; K1 320 re-padded"),
    "g1": GRow(227, 1, 36, FUSED_8_4, 256, 64, note="G = 1"),
    "inside": GRow(200, 3, 36, FUSED_8_4, 256, 64, inside=True, note="goal_dim = 0: the goal in the last columns of states_dev"),
    # one per per-layer kernel kind, by the existing switches
    "lay_tile64": GRow(200, 3, 36, TILE64_TILE64, 256, 64, env=(LAYERED,), note="k_policy_gate, gemm<0,64,true> gemm<1,64,true>"),
    "lay_tile128": GRow(206, 9, 36, TILE128_TILE128, 256, 64, env=(LAYERED, TILE128), note="gemm<0,128,true> gemm<1,128,true>"),
    "lay_wave": GRow(200, 3, 36, WAVE_WAVE, 256, 64, env=(LAYERED, ONE_WAVE), note="layer<0,4,4,true> layer<1,2,4,true>"),
    # non-reference hidden widths
    "tile64_wave": GRow(70, 6, 33, TILE64_WAVE, 128, 64, H1=128, H2=192, note="gemm<0,64,true> with KS = 4, layer<1,2,4,true>"),
    "h64": GRow(40, 6, 5, WAVE_WAVE, 64, 32, H1=64, H2=64, note="KS = 2 in every layer"),
}


def test_ledger_covers_what_the_gate_needs():
    rows = GATED_PATHS.values()
    assert {r.path for r in rows} >= {FUSED_8_2, FUSED_8_4, FUSED_12_2, FUSED_12_4, TILE64_TILE64, TILE128_TILE128, WAVE_WAVE, TILE64_WAVE}
    assert any(r.path < 16 and (r.S - r.G) % 4 for r in rows) and any(r.path < 16 and r.G == 1 for r in rows) and any(r.path < 16 and r.inside for r in rows)
    assert any((r.S - r.G) % 4 for r in rows) and any(r.G == 1 for r in rows) and any(r.G > 32 for r in rows) and any(r.inside for r in rows)
    assert any((r.H1, r.H2) != (1024, 512) for r in rows)
    for name, r in GATED_PATHS.items():
        assert 1 <= r.G < r.S and r.K1 % 64 == 0 and r.K1 >= r.S and r.N3 == (r.A + 31) // 32 * 32, name


# ---------------------------------------------------------------------------------------------------------------------------------- the integer network
def integer_gated_net(row, seed):
    """Main net: w1 with 16 and w2 with 2 non-zeros (+-1) per column, so that twice the largest pre-activation plus beta stays below 256 (pre-activation of
    layer 1: second moment ~1.5 x 16, largest of 4097 x 1024 near 5.5 sigma = 27, more with the clipped inputs of magnitude 6; h1 second moment ~ 20 and a
    heavy tail, layer 2 over 2 of them; doubled by sigma = 2 and shifted by beta; 32 / 4 non-zeros gave h2 up to 271 in the float64 reference).  Gate:
    kernels +-1 with two non-zeros per column (c <= 14, e_i <= 30), the bias projection one (|beta| <= 32), the scale projection 128 x (+-1, two per
    column) with biases in {-128, 0, 128}: its pre-activation is a multiple of 128.  check_gated_reference decides."""
    rng = np.random.default_rng(seed)
    S, G, A, H1, H2 = row.S, row.G, row.A, row.H1, row.H2
    pm1 = lambda *sh: rng.choice(np.array([-1.0, 1.0], np.float32), size=sh)

    def sparse(k, n, d, scale=1.0):
        w = np.zeros((k, n), np.float32)
        for j in range(n):
            idx = rng.choice(k, size=min(d, k), replace=False)
            w[idx, j] = scale * pm1(idx.size)
        return w
    ints = lambda lo, hi, n: rng.integers(lo, hi + 1, n).astype(np.float32)
    w = dict(w1=sparse(S, H1, 16), b1=ints(-2, 2, H1), w2=sparse(H1, H2, 2), b2=ints(-2, 2, H2), w3=pm1(H2, A), b3=ints(-3, 3, A),
             s_mean=ints(-3, 3, S), s_std=rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=S),
             a_mean=ints(-4, 4, A), a_std=rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=A), logstd=rng.uniform(-0.5, 0.5, A).astype(np.float32),
             goal_dim=G, gc_w=sparse(G, GC, 2), gc_b=ints(-1, 2, GC))
    for i, H in ((0, H1), (1, H2)):
        w.update({"g%d_w" % i: sparse(GC, GH, 2), "g%d_b" % i: ints(-1, 2, GH), "g%d_bias_w" % i: sparse(GH, H, 1), "g%d_bias_b" % i: ints(-2, 2, H),
                  "g%d_scale_w" % i: sparse(GH, H, 2, 128.0), "g%d_scale_b" % i: 128.0 * ints(-1, 1, H)})
    return w


def gated_actor_f64(w, cat, s_clip):
    """dm_policy.h GateDev: the gated actor in float64, nothing rounded but sigma (float64 2 / (1 + exp(-z)) rounded to fp32, as the issue of the exact
    check states it: exactly 0, 1 or 2 where z is 0 or of magnitude >= 128)"""
    f = lambda k: np.asarray(w[k], dtype=np.float64)
    x = (np.asarray(cat, np.float64) - f("s_mean")) / f("s_std")
    if s_clip > 0:
        x = np.clip(x, -s_clip, s_clip)
    out = dict(x=x)
    c = out["c"] = np.maximum(x[:, x.shape[1] - int(w["goal_dim"]):] @ f("gc_w") + f("gc_b"), 0.0)
    h = x
    for i, (wk, bk) in enumerate((("w1", "b1"), ("w2", "b2"))):
        e = out["e%d" % i] = np.maximum(c @ f("g%d_w" % i) + f("g%d_b" % i), 0.0)
        beta = out["beta%d" % i] = e @ f("g%d_bias_w" % i) + f("g%d_bias_b" % i)
        z = out["z%d" % i] = e @ f("g%d_scale_w" % i) + f("g%d_scale_b" % i)
        with np.errstate(over="ignore"):
            sigma = out["sigma%d" % i] = (2.0 / (1.0 + np.exp(-z))).astype(np.float32).astype(np.float64)
        h = out["h%d" % (i + 1)] = np.maximum(sigma * (h @ f(wk) + f(bk)) + beta, 0.0)
    out["m"] = h @ f("w3") + f("b3")
    out["a"] = out["m"] * f("a_std") + f("a_mean")
    return out


def check_gated_reference(ref, tag):
    """the precondition of the exact check, on the float64 reference alone"""
    for k in ("x", "c", "e0", "e1", "beta0", "beta1", "h1", "h2"):
        v = ref[k]
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 256, "%s: %s is not an integer of magnitude <= 256 everywhere (max %g)" % (tag, k, np.abs(v).max())
    for i in (0, 1):
        z = ref["z%d" % i]
        assert ((z == 0) | (np.abs(z) >= 128)).all(), tag
        assert set(np.unique(ref["sigma%d" % i])) == {0.0, 1.0, 2.0}, (tag, i, np.unique(ref["sigma%d" % i])[:8])
        assert (ref["h%d" % (i + 1)] != 0).mean() >= 0.01, (tag, i)
    assert np.array_equal(ref["m"], np.rint(ref["m"])) and np.abs(ref["m"]).max() < 2 ** 14, (tag, np.abs(ref["m"]).max())
    assert np.array_equal(ref["a"], ref["a"].astype(np.float32).astype(np.float64)), tag


def gsplit(row, cat):
    return (cat, None) if row.inside else (np.ascontiguousarray(cat[:, :row.S - row.G]), np.ascontiguousarray(cat[:, row.S - row.G:]))


def check_info(run, row, M=None):
    info = run.pol.info()
    has_stream = (row.H1, row.H2) == (1024, 512) and row.K1 <= 384 and row.N3 <= 64
    assert info["gated"] and info["goal_dim"] == row.G and info["fused"] == info["gated_fused"] == has_stream and (info["K1"], info["N3"]) == (row.K1, row.N3), info
    assert (info["path"], info["rows"]) == ((-1, 0) if M is None else (row.path, M)), info


def test_integer_generator_meets_the_precondition():
    """every ledger row, every batch size of the CPU and the GPU run, on the reference alone"""
    for name, row in GATED_PATHS.items():
        w = integer_gated_net(row, seed=sum(map(ord, name)))
        for M in ROWS_GPU:
            check_gated_reference(gated_actor_f64(w, integer_inputs(row, w, M, seed=M), S_CLIP), "%s/M=%d" % (name, M))


def check_row(name, lib, gpu, monkeypatch, counts, report=None):
    row = GATED_PATHS[name]
    set_env(monkeypatch, row.env)
    w = integer_gated_net(row, seed=sum(map(ord, name)))
    run = Runner(w, lib, gpu)
    check_info(run, row)
    for M in counts:
        tag = "%s/M=%d" % (name, M)
        cat = integer_inputs(row, w, M, seed=M)
        ref = gated_actor_f64(w, cat, S_CLIP)
        check_gated_reference(ref, tag)                     # before the kernel is looked at
        s, g = gsplit(row, cat)
        a, lp, fl = run(s, g)                               # (rows beyond M untouched: Runner's sentinels)
        check_info(run, row, M)
        bad = int((a.astype(np.float64) != ref["a"]).sum())
        if report is not None:
            report.append((tag, row.path, bad))
        assert bad == 0, "%s: %d of %d actions differ from float64, worst %g" % (tag, bad, a.size, np.abs(a - ref["a"]).max())
        assert np.allclose(lp, -w["logstd"].astype(np.float64).sum() - row.A * HALF_LOG_2PI, rtol=0, atol=1e-4), tag
        assert not fl.any(), tag
        if M in (1, 33, 4097):
            check_sampling(run, row, w, s, g, a, lp, ref, tag)
    run.close()


@pytest.mark.parametrize("name", sorted(GATED_PATHS))
def test_gated_row_exact_and_sampling_emulator(emu_lib, monkeypatch, name):
    check_row(name, emu_lib, False, monkeypatch, ROWS_EMU)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GATED_PATHS))
def test_gated_row_exact_and_sampling_gpu(hip_lib, monkeypatch, name):
    report = []
    try:
        check_row(name, hip_lib, True, monkeypatch, ROWS_GPU, report)
    finally:
        for tag, path, bad in report:
            print("GATED_ROW %s path %d exact %s" % (tag, path, "equal" if bad == 0 else "%d differ" % bad))


# ---------------------------------------------------------------------------------------------------------------------------------- random weights
def xavier_gated(row, seed=11, neutral=False):
    """test_policy.py make() (Xavier weights, non-zero biases, both normalisers) + Xavier gate layers with non-zero biases; neutral: the scale and bias
    projections zero, kernels and biases (sigma = 1, beta = 0 whatever the goal)"""
    from test_policy import make
    w = make(row.S, row.A, row.H1, row.H2, seed)
    g = random_weights(row.S, row.A, row.H1, row.H2, seed=seed + 100, gated_goal_dim=row.G)
    rng = np.random.default_rng(seed + 200)
    for k in GATE_KEYS:
        w[k] = g[k] if k.endswith("_w") else (0.1 * rng.normal(size=g[k].shape)).astype(np.float32)
        if neutral and ("_bias_" in k or "_scale_" in k):
            w[k] = np.zeros_like(g[k])
    w["goal_dim"] = row.G
    return w


def random_inputs(row, M):
    return (np.random.default_rng(2).normal(size=(M, row.S)) * 1.5 + 0.3).astype(np.float32)


PLAIN_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3", "s_mean", "s_std", "a_mean", "a_std", "logstd")


def check_neutral(name, lib, gpu, monkeypatch, M):
    """(b): fmaf(1, acc + b, 0) is acc + b, so the gated kernels must reproduce the plain ones bit for bit -- same products, same order, same rounding points"""
    row = GATED_PATHS[name]
    w = xavier_gated(row, neutral=True)
    cat = random_inputs(row, M)
    kw = dict(rate=0.5, sample=True, seed=3, step=5, env_id_offset=10)
    set_env(monkeypatch, row.env)
    run = Runner(w, lib, gpu, s_clip=10.0)
    got = run(*gsplit(row, cat), **kw)
    check_info(run, row, M)
    run.close()
    set_env(monkeypatch, row.env)                     # the plain actor dispatches alike: the same path id
    run = Runner({k: w[k] for k in PLAIN_KEYS}, lib, gpu, s_clip=10.0)
    want = run(*gsplit(row, cat), **kw)
    info = run.pol.info()
    assert info["path"] == row.path and not info["gated"], info
    run.close()
    for x, y, what in zip(got, want, ("actions", "logp", "exp_flags")):
        assert np.array_equal(x, y), (name, M, what, int((x != y).sum()))


@pytest.mark.parametrize("name", sorted(n for n, r in GATED_PATHS.items() if (r.H1, r.H2) == (1024, 512)))
def test_neutral_gate_is_the_plain_actor_emulator(emu_lib, monkeypatch, name):
    check_neutral(name, emu_lib, False, monkeypatch, 45)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n, r in GATED_PATHS.items() if (r.H1, r.H2) == (1024, 512)))
def test_neutral_gate_is_the_plain_actor_gpu(hip_lib, monkeypatch, name):
    for M in (45, 4097):
        check_neutral(name, hip_lib, True, monkeypatch, M)


def check_kinds_agree(lib, gpu, monkeypatch, name, M):
    """(c): what test_policy_kernels.py check_paths_agree holds the plain per-layer kernels to"""
    row = GATED_PATHS[name]
    w = xavier_gated(row)
    cat = random_inputs(row, M)
    run = Runner(w, lib, gpu, s_clip=5.0)
    kw = dict(rate=1.0, sample=True, seed=3, step=5, env_id_offset=10)
    out = {}
    for tag, env, path in (("fused", (), row.path), ("tile64", (LAYERED,), TILE64_TILE64), ("tile128", (LAYERED, TILE128), TILE128_TILE128),
                           ("wave", (LAYERED, ONE_WAVE), WAVE_WAVE)):
        set_env(monkeypatch, env)
        out[tag] = run(*gsplit(row, cat), **kw)
        assert run.pol.info()["path"] == path and run.pol.info()["gated"], (tag, run.pol.info())
    run.close()
    assert row.path < 16
    for tag in ("tile64", "tile128"):          # the per-layer kernels accumulate in the fused kernel's order: bit for bit (logp: the order of one A-term sum differs)
        assert np.array_equal(out["fused"][0], out[tag][0]), (tag, int((out["fused"][0] != out[tag][0]).sum()))
        assert np.abs(out["fused"][1] - out[tag][1]).max() < 1e-5 * max(1.0, np.abs(out[tag][1]).max()), tag
    assert np.abs(out["tile64"][0] - out["wave"][0]).max() < 1e-5
    assert np.array_equal(out["tile64"][2], out["wave"][2])


@pytest.mark.parametrize("name,M", [("hum_a36", 65), ("split", 33), ("dog", 33), ("hum_a28", 45)])
def test_gated_kernel_kinds_agree_emulator(emu_lib, monkeypatch, name, M):
    check_kinds_agree(emu_lib, False, monkeypatch, name, M)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hum_a36", "hum_a28", "split", "dog", "g1"])
def test_gated_kernel_kinds_agree_gpu(hip_lib, monkeypatch, name):
    for M in (65, 4096):
        check_kinds_agree(hip_lib, True, monkeypatch, name, M)


# (d) worst |a - ref_bf16| / max(1, |ref|max) with Xavier gates, measured with measure_random below over the ten ledger rows at 1024 / 512 (docs/HISTORY.md has every
# figure).  MI355X, M = 200 / 4096 / 4097: gated 2.5e-4 .. 1.43e-3 (worst: hum_a28 at M = 200; at 4096 / 4097 every row lies in 8.9e-4 .. 1.30e-3), the plain actor on
# the same main weights in the same run 3.5e-6 .. 1.05e-3.  Emulator, M = 37: gated 1.5e-7 .. 4.5e-4, plain 1.5e-7 .. 2.1e-4 -- a row is either at 1e-7 or at 1e-4, the
# size of one bf16 rounding of an activation going the other way, and the figure does not grow from 200 to 4097 rows.  Worst gated / worst plain = 1.4 (1.9 at 4096
# rows), inside the 4x that sigma <= 2 over two layers explains.  The bound is twice the worst gated measurement.
# Against the float64 statement the bf16 operands dominate (measured 3.1e-3 .. 6.0e-3): the plain actor's 2e-2.
MEASURED_GATED = 1.43e-3
RANDOM_BOUND = 2 * MEASURED_GATED


def measure_random(name, lib, gpu, monkeypatch, M):
    """(gated error, plain error on the same main weights, gated error against float64), each as |a - ref| / max(1, |ref|max)"""
    row = GATED_PATHS[name]
    w = xavier_gated(row)
    cat = random_inputs(row, M)
    set_env(monkeypatch, row.env)
    run = Runner(w, lib, gpu, s_clip=10.0)
    a, lp, _ = run(*gsplit(row, cat))
    check_info(run, row, M)
    run.close()
    want_bf, _ = reference_forward(w, cat, s_clip=10.0, bf16=True)
    want_64 = gated_actor_f64(w, cat, 10.0)["a"]
    wp = {k: w[k] for k in PLAIN_KEYS}
    set_env(monkeypatch, row.env)
    run = Runner(wp, lib, gpu, s_clip=10.0)
    ap, _, _ = run(*gsplit(row, cat))
    run.close()
    plain_bf, _ = reference_forward(wp, cat, s_clip=10.0, bf16=True)
    rel = lambda x, y: float(np.abs(x - y).max() / max(1.0, np.abs(y).max()))
    assert np.allclose(lp, -w["logstd"].sum() - row.A * HALF_LOG_2PI, atol=1e-4)
    return rel(a, want_bf), rel(ap, plain_bf), rel(a, want_64)


def check_random(name, lib, gpu, monkeypatch, counts):
    """every figure is printed before anything is asserted"""
    got = [(M,) + measure_random(name, lib, gpu, monkeypatch, M) for M in counts]
    for M, g, p, g64 in got:
        print("GATED_RANDOM %s M=%d gated %.3g plain %.3g gated vs float64 %.3g" % (name, M, g, p, g64))
    for M, g, p, g64 in got:
        assert g < RANDOM_BOUND, (name, M, g, p)
        assert g64 < 2e-2, (name, M, g64)


@pytest.mark.parametrize("name", sorted(n for n, r in GATED_PATHS.items() if (r.H1, r.H2) == (1024, 512)))
def test_gated_random_weights_emulator(emu_lib, monkeypatch, name):
    check_random(name, emu_lib, False, monkeypatch, (37,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n, r in GATED_PATHS.items() if (r.H1, r.H2) == (1024, 512)))
def test_gated_random_weights_gpu(hip_lib, monkeypatch, name):
    check_random(name, hip_lib, True, monkeypatch, (200, 4096, 4097))


# ---------------------------------------------------------------------------------------------------------------------------------- non-finite inputs
def check_nonfinite(name, lib, gpu, monkeypatch):
    """include/dm_hip.h dm_policy_params, per row: with a clip +-inf is clipped and NaN enters as -s_clip -- also in the goal, where it reaches every feature
    through the gate; without a clip the row's own output is unspecified.  Either way no other row changes by a bit."""
    row = GATED_PATHS[name]
    set_env(monkeypatch, row.env)
    w = integer_gated_net(row, seed=5)
    M = 45
    cat = integer_inputs(row, w, M, seed=3)
    poisoned = cat.copy()
    spots = [(3, 0, np.inf), (17, row.S - 1, -np.inf), (33, row.S // 2, np.nan), (44, row.S - 1, np.nan), (20, row.S - row.G, np.inf)]
    for r, c, v in spots:
        poisoned[r, c] = v
    hit = sorted({r for r, _, _ in spots}); clean = np.setdiff1d(np.arange(M), hit)
    as_clipped = cat.astype(np.float64)
    for r, c, v in spots:
        as_clipped[r, c] = w["s_mean"][c] + w["s_std"][c] * (S_CLIP if v == np.inf else -S_CLIP)
    ref = gated_actor_f64(w, as_clipped, S_CLIP)
    check_gated_reference(ref, name)
    run = Runner(w, lib, gpu)
    a, lp, _ = run(*gsplit(row, poisoned))
    check_info(run, row, M)
    assert np.array_equal(a.astype(np.float64), ref["a"]), np.argwhere(a != ref["a"])[:5]
    run.close()
    run = Runner(w, lib, gpu, s_clip=0.0)
    a_clean, lp_clean, _ = run(*gsplit(row, cat))
    a_p, lp_p, _ = run(*gsplit(row, poisoned))
    assert np.array_equal(a_p[clean], a_clean[clean]) and np.array_equal(lp_p[clean], lp_clean[clean])
    run.close()


NONFINITE_ROWS = ("hum_a36", "split", "dog", "inside", "lay_tile64", "lay_tile128", "lay_wave", "h64")


@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_gated_nonfinite_emulator(emu_lib, monkeypatch, name):
    check_nonfinite(name, emu_lib, False, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_gated_nonfinite_gpu(hip_lib, monkeypatch, name):
    check_nonfinite(name, hip_lib, True, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------- interface
def test_gated_create_and_forward_refusals(emu_lib):
    row = GATED_PATHS["hum_a36"]
    w = xavier_gated(row)
    for change, text in ((dict(goal_dim=0), "goal_dim"), (dict(goal_dim=row.S), "goal_dim")):
        with pytest.raises((RuntimeError, ValueError), match=text):
            bad = dict(w); bad.update(change); bad["gc_w"] = np.zeros((max(bad["goal_dim"], 1), GC), np.float32) if bad["goal_dim"] else np.zeros((0, GC), np.float32)
            Policy(bad, lib_path=emu_lib)
    bad = random_weights(row.S, row.A, seed=1, gated_goal_dim=3, gate_common=48)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        Policy(bad, lib_path=emu_lib)
    bad = dict(w); del bad["g1_scale_b"]
    with pytest.raises(ValueError, match="g1_scale_b"):
        Policy(bad, lib_path=emu_lib)
    pol = Policy(w, lib_path=emu_lib)
    s = np.zeros((4, row.S - 2), np.float32); g = np.zeros((4, 2), np.float32)
    with pytest.raises(RuntimeError, match="gated actor takes its goal"):
        pol.forward_host_ex(s, g)
    pol.close()


def test_reference_forward_plain_dict_is_unchanged_and_gate_matters():
    row = GATED_PATHS["hum_a36"]
    w = xavier_gated(row); cat = random_inputs(row, 9)
    plain = {k: w[k] for k in PLAIN_KEYS}
    neutral = xavier_gated(row, neutral=True)
    for bf in (False, True):
        a_plain = reference_forward(plain, cat, s_clip=10.0, bf16=bf)[0]
        assert np.array_equal(reference_forward(neutral, cat, s_clip=10.0, bf16=bf)[0], a_plain)
        assert np.abs(reference_forward(w, cat, s_clip=10.0, bf16=bf)[0] - a_plain).max() > 1e-3
    a32 = reference_forward(w, cat, s_clip=10.0)[0]
    assert np.abs(a32 - gated_actor_f64(w, cat, 10.0)["a"]).max() < 1e-4 * max(1.0, np.abs(a32).max())
