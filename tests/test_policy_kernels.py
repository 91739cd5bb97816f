"""Every policy kernel variant (deepmimic_amd/csrc/dm_policy.h) against an exact float64 statement of the actor, with the path that ran
reported by the library (dm_policy_info, include/dm_hip.h dm_policy_path).

POLICY_PATHS is the ledger: one row per (shape, environment switches) with the path id it must report.  Every row runs, on the emulator and
under `-m gpu` on the device through raw device pointers:

(a) exact: integer-valued networks (inputs, weights, biases and every activation are integers of magnitude <= 256, exact in bf16; layer-3 sums
    below 2^24, exact in fp32) make every product and every partial sum exact, so the result does not depend on the summation order, on the
    MFMA's internal order or on bf16 rounding: actions must equal the float64 reference BIT FOR BIT.  The precondition is asserted on the
    reference alone before the kernel is looked at.  Two instances per row: "w2" (w1 dense +-1, w2 sparse) and "w1" (w1 sparse, w2 dense +-1).
(b) sampling and the exploration coin against the Philox stream of deepmimic_amd/streams.py, bounds of tests/test_policy.py;
(c) at 1024 / 512 on random weights: fused == tiled (bit for bit), tiled == one-wave (1e-5, another summation order);
(d) on the GPU at 1024 / 512: the bounds of test_policy.py::test_policy_gpu_matches_reference on random weights at every ledger shape.
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np
import pytest

from deepmimic_amd import streams
from deepmimic_amd.policy import Policy, random_weights, reference_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/dm_hip.h dm_policy_path (test_ledger_matches_header holds the two equal)
FUSED_8_2, FUSED_8_4, FUSED_12_2, FUSED_12_4 = 0, 1, 2, 3
WAVE_WAVE, TILE64_WAVE, TILE128_WAVE, WAVE_TILE64, TILE64_TILE64, WAVE_TILE128, TILE128_TILE128 = 16, 17, 18, 20, 21, 24, 26
LAYERED, ONE_WAVE, TILE128 = ("DM_POLICY_LAYERED", "1"), ("DM_POLICY_ONE_WAVE", "1"), ("DM_POLICY_TILE", "128")
SWITCHES = ("DM_POLICY_LAYERED", "DM_POLICY_ONE_WAVE", "DM_POLICY_TILE")


@dataclass(frozen=True)
class Row:
    """S counts the G goal columns (dm_policy_forward_ex); env: the environment switches of the call; path: the id dm_policy_info must report;
    K1 / N3: the padded widths it must report"""
    S: int
    G: int
    A: int
    path: int
    K1: int
    N3: int
    H1: int = 1024
    H2: int = 512
    env: tuple = ()
    note: str = field(default="", compare=False)


POLICY_PATHS = {
    # one launch, k_policy_fused<8, 2>
    "f82_s197": Row(197, 0, 28, FUSED_8_2, 256, 32, note="the humanoid's observation width"),
    "f82_s256": Row(256, 0, 32, FUSED_8_2, 256, 32, note="no padded input column, no padded action column"),
    "f82_s100": Row(100, 0, 7, FUSED_8_2, 256, 32, note="K1 128 re-padded to 256"),
    "f82_s1": Row(1, 0, 1, FUSED_8_2, 256, 32, note="every padded column reads the clamped address S - 1"),
    # k_policy_fused<8, 4>
    "f84_a36": Row(197, 0, 36, FUSED_8_4, 256, 64, note="humanoid3d"),
    "f84_a33": Row(227, 0, 33, FUSED_8_4, 256, 64, note="one column in the second block"),
    "f84_a64": Row(130, 0, 64, FUSED_8_4, 256, 64, note="no padded action column"),
    # k_policy_fused<12, 2>
    "f122_s300": Row(300, 0, 28, FUSED_12_2, 384, 32, note="K1 320 re-padded to 384"),
    "f122_s384": Row(384, 0, 32, FUSED_12_2, 384, 32, note="no padded column at all"),
    # k_policy_fused<12, 4>
    "f124_dog": Row(347, 0, 58, FUSED_12_4, 384, 64, note="dog3d"),
    # goal block inside the fused kernel
    "goal_split": Row(300, 50, 28, FUSED_12_2, 384, 32, note="S - G = 250 < 256 < S: state columns in the first column pass, goal columns in both; 250 % 4 != 0"),
    "goal_g1": Row(227, 1, 36, FUSED_8_4, 256, 64, note="G = 1"),
    "goal_k256": Row(197, 10, 28, FUSED_8_2, 256, 32, note="S - G = 187, one column pass"),
    "goal_dog": Row(347, 91, 58, FUSED_12_4, 384, 64, note="S - G = 256 exactly: the second column pass is all goal"),
    # 1024 / 512 but not compiled as one launch
    "wide_s400": Row(400, 0, 28, TILE64_TILE64, 448, 32, note="K1 = 448: no fused stream"),
    "wide_a70": Row(227, 0, 70, TILE64_TILE64, 256, 96, note="N3 = 96: three column blocks in layer<2,1,2>, logp over all of them"),
    # per-layer kernels at 1024 / 512 by switch
    "lay_tile64": Row(227, 7, 36, TILE64_TILE64, 256, 64, env=(LAYERED,), note="gemm<0,64> gemm<1,64>, goal block through k_policy_prep"),
    "lay_tile128": Row(197, 0, 36, TILE128_TILE128, 256, 64, env=(LAYERED, TILE128), note="gemm<0,128> gemm<1,128>"),
    "lay_tile128_dog": Row(347, 0, 58, TILE128_TILE128, 384, 64, env=(LAYERED, TILE128)),
    "lay_wave": Row(197, 0, 36, WAVE_WAVE, 256, 64, env=(LAYERED, ONE_WAVE), note="layer<0,4,4> layer<1,2,4> at full width"),
    # one-wave by width
    "h192": Row(45, 0, 7, WAVE_WAVE, 64, 32, H1=192, H2=192, note="192 is no multiple of 128"),
    "h64": Row(40, 6, 5, WAVE_WAVE, 64, 32, H1=64, H2=64, note="KS = 2 in every layer"),
    # mixed, and the shortest k loops of k_policy_gemm (KS = 2: `if (2 < KS)` / `ks + 3 < KS`)
    "ks2_tile64": Row(50, 0, 9, TILE64_TILE64, 64, 32, H1=128, H2=128, note="gemm<0,64> with KS = 2"),
    "ks2_tile128": Row(64, 0, 9, TILE128_TILE128, 64, 32, H1=128, H2=128, env=(TILE128,), note="gemm<0,128> with KS = 2, S = K1"),
    "wave_tile64": Row(40, 0, 5, WAVE_TILE64, 64, 32, H1=64, H2=128, note="gemm<1,64> with KS = 2"),
    "wave_tile128": Row(40, 0, 5, WAVE_TILE128, 64, 32, H1=64, H2=128, env=(TILE128,), note="gemm<1,128> with KS = 2"),
    "tile64_wave": Row(70, 0, 33, TILE64_WAVE, 128, 64, H1=128, H2=192, note="gemm<0,64> with KS = 4, layer<1,2,4>"),
    "tile128_wave": Row(70, 0, 33, TILE128_WAVE, 128, 64, H1=128, H2=192, env=(TILE128,)),
}
# M = 1; one short of, exactly and one over a 32-row tile; 200 leaves a ragged 64- and a ragged 128-row block (and a ragged 16- and 32-row one)
ROWS_EMU = (1, 31, 32, 33, 200)
ROWS_GPU = ROWS_EMU + (4096, 4097)
PAD, SENTINEL, SENTINEL_I = 64, np.float32(-12345.5), -77
S_CLIP = 6.0
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)
# (b): 64-bit seed with a non-zero high word, env_id_offset > 0, and a step for which step * A wraps 32 bits for every A >= 1 ... 70 (0xF0000000 * A
# exceeds 2^32 from A = 2 on; A = 1 cannot wrap)
SEED, STEP, ENV_OFF = 0x9E3779B97F4A7C15, 0xF0000123, 1000


# ---------------------------------------------------------------------------------------------------------------------------------- the integer network
def w2_nonzeros(row):
    """"w2" instance: non-zeros per column of w2.  h2 is a sum of that many h1 values with random signs; h1 = relu(sum of S inputs of second moment
    ~1.5) has second moment ~0.75 S, and the largest of up to 4097 x 512 such sums would lie near 5.3 sigma if they were Gaussian, so
    5.3 sqrt(0.75 S d) <= 256 needs d <= 3100 / S.  The rows with many clipped inputs make the tail heavier than that (2400 / S still gave
    h2 up to 301 in the float64 reference): 1400 / S, at most 16.  The precondition in check_reference decides."""
    return int(min(16, row.H1, max(2, 1400 // row.S)))


def integer_net(row, instance, seed):
    rng = np.random.default_rng(seed)
    S, A, H1, H2 = row.S, row.A, row.H1, row.H2
    pm1 = lambda *sh: rng.choice(np.array([-1.0, 1.0], np.float32), size=sh)

    def sparse(k, n, d):
        w = np.zeros((k, n), np.float32)
        for j in range(n):
            idx = rng.choice(k, size=d, replace=False)
            w[idx, j] = pm1(d)
        return w
    if instance == "w2":
        w1 = pm1(S, H1); b1 = rng.integers(-2, 3, H1).astype(np.float32)
        w2 = sparse(H1, H2, w2_nonzeros(row))
    else:
        # few, small h1: one input per feature at H1 = 1024 (two gave h2 up to 268 in the float64 reference), two at the small widths, and b1 <= 0;
        # h2 is then a dense +-1 sum over all H1 of them
        w1 = sparse(S, H1, 1 if H1 >= 512 else min(S, 2)); b1 = -(rng.random(H1) < 0.1).astype(np.float32)
        w2 = pm1(H1, H2)
    w = dict(w1=w1, b1=b1, w2=w2, b2=rng.integers(-2, 3, H2).astype(np.float32), w3=pm1(H2, A), b3=rng.integers(-3, 4, A).astype(np.float32),
             s_mean=rng.integers(-3, 4, S).astype(np.float32), s_std=rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=S),
             a_mean=rng.integers(-4, 5, A).astype(np.float32), a_std=rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=A),
             logstd=rng.uniform(-0.5, 0.5, A).astype(np.float32))
    return w


def integer_inputs(row, w, M, seed):
    """s = s_mean + s_std * x with x mostly in {-1, 0, 1} and ~2 % of magnitude 5 .. 9 (the clip at 6 engages, exactly); fp32 holds s exactly"""
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 0.0, 1.0]), p=[0.4, 0.2, 0.4], size=(M, row.S))
    big = rng.random((M, row.S)) < (0.02 if row.S > 1 else 0.0)      # (S = 1: every feature sees the same input, a 6 there is a 6 in all 1024 of them)
    x[big] = (rng.integers(5, 10, size=int(big.sum())) * rng.choice([-1, 1], size=int(big.sum())))
    s = (w["s_mean"].astype(np.float64) + w["s_std"].astype(np.float64) * x).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), w["s_mean"] + w["s_std"].astype(np.float64) * x)
    return s


def actor_f64(w, cat, s_clip):
    """dm_policy.h header comment: a = unnormalize_a(W3 relu(W2 relu(W1 normalize_s(s) + b1) + b2) + b3), all in float64, nothing rounded"""
    f = lambda k: np.asarray(w[k], dtype=np.float64)
    x = (np.asarray(cat, np.float64) - f("s_mean")) / f("s_std")
    if s_clip > 0:
        x = np.clip(x, -s_clip, s_clip)
    h1 = np.maximum(x @ f("w1") + f("b1"), 0.0)
    h2 = np.maximum(h1 @ f("w2") + f("b2"), 0.0)
    m = h2 @ f("w3") + f("b3")
    return dict(x=x, h1=h1, h2=h2, m=m, a=m * f("a_std") + f("a_mean"))


def check_reference(ref, tag):
    """the precondition of the exact check, on the float64 reference alone, for every element"""
    for k in ("x", "h1", "h2"):
        v = ref[k]
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 256, "%s: %s is not an integer of magnitude <= 256 everywhere (max %g)" % (tag, k, np.abs(v).max())
    assert np.array_equal(ref["m"], np.rint(ref["m"])) and np.abs(ref["m"]).max() < 2 ** 24 - 8, (tag, np.abs(ref["m"]).max())
    assert np.array_equal(ref["a"], ref["a"].astype(np.float32).astype(np.float64)), tag
    if ref["x"].shape[0] >= 31:      # not degenerate (a single row of S = 1 has a handful of distinct values: judged on the larger batches)
        for k in ("h1", "h2"):
            pos = (ref[k] > 0).mean()
            assert 0.3 <= pos <= 0.7, "%s: %.0f %% of %s positive" % (tag, 100 * pos, k)
    assert np.abs(ref["x"]).max() == S_CLIP or ref["x"].size < 500 or ref["x"].shape[1] == 1, tag      # the clip engaged


# ---------------------------------------------------------------------------------------------------------------------------------- running a call
class Runner:
    """one Policy on one library; buffers carry PAD rows behind the M rows of the call, pre-filled with a sentinel that must survive"""

    def __init__(self, w, lib, gpu, s_clip=S_CLIP):
        self.gpu, self.A = gpu, w["w3"].shape[1]
        self.pol = Policy(w, lib_path=lib, s_clip=s_clip)

    def __call__(self, s, g=None, rate=1.0, sample=False, want_logp=True, want_flags=True, **kw):
        M, A = s.shape[0], self.A
        a = np.full((M + PAD, A), SENTINEL, np.float32); lp = np.full(M + PAD, SENTINEL, np.float32); fl = np.full(M + PAD, SENTINEL_I, np.int32)
        if self.gpu:
            import torch
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            ds, dg, da, dl, df = dev(s), (None if g is None else dev(g)), dev(a), dev(lp), dev(fl)
            torch.cuda.synchronize()
            ptr = lambda t: t.data_ptr()
        else:
            ds, dg, da, dl, df = np.ascontiguousarray(s), (None if g is None else np.ascontiguousarray(g)), a, lp, fl
            ptr = lambda t: t.ctypes.data
        self.pol.forward_device_ex(ptr(ds), M, ptr(da), 0 if dg is None else ptr(dg), 0 if dg is None else g.shape[1], ptr(dl) if want_logp else 0,
                                   ptr(df) if want_flags else 0, rate, sample, **kw)
        if self.gpu:
            torch.cuda.synchronize()
            a, lp, fl = da.cpu().numpy(), dl.cpu().numpy(), df.cpu().numpy()
        assert (a[M:] == SENTINEL).all() and (lp[M:] == SENTINEL).all() and (fl[M:] == SENTINEL_I).all(), "rows beyond M were written"
        if not want_logp:
            assert (lp == SENTINEL).all()
        if not want_flags:
            assert (fl == SENTINEL_I).all()
        return a[:M], lp[:M], fl[:M]

    def close(self):
        self.pol.close()


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def split(row, cat):
    """(state block, goal block or None) of concatenated inputs"""
    return (cat, None) if row.G == 0 else (np.ascontiguousarray(cat[:, :row.S - row.G]), np.ascontiguousarray(cat[:, row.S - row.G:]))


def noise_f64(seed, env_ids, step, A):
    """streams.normal_noise for a 64-bit seed (key = (seed_lo + env, seed_hi), counter (step * A + j mod 2^32, 0, 0, 0)) on the 24-bit uniforms the
    kernels document (dm_policy.h philox_normal), Box-Muller in float64"""
    env_ids = np.asarray(env_ids, dtype=np.int64); n = env_ids.size
    ctr = np.zeros((n, A, 4), np.uint32); ctr[..., 0] = ((int(step) * A + np.arange(A, dtype=np.int64)) & 0xFFFFFFFF)[None, :]
    key = np.zeros((n, A, 2), np.uint32); key[..., 0] = (((seed & 0xFFFFFFFF) + env_ids) & 0xFFFFFFFF)[:, None]; key[..., 1] = (seed >> 32) & 0xFFFFFFFF
    r = streams.philox4x32_10(ctr, key)
    u1 = ((r[..., 0] >> 8).astype(np.float64) + 0.5) / 16777216.0; u2 = ((r[..., 1] >> 8).astype(np.float64) + 0.5) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def coin_f64(seed, env_ids, step):
    from test_policy import _coin
    return _coin(seed, env_ids, step)


def test_noise_helper_is_the_streams_generator():
    """noise_f64 with the key streams.normal_noise uses is that function up to its 32- instead of 24-bit uniforms"""
    a = noise_f64(0xD33B, 5 + np.arange(40), 9, 7); b = streams.normal_noise(5 + np.arange(40), 9, 7, sigma=1.0)
    assert np.abs(a - b).max() < 1e-3
    assert (STEP * 2) >> 32 and (SEED >> 32)


# ---------------------------------------------------------------------------------------------------------------------------------- checks (a), (b)
def check_row(name, lib, gpu, monkeypatch, counts, report=None):
    row = POLICY_PATHS[name]
    set_env(monkeypatch, row.env)
    differing = 0
    for inst in ("w2", "w1"):
        w = integer_net(row, inst, seed=sum(map(ord, name)))
        run = Runner(w, lib, gpu)
        info = run.pol.info()
        assert info["path"] == -1 and (info["K1"], info["N3"]) == (row.K1, row.N3), info
        assert info["fused"] == (row.H1 == 1024 and row.H2 == 512 and row.K1 <= 384 and row.N3 <= 64)
        for M in counts:
            tag = "%s/%s/M=%d" % (name, inst, M)
            cat = integer_inputs(row, w, M, seed=M)
            ref = actor_f64(w, cat, S_CLIP)
            check_reference(ref, tag)                     # before the kernel is looked at
            s, g = split(row, cat)
            a, lp, fl = run(s, g)
            info = run.pol.info()
            assert info["path"] == row.path and info["rows"] == M, (tag, info)
            bad = int((a.astype(np.float64) != ref["a"]).sum())
            differing += bad
            if report is not None:
                report.append((tag, info["path"], bad))
            assert np.array_equal(a.astype(np.float64), ref["a"]), "%s: %d of %d actions differ from float64, worst %g" % (
                tag, bad, a.size, np.abs(a - ref["a"]).max())
            assert np.allclose(lp, -w["logstd"].astype(np.float64).sum() - row.A * HALF_LOG_2PI, rtol=0, atol=1e-4), tag
            assert not fl.any(), tag
            if M in (1, 33, 200, 4097):
                check_sampling(run, row, w, s, g, a, lp, ref, tag)
        run.close()
    return differing


def check_sampling(run, row, w, s, g, a_mode, lp_mode, ref, tag):
    """(b): with the integer network a_sampled - a_mode = exp(logstd) z a_std up to the fp32 rounding of the head's two adds.  With |mean| < 2^14
    (asserted on the reference) the first add rounds by at most half an ulp = 2^-11, the second (after the exact scaling by a power of two, one
    binade up at worst) by a_std 2^-10; divided by exp(logstd) a_std >= 0.6 a_std that is below 2.5e-3 in z: inside the 5e-3 of test_policy.py"""
    M, A = a_mode.shape
    assert np.abs(ref["m"]).max() < 2 ** 14, (tag, np.abs(ref["m"]).max())
    kw = dict(seed=SEED, step=STEP, env_id_offset=ENV_OFF)
    ids = ENV_OFF + np.arange(M)
    z_want = noise_f64(SEED, ids, STEP, A)
    coin = coin_f64(SEED, ids, STEP)
    a_all, lp_all, fl_all = run(s, g, 1.0, True, **kw)
    assert fl_all.all(), tag
    z = (a_all.astype(np.float64) - a_mode) / (np.exp(w["logstd"].astype(np.float64)) * w["a_std"])
    assert np.abs(z - z_want).max() < 5e-3, (tag, np.abs(z - z_want).max())
    lp_want = (-0.5 * z_want ** 2 - w["logstd"]).sum(1) - A * HALF_LOG_2PI
    assert np.abs(lp_all - lp_want).max() < 2e-2 * max(1.0, np.abs(lp_want).max() / 10), (tag, np.abs(lp_all - lp_want).max())
    a_mix, lp_mix, fl_mix = run(s, g, 0.3, True, **kw)
    ex = coin < 0.3
    assert np.array_equal(fl_mix != 0, ex) and set(np.unique(fl_mix)) <= {0, 1}, tag
    assert np.array_equal(a_mix[ex], a_all[ex]) and np.array_equal(lp_mix[ex], lp_all[ex]), tag
    assert np.array_equal(a_mix[~ex], a_mode[~ex]) and np.array_equal(lp_mix[~ex], lp_mode[~ex]), tag
    a0, lp0, fl0 = run(s, g, 0.0, True, **kw)
    assert np.array_equal(a0, a_mode) and np.array_equal(lp0, lp_mode) and not fl0.any(), tag
    # null logp / exp_flags: no fault, same actions
    a_n, _, _ = run(s, g, 0.3, True, want_logp=False, want_flags=False, **kw)
    assert np.array_equal(a_n, a_mix), tag
    a_n, _, fl_n = run(s, g, 0.3, True, want_logp=False, **kw)
    assert np.array_equal(a_n, a_mix) and np.array_equal(fl_n, fl_mix), tag


# ---------------------------------------------------------------------------------------------------------------------------------- ledger (CPU)
def header_paths():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"enum dm_policy_path \{(.*?)\};", src, re.S).group(1)
    return {n: int(v) for n, v in re.findall(r"DM_POLICY_PATH_(\w+) = (-?\d+)", body)}


def test_ledger_matches_header():
    """every path id the header declares has a row; a kernel choice added to the dispatcher fails here until it has one"""
    ids = header_paths()
    assert ids.pop("NONE") == -1
    mine = dict(FUSED_8_2=FUSED_8_2, FUSED_8_4=FUSED_8_4, FUSED_12_2=FUSED_12_2, FUSED_12_4=FUSED_12_4, WAVE_WAVE=WAVE_WAVE, TILE64_WAVE=TILE64_WAVE,
                TILE128_WAVE=TILE128_WAVE, WAVE_TILE64=WAVE_TILE64, TILE64_TILE64=TILE64_TILE64, WAVE_TILE128=WAVE_TILE128, TILE128_TILE128=TILE128_TILE128)
    assert ids == mine
    # DM_POLICY_PATH_LAYERED(l1, l2) = 16 + l1 + 4 l2 with one-wave 0, 64-row tile 1, 128-row tile 2; both tiled layers share the tile height
    kinds = dict(WAVE=0, TILE64=1, TILE128=2)
    for n, v in ids.items():
        if not n.startswith("FUSED"):
            l1, l2 = n.split("_")
            assert v == 16 + kinds[l1] + 4 * kinds[l2], n
    covered = {r.path for r in POLICY_PATHS.values()}
    assert covered == set(ids.values()), sorted(set(ids.values()) ^ covered)
    host = open(os.path.join(ROOT, "deepmimic_amd", "csrc", "dm_policy_host.h")).read()
    assert host.count("policy_path(d)") == 1 and len(re.findall(r"getenv\(\"DM_POLICY_(LAYERED|ONE_WAVE|TILE)\"\)", host)) == 3      # one dispatcher
    for name, r in POLICY_PATHS.items():
        assert 0 <= r.G < r.S and r.K1 % 64 == 0 and r.K1 >= r.S and r.N3 % 32 == 0 and r.N3 >= r.A, name
    # the shapes the kernels' edges need (module docstring of dm_policy.h, dm_policy_host.h dm_policy_create)
    rows = POLICY_PATHS.values()
    assert any(r.path == FUSED_12_2 and 257 <= r.S <= 320 for r in rows) and any(r.path == FUSED_8_2 and r.S <= 192 for r in rows)
    assert any(r.path < 16 and r.G and r.S - r.G < 256 < r.S and (r.S - r.G) % 4 for r in rows) and any(r.G == 1 for r in rows)
    assert any(r.N3 == 96 for r in rows) and any(r.K1 == 448 for r in rows) and any(r.S == 1 for r in rows)
    assert any(r.K1 == 64 and r.H1 % 128 == 0 for r in rows) and any(r.H1 == 64 for r in rows)


@pytest.mark.parametrize("name", sorted(POLICY_PATHS))
def test_row_exact_and_sampling_emulator(emu_lib, monkeypatch, name):
    check_row(name, emu_lib, False, monkeypatch, ROWS_EMU)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POLICY_PATHS))
def test_row_exact_and_sampling_gpu(hip_lib, monkeypatch, name):
    report = []
    try:
        check_row(name, hip_lib, True, monkeypatch, ROWS_GPU, report)
    finally:
        for tag, path, bad in report:
            print("POLICY_ROW %s path %d exact %s" % (tag, path, "equal" if bad == 0 else "%d differ" % bad))


# ---------------------------------------------------------------------------------------------------------------------------------- non-finite observations
def check_nonfinite(name, lib, gpu, monkeypatch):
    """What the actor returns for a non-finite observation (include/dm_hip.h dm_policy_params): with a clip, +-inf is clipped like any large value and
    NaN becomes -s_clip (fmaxf / fminf return their other operand); without one the row's own output is unspecified.  Either way no other row of
    the tile changes by a bit."""
    row = POLICY_PATHS[name]
    set_env(monkeypatch, row.env)
    w = integer_net(row, "w2", seed=5)
    M = 45
    cat = integer_inputs(row, w, M, seed=3)
    poisoned = cat.copy()
    spots = [(3, 0, np.inf), (17, row.S - 1, -np.inf), (33, row.S // 2, np.nan), (44, row.S - 1, np.nan)]
    for r, c, v in spots:
        poisoned[r, c] = v
    hit = sorted({r for r, _, _ in spots}); clean = np.setdiff1d(np.arange(M), hit)
    # clipped: equal to the float64 statement with the clipped value in place, bit for bit
    as_clipped = cat.astype(np.float64)
    for r, c, v in spots:
        as_clipped[r, c] = w["s_mean"][c] + w["s_std"][c] * (S_CLIP if v == np.inf else -S_CLIP)
    ref = actor_f64(w, as_clipped, S_CLIP)
    check_reference(ref, name)
    run = Runner(w, lib, gpu)
    a, lp, _ = run(*split(row, poisoned))
    assert run.pol.info()["path"] == row.path
    assert np.array_equal(a.astype(np.float64), ref["a"]), np.argwhere(a != ref["a"])[:5]
    run.close()
    # no clip: the other rows are those of the clean batch
    run = Runner(w, lib, gpu, s_clip=0.0)
    a_clean, lp_clean, _ = run(*split(row, cat))
    a_p, lp_p, _ = run(*split(row, poisoned))
    assert np.array_equal(a_p[clean], a_clean[clean]) and np.array_equal(lp_p[clean], lp_clean[clean])
    run.close()


NONFINITE_ROWS = ("f82_s197", "goal_split", "f124_dog", "lay_tile64", "lay_wave", "h64")


@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_nonfinite_observations_emulator(emu_lib, monkeypatch, name):
    check_nonfinite(name, emu_lib, False, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_nonfinite_observations_gpu(hip_lib, monkeypatch, name):
    check_nonfinite(name, hip_lib, True, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------- (c) paths agree
def xavier_net(S, A, H1=1024, H2=512, seed=1):
    """random Xavier weights with non-zero biases and an observation normaliser"""
    w = random_weights(S, A, H1, H2, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for k, d in (("b1", H1), ("b2", H2), ("b3", A)):
        w[k] = (0.1 * rng.normal(size=d)).astype(np.float32)
    w["s_mean"] = rng.normal(size=S).astype(np.float32); w["s_std"] = (1 + rng.random(S)).astype(np.float32)
    return w


def check_paths_agree(lib, gpu, monkeypatch, S, A, M):
    w = xavier_net(S, A)
    x = (2 * np.random.default_rng(2).normal(size=(M, S))).astype(np.float32)
    run = Runner(w, lib, gpu, s_clip=5.0)
    kw = dict(rate=1.0, sample=True, seed=3, step=5, env_id_offset=10)
    out = {}
    for tag, env, path in (("fused", (), FUSED_8_2 if S <= 256 else FUSED_12_4), ("tile64", (LAYERED,), TILE64_TILE64),
                           ("tile128", (LAYERED, TILE128), TILE128_TILE128), ("wave", (LAYERED, ONE_WAVE), WAVE_WAVE)):
        set_env(monkeypatch, env)
        out[tag] = run(x, None, **kw)
        assert run.pol.info()["path"] == path, (tag, run.pol.info())
    run.close()
    res = {}
    for tag in ("tile64", "tile128", "wave"):
        res[tag] = (int((out["fused"][0] != out[tag][0]).sum()), float(np.abs(out["fused"][0] - out[tag][0]).max()))
    print("POLICY_PATHS_AGREE S=%d A=%d M=%d differing elements / max |diff| against fused: %s" % (S, A, M, res))
    # the per-layer default accumulates in the fused kernel's order: bit for bit (log-probabilities: the order of one A-term sum differs)
    for tag in ("tile64", "tile128"):
        assert np.array_equal(out["fused"][0], out[tag][0]), (tag, res[tag])
        assert np.abs(out["fused"][1] - out[tag][1]).max() < 1e-5 * max(1.0, np.abs(out[tag][1]).max()), tag
    assert np.abs(out["tile64"][0] - out["wave"][0]).max() < 1e-5        # test_policy_emulator_tiled_gemm_and_one_wave_kernels_agree's bound
    assert np.array_equal(out["fused"][2], out["wave"][2])


@pytest.mark.parametrize("M", [33, 65])
@pytest.mark.parametrize("S,A", [(227, 28), (347, 58)])
def test_paths_agree_emulator(emu_lib, monkeypatch, S, A, M):
    check_paths_agree(emu_lib, False, monkeypatch, S, A, M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [33, 65, 4096])
@pytest.mark.parametrize("S,A", [(227, 28), (347, 58)])
def test_paths_agree_gpu(hip_lib, monkeypatch, S, A, M):
    check_paths_agree(hip_lib, True, monkeypatch, S, A, M)


# ---------------------------------------------------------------------------------------------------------------------------------- (d) random weights
def random_case(row, M, seed=11):
    """test_policy.py make(): Xavier weights, non-zero biases, both normalisers; inputs as test_policy_gpu_matches_reference draws them"""
    from test_policy import make
    w = make(row.S, row.A, row.H1, row.H2, seed)
    cat = (np.random.default_rng(2).normal(size=(M, row.S)) * 1.5 + 0.3).astype(np.float32)
    return w, cat


def check_random(name, lib, gpu, monkeypatch, M):
    row = POLICY_PATHS[name]
    set_env(monkeypatch, row.env)
    w, cat = random_case(row, M)
    run = Runner(w, lib, gpu, s_clip=10.0)
    a, lp, _ = run(*split(row, cat))
    assert run.pol.info()["path"] == row.path
    run.close()
    want_bf, _ = reference_forward(w, cat, s_clip=10.0, bf16=True)
    want_32, _ = reference_forward(w, cat, s_clip=10.0, bf16=False)
    want_64 = actor_f64(w, cat, 10.0)["a"]
    scale = np.abs(want_32).max()
    assert np.abs(a - want_bf).max() < 2e-3 * scale, (name, np.abs(a - want_bf).max(), scale)
    assert np.abs(a - want_32).max() < 2e-2 * scale, (name, np.abs(a - want_32).max(), scale)
    assert np.abs(a - want_64).max() < 2e-2 * scale, (name, np.abs(a - want_64).max(), scale)
    assert np.allclose(lp, -w["logstd"].sum() - row.A * HALF_LOG_2PI, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n, r in POLICY_PATHS.items() if (r.H1, r.H2) == (1024, 512)))
def test_row_random_weights_gpu(hip_lib, monkeypatch, name):
    for M in (200, 4097):
        check_random(name, hip_lib, True, monkeypatch, M)


def test_row_random_weights_emulator(emu_lib, monkeypatch):
    """the same statement on the emulator at the two fused shapes no other CPU test runs: K1 = 384 and a goal block, ragged tile"""
    for name in ("f122_s300", "goal_dog"):
        check_random(name, emu_lib, False, monkeypatch, 37)
