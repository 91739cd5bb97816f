"""AMP batch rewards, reward statistics, running value bounds and the value clip on the device (deepmimic_amd/csrc/dm_amp_rewards.h, include/dm_hip.h
dm_amp_batch_rewards / dm_amp_value_clip, deepmimic_amd/amp_rewards.py).  Every case runs on the emulator through host addresses (torch CPU tensors) and, marked
`gpu`, on the device through torch tensors.

Shapes: T in {1, 5, 7} x N in {3, 64, 65} (one partial wave, one full, one full + one lane) with the flag columns of tests/golden/td_returns.npz (no done, done at
0, done at T - 1, consecutive dones, an invalid episode in the middle and one running into t = 0, random), and (2, 16385): 257 group partials, the smallest N at
which a thread of the 256-thread fold owns two of them, so that the fold's run loop executes.

(1) mask: bit-equal to dm_td_lambda_returns' mask_out on the same flags -- the library against itself -- and to the mirror;
(2) rewards: bit-equal to the mirror; bit-equal to Discriminator.eval_* `out` for the same rows and task reward (S = 8, 64 / 64 hidden -- the narrowest net dm_policy_create takes --, 15 rows); logits at the
    reward's kinks, around them, +-inf and NaN;
(3) statistics and bounds: bit-equal to the mirror; against np.mean / np.std / np.amin / np.amax in float64 within derived bounds (below); determinism; a second
    call moves the bounds outwards only; the initial {+inf, -inf};
(4) exclusion: an invalid episode's rows reach nothing; one NaN in a counted row makes the bounds NaN and nothing else; n = 0;
(5) clip: against the mirror, heads.reference_value and a Critic(lo, hi) rebuilt from the host copy of the bounds; critic_returns_torch(bounds=...);
(6) refusals by name on sentinel-filled outputs;
(7) all_reduce_reward_bounds on two gloo ranks.

The float64 bounds of (3), with u = 2^-53, n counted rows, exact mean m and exact population standard deviation sd:
  mean: a sum of n terms in ANY order is within (n - 1) u sum|s| of the exact sum (to first order; the kernel's longest chain of additions is far shorter than
        n - 1), the division rounds once: |mean - m| <= dm := (n - 1) u sum|s| / n + u |m|.
  std:  the kernel forms d_i = fl(s_i - mean) = (s_i - m) + e_i with |e_i| <= dm + u |d_i|.  By Minkowski's inequality the root mean square of (s_i - m) + e_i
        is within RMS(e) <= dm + u sd of sd, so the mean's error enters linearly, not divided by sd.  Each square rounds once (relative u), the sum of n of
        them in any order adds (n - 1) u, the division u: relative (n + 1) u on the quotient, half of it on the square root, which rounds once more:
        |std - sd| <= dm + u sd + ((n + 1) / 2 + 1) u sd  <=  dm + (n / 2 + 4) u sd.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from deepmimic_amd import amp_rewards as ar
from deepmimic_amd import heads, returns
from deepmimic_amd.core import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "td_returns.npz")
BASE = [(T, N) for T in (1, 5, 7) for N in (3, 64, 65)]
RUN_LOOP = (2, 16385)                   # ceil(16385 / 64) = 257 partials > 256 folding threads: per = 2
SHAPES = BASE + [RUN_LOOP]
U = 2.0 ** -53
F32 = np.float32
_gold, _cases = None, {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def flags(T, N):
    """done, valid, terminate [T, N] int32: the fixture's columns at the base shapes, random ones (about one done in 3, one invalid in 4) at the others"""
    global _gold
    if (T, N) in BASE:
        if _gold is None:
            _gold = dict(np.load(GOLD))
        return tuple(np.ascontiguousarray(_gold["T%d_N%d/%s" % (T, N, k)]) for k in ("done", "valid", "terminate"))
    rng = np.random.default_rng(1000 * T + N)
    done = (rng.random((T, N)) < 0.34).astype(np.int32)
    valid = np.where(done != 0, (rng.random((T, N)) >= 0.25), 1).astype(np.int32)
    return done, valid, np.zeros((T, N), np.int32)


def case(T, N):
    """one seeded rollout per shape, shared by the tests (never modified): logits around the reward's support [-1, 3], task rewards in [0, 1)"""
    if (T, N) not in _cases:
        rng = np.random.default_rng(7 * T + N)
        done, valid, terminate = flags(T, N)
        logits = (1.0 + 1.6 * rng.standard_normal((T, N))).astype(F32)
        task = rng.random((T, N)).astype(F32)
        for a in (done, valid, terminate, logits, task):
            a.setflags(write=False)
        _cases[(T, N)] = dict(logits=logits, task=task, done=done, valid=valid, terminate=terminate)
    return _cases[(T, N)]


# ---------------------------------------------------------------------------------------------------------------------------------- running a call
def dev_tensor(a, gpu):
    import torch
    t = torch.from_numpy(np.array(a))          # (a copy: the shared cases are read-only)
    return t.cuda() if gpu else t


def tracker(lib, gpu, **kw):
    return ar.AmpRewards("cuda:0" if gpu else "cpu", lib_path=lib, **kw)


def update(trk, gpu, logits, task=None, done=None, valid=None):
    """AmpRewards.update_torch on host arrays; everything comes back as host arrays"""
    args = [None if a is None else dev_tensor(a, gpu) for a in (logits, task, done, valid)]
    r, m = trk.update_torch(*args)
    return dict(rewards=r.cpu().numpy(), mask=m.cpu().numpy(), stats=trk.stats.cpu().numpy().copy(), bounds=trk.bounds.cpu().numpy().copy())


def library_mask(lib, gpu, c):
    """mask_out of dm_td_lambda_returns on the case's flags (rewards and values do not enter it)"""
    T, N = c["done"].shape
    z = np.zeros((T + 1, N), F32)
    if gpu:
        t = lambda a: dev_tensor(a, True)
        return returns.td_lambda_returns_torch(t(z[:T]), t(z), t(z[:T]), t(c["terminate"]), t(c["done"]), t(c["valid"]), 0.95, 0.95, 0.0, 1.0, lib_path=lib)[1].cpu().numpy()
    ret, mask = np.zeros((T, N), F32), np.full((T, N), -1, np.int32)
    returns.td_lambda_returns(T, N, z.ctypes.data, z.ctypes.data, z.ctypes.data, c["terminate"].ctypes.data, c["done"].ctypes.data, c["valid"].ctypes.data,
                              0.95, 0.95, 0.0, 1.0, ret.ctypes.data, mask.ctypes.data, lib_path=lib)
    return mask


# ---------------------------------------------------------------------------------------------------------------------------------- (1) - (3) per shape
def check_shape(lib, gpu, T, N):
    c = case(T, N)
    scale, lerp = 2.0, 0.3
    # (1) the mask: the library against itself, and the mirror
    lm = library_mask(lib, gpu, c)
    assert same_bits(lm, ar.reference_mask(c["done"], c["valid"]))
    if (T, N) in BASE and T >= 5 and N > 6:
        assert (lm == 0).any() and (lm[:, 0] == 1).all()
    for task in (c["task"], None):
        trk = tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp)
        got = update(trk, gpu, c["logits"], task, c["done"], c["valid"])
        want = ar.reference_batch_rewards(c["logits"], task, c["done"], c["valid"], scale, lerp)
        assert same_bits(got["mask"], lm)
        # (2) the rewards
        assert same_bits(got["rewards"], want["rewards"]), np.abs(got["rewards"] - want["rewards"]).max()
        # (3) statistics and bounds: the mirror, bit for bit
        print("T=%d N=%d task=%s stats got %r mirror %r bounds %r" % (T, N, task is not None, got["stats"].tolist(), want["stats"].tolist(), got["bounds"].tolist()))
        assert same_bits(got["stats"], want["stats"]) and same_bits(got["bounds"], want["bounds"])
        # ... and plain numpy in float64 on the counted rows
        counted = lm != 0
        n = int(counted.sum())
        assert got["stats"][ar.STAT_N] == n and n > 0
        s64, r_c = want["style"][counted].astype(np.float64), want["rewards"][counted]
        m, sd = np.mean(s64), np.std(s64)
        dm = (n - 1) * U * np.abs(s64).sum() / n + U * abs(m)
        print("    n=%d |mean - np.mean|=%.3e (bound %.3e) |std - np.std|=%.3e (bound %.3e)" % (n, abs(got["stats"][ar.STAT_MEAN] - m), dm, abs(got["stats"][ar.STAT_STD] - sd),
                                                                                              dm + (n / 2 + 4) * U * sd))
        assert abs(got["stats"][ar.STAT_MEAN] - m) <= dm
        assert abs(got["stats"][ar.STAT_STD] - sd) <= dm + (n / 2 + 4) * U * sd
        assert got["stats"][ar.STAT_MIN] == np.amin(r_c) and got["stats"][ar.STAT_MAX] == np.amax(r_c)
        assert got["bounds"][0] == np.amin(r_c) and got["bounds"][1] == np.amax(r_c)          # from the initial {+inf, -inf}
        assert sd > 0 and got["bounds"][0] < got["bounds"][1]
        # two calls on one input: the same bytes (the bounds do not move: min(b, b) = b)
        again = update(trk, gpu, c["logits"], task, c["done"], c["valid"])
        assert all(same_bits(again[k], got[k]) for k in ("rewards", "mask", "stats", "bounds"))
    # without `valid` every row counts, and `done` is not needed
    trk = tracker(lib, gpu, reward_scale=scale)
    got = update(trk, gpu, c["logits"])
    want = ar.reference_batch_rewards(c["logits"], reward_scale=scale)
    assert (got["mask"] == 1).all() and got["stats"][ar.STAT_N] == T * N
    assert same_bits(got["rewards"], want["rewards"]) and same_bits(got["stats"], want["stats"]) and same_bits(got["bounds"], want["bounds"])


@pytest.mark.parametrize("T,N", SHAPES)
def test_rewards_mask_statistics_and_bounds_emulator(emu_lib, T, N):
    check_shape(emu_lib, False, T, N)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_rewards_mask_statistics_and_bounds_gpu(hip_lib, T, N):
    check_shape(hip_lib, True, T, N)


def test_the_run_loop_shape_gives_a_folding_thread_two_partials():
    groups = lambda N: (N + ar.SCAN - 1) // ar.SCAN
    per = lambda N: (groups(N) + ar.FOLD - 1) // ar.FOLD
    assert per(RUN_LOOP[1]) == 2 and per(RUN_LOOP[1] - 1) == 1


# ---------------------------------------------------------------------------------------------------------------------------------- (2) kinks and the head
def kink_logits():
    """15 rows: the kinks y = -1, 1, 3 of max(0, 1 - (1 - y)^2 / 4), the floats on both sides of each, +-inf, NaN, and an ordinary row"""
    ys = []
    for k in (-1.0, 1.0, 3.0):
        k = F32(k)
        ys += [np.nextafter(k, F32(-np.inf)), k, np.nextafter(k, F32(np.inf))]
    ys += [F32(np.inf), F32(-np.inf), F32(np.nan), F32(0.25), F32(-7.5), F32(1e30)]
    return np.array(ys, F32).reshape(3, 5)


def check_kinks(lib, gpu):
    y = kink_logits()
    task = np.linspace(-1.0, 2.5, 15).astype(F32).reshape(3, 5)
    scale, lerp = 2.0, 0.5
    for tk in (None, task):
        got = update(tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp), gpu, y, tk)
        want = ar.reference_batch_rewards(y, tk, reward_scale=scale, task_reward_lerp=lerp)
        assert same_bits(got["rewards"], want["rewards"]) and same_bits(got["stats"], want["stats"]) and same_bits(got["bounds"], want["bounds"])
        # the float64 statement of the head.  With u = 2^-24: d = fl(1 - y) is within u |d|, so d^2 / 4 within |d|^2 u / 2 <= 2 u where the reward is not clipped
        # to 0 on both sides (|d| <= 2; a float next to -1 or 3 may round onto the kink), the fmaf rounds once (u), scale = 2 and 1 - lerp = 1 / 2 are exact
        # factors, the blend's fmaf rounds once (u |r|): |r - ref| <= (3 scale + |r|) u <= 4 u (scale + |task_r|)
        ref = heads.reference_style_reward(y.astype(np.float64), scale, lerp if tk is not None else None, tk)
        near = np.isfinite(y) & (np.abs(y) < 4)
        assert (np.abs(got["rewards"].astype(np.float64) - ref)[near] <= 4 * 2.0 ** -24 * (scale + (0 if tk is None else np.abs(tk[near])))).all()
        s = want["style"].reshape(-1)                            # rows 0 .. 8: below, at and above -1, 1, 3
        assert s[1] == 0 and s[4] == scale and s[7] == 0 and s[0] == 0 and s[8] == 0 and (s >= 0).all() and (s <= scale).all()
        assert 0 < s[3] <= scale and 0 < s[5] <= scale and s[2] < 1e-6 and s[6] < 1e-6
        assert (s[[9, 10, 11, 13, 14]] == 0).all()               # +-inf, NaN (fmaxf drops it) and far outside: no style reward
        assert np.isfinite(got["rewards"]).all() and np.isfinite(got["stats"]).all()


def test_logits_at_the_kinks_emulator(emu_lib):
    check_kinks(emu_lib, False)


@pytest.mark.gpu
def test_logits_at_the_kinks_gpu(hip_lib):
    check_kinks(hip_lib, True)


def small_net(seed, scale=1.0):
    from deepmimic_amd.policy import random_weights
    w = random_weights(8, 1, 64, 64, seed=seed, init_output_scale=scale)          # (64 / 64: the narrowest hidden layers dm_policy_create takes)
    return {k: v for k, v in w.items() if k not in ("a_mean", "a_std", "logstd")}


def check_head(lib, gpu):
    """the pass on the discriminator's own logits == the discriminator's own reward, for the same rows and task reward: S = 8, 64 / 64 hidden (the one-wave
    per-layer route), 15 rows"""
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((3, 5, 8)).astype(F32)
    task = rng.random((3, 5)).astype(F32)
    for lerp, tk in ((0.3, task), (None, None)):
        disc = heads.Discriminator(small_net(3, scale=4.0), reward_scale=1.5, task_reward_lerp=lerp, lib_path=lib)
        trk = tracker(lib, gpu, reward_scale=1.5, task_reward_lerp=lerp)
        if gpu:
            kw = {} if tk is None else dict(task_reward=dev_tensor(tk, True))
            out, y = disc.eval_torch(dev_tensor(obs, True), raw=True, **kw)
            r, _ = trk.update_from_disc(disc, dev_tensor(obs, True), None if tk is None else dev_tensor(tk, True))
            out, y, r = out.cpu().numpy(), y.cpu().numpy(), r.cpu().numpy()
        else:
            out, y = disc.eval_host(obs.reshape(15, 8), **({} if tk is None else dict(task_reward=tk.reshape(15))))
            out, y = out.reshape(3, 5), y.reshape(3, 5)
            r = update(trk, False, y, tk)["rewards"]
        assert np.unique(y).size == 15 and ((out > 0) & (out < 1.5)).sum() >= 4, (y, out)          # not a constant head
        assert same_bits(r, out)
        disc.close()


def test_rewards_equal_the_style_head_emulator(emu_lib):
    check_head(emu_lib, False)


@pytest.mark.gpu
def test_rewards_equal_the_style_head_gpu(hip_lib):
    check_head(hip_lib, True)


# ---------------------------------------------------------------------------------------------------------------------------------- (3) running bounds
def check_running_bounds(lib, gpu):
    c = case(5, 65)
    trk = tracker(lib, gpu, reward_scale=1.0, task_reward_lerp=0.5)
    assert same_bits(trk.bounds.cpu().numpy(), np.array([np.inf, -np.inf], F32))
    a = update(trk, gpu, c["logits"], c["task"], c["done"], c["valid"])
    assert np.isfinite(a["bounds"]).all()
    # narrower rewards: the bounds stay; wider ones on one side: that bound alone moves
    b = update(trk, gpu, c["logits"], (0.5 * c["task"] + 0.25).astype(F32), c["done"], c["valid"])
    assert same_bits(b["bounds"], a["bounds"]) and b["stats"][ar.STAT_MIN] > a["bounds"][0] and b["stats"][ar.STAT_MAX] < a["bounds"][1]
    d = update(trk, gpu, c["logits"], (c["task"] + 3.0).astype(F32), c["done"], c["valid"])
    assert d["bounds"][0] == a["bounds"][0] and d["bounds"][1] > a["bounds"][1] and d["bounds"][1] == d["stats"][ar.STAT_MAX]
    e = update(trk, gpu, c["logits"], (c["task"] - 3.0).astype(F32), c["done"], c["valid"])
    assert e["bounds"][0] < a["bounds"][0] and e["bounds"][0] == e["stats"][ar.STAT_MIN] and e["bounds"][1] == d["bounds"][1]
    want = ar.reference_batch_rewards(c["logits"], (c["task"] - 3.0).astype(F32), c["done"], c["valid"], 1.0, 0.5, bounds=d["bounds"])
    assert same_bits(e["bounds"], want["bounds"]) and same_bits(e["stats"], want["stats"])
    st = trk.state_host()
    assert st["reward_min"] == e["bounds"][0] and st["reward_max"] == e["bounds"][1] and st["n"] == int(e["stats"][ar.STAT_N])
    assert st["disc_reward_mean"] == e["stats"][ar.STAT_MEAN] and st["disc_reward_std"] == e["stats"][ar.STAT_STD]
    assert a["stats"][ar.STAT_MEAN] == e["stats"][ar.STAT_MEAN] and a["stats"][ar.STAT_STD] == e["stats"][ar.STAT_STD]      # the style term: before the blend


def test_bounds_run_outwards_emulator(emu_lib):
    check_running_bounds(emu_lib, False)


@pytest.mark.gpu
def test_bounds_run_outwards_gpu(hip_lib):
    check_running_bounds(hip_lib, True)


# ---------------------------------------------------------------------------------------------------------------------------------- (4) exclusion
def check_exclusion(lib, gpu):
    T, N = 7, 65
    c = case(T, N)
    mask = ar.reference_mask(c["done"], c["valid"])
    col = 4                                                     # the fixture's "invalid in the middle": mask [1, 1, 0, 0, 1, 1, 1]
    assert mask[:, col].tolist() == [1, 1, 0, 0, 1, 1, 1]
    scale, lerp = 2.0, 0.3
    dirty = c["task"].copy()
    dirty[2, col], dirty[3, col] = np.nan, 3e38
    uncounted = (mask == 0)
    logits = c["logits"].copy()
    logits[uncounted & (np.arange(N)[None, :] != col)] = np.nan          # NaN logits in every other row that is not counted
    got = update(tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp), gpu, logits, dirty, c["done"], c["valid"])
    assert np.isnan(got["rewards"][2, col]) and got["rewards"][3, col] > 1e37          # rewards_out holds them
    # the run that sees the counted rows only (what is not counted replaced by ordinary values, so that the sums keep their order): the same bytes from the
    # device and from the mirror; and plain numpy on the counted rows
    clean_in = (np.where(uncounted, F32(1.0), logits), np.where(uncounted, F32(0.5), dirty))
    clean_run = update(tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp), gpu, clean_in[0], clean_in[1], c["done"], c["valid"])
    clean = ar.reference_batch_rewards(clean_in[0], clean_in[1], c["done"], c["valid"], scale, lerp)
    assert same_bits(got["stats"], clean_run["stats"]) and same_bits(got["bounds"], clean_run["bounds"]) and np.isfinite(clean_run["rewards"]).all()
    assert same_bits(got["stats"], clean["stats"]) and same_bits(got["bounds"], clean["bounds"])
    r_c = clean["rewards"][mask != 0]
    assert np.isfinite(got["stats"]).all() and got["bounds"][0] == np.amin(r_c) and got["bounds"][1] == np.amax(r_c) and got["stats"][ar.STAT_N] == (mask != 0).sum()
    # one NaN in a counted row: the bounds (and this call's min / max) are NaN, nothing else is
    one = c["task"].copy(); one[0, col] = np.nan
    trk = tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp)
    bad = update(trk, gpu, c["logits"], one, c["done"], c["valid"])
    good = ar.reference_batch_rewards(c["logits"], c["task"], c["done"], c["valid"], scale, lerp)
    assert np.isnan(bad["bounds"]).all() and np.isnan(bad["stats"][[ar.STAT_MIN, ar.STAT_MAX]]).all()
    assert same_bits(bad["stats"][:3], good["stats"][:3])
    assert np.isnan(bad["rewards"][0, col]) and np.isnan(bad["rewards"]).sum() == 1 and same_bits(bad["mask"], good["mask"])
    keep = np.ones((T, N), bool); keep[0, col] = False
    assert same_bits(bad["rewards"][keep], good["rewards"][keep])
    mirror = ar.reference_batch_rewards(c["logits"], one, c["done"], c["valid"], scale, lerp)
    assert np.isnan(mirror["bounds"]).all() and same_bits(mirror["stats"][:3], bad["stats"][:3])
    assert np.isnan(update(trk, gpu, c["logits"], c["task"], c["done"], c["valid"])["bounds"]).all()          # and stays visible
    # n = 0: every episode ends invalid at T - 1
    done = np.zeros((T, N), np.int32); done[T - 1] = 1
    valid = np.ones((T, N), np.int32); valid[T - 1] = 0
    trk = tracker(lib, gpu, reward_scale=scale, task_reward_lerp=lerp)
    for start in (np.array([np.inf, -np.inf], F32), np.array([-0.25, 1.75], F32)):
        trk.bounds.copy_(dev_tensor(start, gpu))
        z = update(trk, gpu, c["logits"], c["task"], done, valid)
        assert same_bits(z["bounds"], start) and (z["mask"] == 0).all()
        assert same_bits(z["stats"], np.array([0.0, 0.0, 0.0, np.inf, -np.inf]))
        assert same_bits(z["rewards"], good["rewards"])
        assert same_bits(ar.reference_batch_rewards(c["logits"], c["task"], done, valid, scale, lerp, bounds=start)["bounds"], start)


def test_uncounted_rows_reach_nothing_emulator(emu_lib):
    check_exclusion(emu_lib, False)


@pytest.mark.gpu
def test_uncounted_rows_reach_nothing_gpu(hip_lib):
    check_exclusion(hip_lib, True)


# ---------------------------------------------------------------------------------------------------------------------------------- (5) the clip
def clip_values(lo, hi):
    """hand-built rows on both sides of lo and hi, at them, next to them, +-inf and NaN; 67 rows: more than one wavefront"""
    nx = lambda x, d: np.nextafter(F32(x), F32(d))
    v = [lo, hi, nx(lo, -np.inf), nx(lo, np.inf), nx(hi, -np.inf), nx(hi, np.inf), lo - 100, hi + 100, 0.5 * (lo + hi), np.inf, -np.inf, np.nan, 0.0, -0.0]
    rng = np.random.default_rng(2)
    return np.concatenate([np.array(v, F32), rng.uniform(lo - 5, hi + 5, 67 - len(v)).astype(F32)])


def check_clip(lib, gpu):
    discount = 0.95
    trk = tracker(lib, gpu, discount=discount)
    b = np.array([-0.3, 1.7], F32)
    trk.bounds.copy_(dev_tensor(b, gpu))
    lo, hi = ar.value_bounds(b, discount)
    assert lo == F32(float(b[0]) / (1 - discount)) and hi == F32(float(b[1]) / (1 - discount)) and lo < hi
    v = clip_values(lo, hi)
    rm = (np.arange(v.size) % 3 != 1).astype(np.int32)
    for row_mask, fill in ((None, 0.0), (rm, -9.5)):
        got = trk.clip_torch(dev_tensor(v, gpu), None if row_mask is None else dev_tensor(row_mask, gpu), fill).cpu().numpy()
        assert same_bits(got, ar.reference_value_clip(v, b, discount, row_mask, fill))
        ref = heads.reference_value(v.astype(np.float64), float(lo), float(hi), row_mask=row_mask, fill=fill).astype(F32)
        assert same_bits(got, ref)
        on = np.ones(v.size, bool) if row_mask is None else row_mask != 0
        for k, at in ((0, lo), (1, hi), (2, lo), (3, v[3]), (4, v[4]), (5, hi), (9, hi), (10, lo), (11, lo)):          # (a NaN value comes out as lo)
            assert got[k] == (at if on[k] else F32(fill)), k
        assert (got[on] >= lo).all() and (got[on] <= hi).all()
        assert (got[~on] == F32(fill)).all() and ((got[on] > lo) & (got[on] < hi)).sum() >= 8
    x = dev_tensor(v, gpu)                                      # in place
    assert trk.clip_torch(x, out=x) is x and same_bits(x.cpu().numpy(), ar.reference_value_clip(v, b, discount))
    # what a NaN bound and the initial bounds give, as the header says
    for bb in (np.array([np.nan, 1.7], F32), np.array([-0.3, np.nan], F32), np.array([np.nan, np.nan], F32), np.array([np.inf, -np.inf], F32)):
        trk.bounds.copy_(dev_tensor(bb, gpu))
        got = trk.clip_torch(dev_tensor(v, gpu)).cpu().numpy()
        assert same_bits(got, ar.reference_value_clip(v, bb, discount))
    assert (got == -np.inf).all()                               # {+inf, -inf}: fminf(fmaxf(v, +inf), -inf)


def test_value_clip_emulator(emu_lib):
    check_clip(emu_lib, False)


@pytest.mark.gpu
def test_value_clip_gpu(hip_lib):
    check_clip(hip_lib, True)


def critic_case():
    rng = np.random.default_rng(9)
    T, N = 5, 7
    obs = rng.standard_normal((T + 1, N, 8)).astype(F32); tobs = rng.standard_normal((T, N, 8)).astype(F32)
    done = (rng.random((T, N)) < 0.3).astype(np.int32); done[T - 1, 0] = 1
    terminate = np.where(done != 0, rng.integers(0, 3, (T, N)), 0).astype(np.int32)
    valid = np.where(done != 0, rng.random((T, N)) >= 0.2, 1).astype(np.int32)
    rewards = rng.random((T, N)).astype(F32)
    return T, N, obs, tobs, done, terminate, valid, rewards


def test_clip_equals_a_critic_rebuilt_from_the_bounds_emulator(emu_lib):
    T, N, obs, tobs, done, terminate, valid, rewards = critic_case()
    w = small_net(4, scale=8.0)
    b = np.array([-0.05, 0.06], F32)
    lo, hi = ar.value_bounds(b, 0.95)
    free, crit = heads.Critic(w, lib_path=emu_lib), heads.Critic(w, lo=float(lo), hi=float(hi), lib_path=emu_lib)
    trk = tracker(emu_lib, False, discount=0.95); trk.bounds.copy_(dev_tensor(b, False))
    y = free.eval_host(obs.reshape(-1, 8))[0]
    want = crit.eval_host(obs.reshape(-1, 8))[0]
    assert (want == lo).any() and (want == hi).any() and ((want > lo) & (want < hi)).any()
    assert same_bits(trk.clip_torch(dev_tensor(y, False)).numpy(), want)
    ty = free.eval_host(tobs.reshape(-1, 8), row_mask=done.reshape(-1), fill=0.0)[0]
    twant = crit.eval_host(tobs.reshape(-1, 8), row_mask=done.reshape(-1), fill=0.0)[0]
    assert same_bits(trk.clip_torch(dev_tensor(ty, False), dev_tensor(done.reshape(-1), False), 0.0).numpy(), twant)
    free.close(); crit.close()


@pytest.mark.gpu
def test_critic_returns_with_device_bounds_equal_the_rebuilt_critic_gpu(hip_lib):
    T, N, obs, tobs, done, terminate, valid, rewards = critic_case()
    w = small_net(4, scale=8.0)
    trk = tracker(hip_lib, True, reward_scale=1.0, task_reward_lerp=0.5, discount=0.95)
    trk.bounds.copy_(dev_tensor(np.array([-0.05, 0.06], F32), True))
    st = trk.state_host()                                       # the host copy a learner without the tracker would read every iteration
    free = heads.Critic(w, val_fail=-0.5, val_succ=2.0, lib_path=hip_lib)
    crit = heads.Critic(w, lo=st["reward_min"] / (1 - 0.95), hi=st["reward_max"] / (1 - 0.95), val_fail=-0.5, val_succ=2.0, lib_path=hip_lib)
    t = lambda a: dev_tensor(a, True)
    args = (t(obs), None, t(tobs), None, t(terminate), t(done), t(valid), t(rewards), 0.95, 0.9)
    ret, mask, values = returns.critic_returns_torch(free, *args, lib_path=hip_lib, return_values=True, bounds=trk)
    wret, wmask, wvalues = returns.critic_returns_torch(crit, *args, lib_path=hip_lib, return_values=True)
    uret, _, uvalues = returns.critic_returns_torch(free, *args, lib_path=hip_lib, return_values=True)
    v = wvalues.cpu().numpy()
    assert (v == F32(crit.lo)).any() and (v == F32(crit.hi)).any() and not same_bits(uvalues.cpu().numpy(), v)          # the clip acts on this case
    assert same_bits(values.cpu().numpy(), v) and same_bits(ret.cpu().numpy(), wret.cpu().numpy()) and same_bits(mask.cpu().numpy(), wmask.cpu().numpy())
    assert not same_bits(uret.cpu().numpy(), wret.cpu().numpy())
    free.close(); crit.close()


# ---------------------------------------------------------------------------------------------------------------------------------- (6) refusals
def _refusals(lib_path, gpu):
    """every refusal by name; host addresses on the GPU too -- every call is refused before a launch, so none is dereferenced -- except the device id check,
    which is the last one and gets device tensors there"""
    lib = load_library(lib_path)
    T, N = 2, 4
    f = np.zeros(T * N, F32); i = np.ones(T * N, np.int32)
    sent = dict(rewards=np.full(T * N, -77.0, F32), mask=np.full(T * N, -77, np.int32), bounds=np.full(2, -77.0, F32), stats=np.full(ar.STATS_WORDS, -77.0),
                work=np.full(8, -77.0), out=np.full(T * N, -77.0, F32))
    nbytes = ar.workspace_bytes(T, N, lib_path)
    assert 0 < nbytes <= sent["work"].nbytes and nbytes % 8 == 0
    p = {k: v.ctypes.data for k, v in sent.items()}
    good = dict(T=T, N=N, logits_ptr=f.ctypes.data, task_reward_ptr=f.ctypes.data, done_ptr=i.ctypes.data, valid_ptr=i.ctypes.data, reward_scale=2.0, task_reward_lerp=0.5,
                rewards_ptr=p["rewards"], mask_ptr=p["mask"], bounds_ptr=p["bounds"], stats_ptr=p["stats"], work_ptr=p["work"], work_nbytes=nbytes, lib_path=lib_path)
    bad = [(dict(T=0), "T and N must be >= 1"), (dict(N=0), "T and N must be >= 1"), (dict(N=-2), "T and N must be >= 1"),
           (dict(T=65536, N=32768), "too many elements"),
           (dict(logits_ptr=0), "null argument"), (dict(rewards_ptr=0), "null argument"), (dict(bounds_ptr=0), "null argument"), (dict(stats_ptr=0), "null argument"),
           (dict(work_ptr=0), "null argument"), (dict(done_ptr=0), "valid needs done"),
           (dict(work_nbytes=nbytes - 1), "workspace too small"), (dict(work_nbytes=0), "workspace too small"),
           (dict(work_ptr=p["work"] + 4), "8-byte aligned"), (dict(stats_ptr=p["stats"] + 4), "8-byte aligned"),
           (dict(task_reward_lerp=None), "a task reward needs task_reward_lerp"), (dict(task_reward_lerp=1.5), "a task reward needs task_reward_lerp"),
           (dict(task_reward_lerp=-0.1), "a task reward needs task_reward_lerp")]
    for change, why in bad:
        with pytest.raises(RuntimeError, match="dm_amp_batch_rewards: .*" + why):
            ar.batch_rewards_device(**dict(good, **change))
        assert b"dm_amp_batch_rewards" in lib.dm_last_error()
    for change in (dict(T=0), dict(T=65536, N=32768)):
        with pytest.raises(RuntimeError, match="dm_amp_batch_rewards_workspace"):
            ar.workspace_bytes(**dict(dict(T=T, N=N, lib_path=lib_path), **change))
    cgood = dict(n=T * N, values_ptr=f.ctypes.data, bounds_ptr=p["bounds"], discount=0.95, out_ptr=p["out"], row_mask_ptr=i.ctypes.data, fill=0.0, lib_path=lib_path)
    cbad = [(dict(n=0), "n must be >= 1"), (dict(n=-1), "n must be >= 1"), (dict(values_ptr=0), "null argument"), (dict(bounds_ptr=0), "null argument"),
            (dict(out_ptr=0), "null argument"), (dict(discount=1.0), "discount must be in"), (dict(discount=-0.01), "discount must be in"),
            (dict(discount=float("nan")), "discount must be in")]
    for change, why in cbad:
        with pytest.raises(RuntimeError, match="dm_amp_value_clip: .*" + why):
            ar.value_clip_device(**dict(cgood, **change))
        assert b"dm_amp_value_clip" in lib.dm_last_error()
    if gpu:
        import torch
        dev = {k: torch.from_numpy(v).cuda() for k, v in sent.items()}
        df, di = torch.from_numpy(f).cuda(), torch.from_numpy(i).cuda()
        q = {k: v.data_ptr() for k, v in dev.items()}
        for device_id in (-1, torch.cuda.device_count()):
            with pytest.raises(RuntimeError, match="dm_amp_batch_rewards: invalid device_id"):
                ar.batch_rewards_device(**dict(good, logits_ptr=df.data_ptr(), task_reward_ptr=df.data_ptr(), done_ptr=di.data_ptr(), valid_ptr=di.data_ptr(), rewards_ptr=q["rewards"],
                                               mask_ptr=q["mask"], bounds_ptr=q["bounds"], stats_ptr=q["stats"], work_ptr=q["work"], device_id=device_id))
            with pytest.raises(RuntimeError, match="dm_amp_value_clip: invalid device_id"):
                ar.value_clip_device(**dict(cgood, values_ptr=df.data_ptr(), bounds_ptr=q["bounds"], out_ptr=q["out"], row_mask_ptr=di.data_ptr(), device_id=device_id))
        torch.cuda.synchronize()
        for k, v in dev.items():
            assert (v == -77).all(), k
    for k, v in sent.items():
        assert (v == -77).all(), k          # nothing was launched, nothing written


def test_refusals_emulator(emu_lib):
    _refusals(emu_lib, False)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    _refusals(hip_lib, True)


def test_the_front_end_checks_its_arguments(emu_lib):
    import torch
    trk = tracker(emu_lib, False, reward_scale=1.0)             # no TaskRewardLerp
    y = torch.zeros((2, 3))
    with pytest.raises(ValueError, match="task_reward_lerp"):
        trk.update_torch(y, torch.zeros((2, 3)))
    for bad in (dict(logits=torch.zeros(6)), dict(logits=y.double()), dict(done=torch.zeros((3, 2), dtype=torch.int32)), dict(valid=torch.zeros((2, 3)))):
        with pytest.raises(ValueError):
            trk.update_torch(**dict(dict(logits=y), **bad))
    with pytest.raises(ValueError):
        trk.clip_torch(y, row_mask=torch.zeros((3, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="discount"):
        tracker(emu_lib, False, discount=1.0)
    r, m = trk.update_torch(y, done=torch.zeros((2, 3), dtype=torch.bool), valid=torch.ones((2, 3), dtype=torch.int32))
    assert r.shape == (2, 3) and (m == 1).all()


# ---------------------------------------------------------------------------------------------------------------------------------- (7) two ranks
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["DM_ROOT"]); sys.path.insert(0, os.path.join(os.environ["DM_ROOT"], "tests"))
import torch, torch.distributed as dist
from deepmimic_amd import amp_rewards as ar
from deepmimic_amd.dist import all_reduce_reward_bounds
from test_amp_rewards import rank_case
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
trk = ar.AmpRewards("cpu", reward_scale=2.0, task_reward_lerp=0.3, lib_path=os.environ["DM_HIP_LIB"])
for it in range(2):
    c = rank_case(it)
    cols = slice(rank * 40, rank * 40 + 40)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, cols]))
    trk.update_torch(t(c["logits"]), t(c["task"]), t(c["done"]), t(c["valid"]))
    all_reduce_reward_bounds(trk)
    np.save(os.environ["DM_OUT"] + ".it%d.r%d.npy" % (it, rank), trk.bounds.numpy())
dist.barrier()
dist.destroy_process_group()
'''


def rank_case(it):
    """iteration `it` of an 80-column rollout, 40 columns per rank; the second one is shifted so that only one side of the bounds moves"""
    rng = np.random.default_rng(31 + it)
    T, N = 5, 80
    done = (rng.random((T, N)) < 0.3).astype(np.int32)
    valid = np.where(done != 0, rng.random((T, N)) >= 0.3, 1).astype(np.int32)
    return dict(logits=(1.0 + 1.5 * rng.standard_normal((T, N))).astype(F32), task=(rng.random((T, N)) + 2.0 * it).astype(F32), done=done, valid=valid)


def test_two_ranks_hold_the_single_process_bounds(emu_lib, tmp_path):
    out = str(tmp_path / "bounds")
    script = tmp_path / "amp_rewards_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, DM_ROOT=ROOT, DM_HIP_LIB=emu_lib, DM_OUT=out, MASTER_ADDR="127.0.0.1", DM_ALLOW_EMULATOR="1")
    port = 37500 + (os.getpid() % 2000)
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], env=env, timeout=600)
    single = tracker(emu_lib, False, reward_scale=2.0, task_reward_lerp=0.3)
    halves = []
    for it in range(2):
        c = rank_case(it)
        got = update(single, False, c["logits"], c["task"], c["done"], c["valid"])          # the concatenated rollouts
        a, b = np.load(out + ".it%d.r0.npy" % it), np.load(out + ".it%d.r1.npy" % it)
        assert same_bits(a, b) and same_bits(a, got["bounds"]) and np.isfinite(a).all()
        halves.append([ar.reference_batch_rewards(c["logits"][:, s], c["task"][:, s], c["done"][:, s], c["valid"][:, s], 2.0, 0.3)["bounds"] for s in (slice(0, 40), slice(40, 80))])
    h = halves[0]
    assert (h[0][0] != h[1][0]) and (h[0][1] != h[1][1])          # the ranks' own extrema differ: the reduction did something
