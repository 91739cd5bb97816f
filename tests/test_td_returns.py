"""TD(lambda) returns on the device (deepmimic_amd/csrc/dm_returns.h, include/dm_hip.h dm_td_lambda_returns) against the reference's own
RLUtil.compute_return: tests/golden/td_returns.npz holds random [T, N] rollouts cut into paths, each path's return from the reference's function with val_t assembled
by the end-of-path rules of learning/ppo_agent.py:251-266 (tests/golden/make_td_returns.py wrote it where the reference lies).  The kernel computes in fp64 with the
reference's association and rounds once, so the comparison is an equality of bits: there is no tolerance.  Shapes: T in {1, 5, 7} x N in {3, 64, 65} (one partial wave,
one full, one full + one lane); columns: no done, done at 0, done at T - 1, consecutive dones of every kind, an invalid episode in the middle / running into t = 0, random."""
import ctypes as C
import os

import numpy as np
import pytest

from deepmimic_amd import returns
from deepmimic_amd.core import load_library

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "td_returns.npz")
INPUTS = ("rewards", "values", "term_values", "terminate", "done", "valid")
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(GOLD))
    return _gold


def shapes():
    return [(T, N) for T in (1, 5, 7) for N in (3, 64, 65)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_fixture(T, N, run):
    """run(inputs dict of host arrays, gamma, lambda, val_fail, val_succ) -> (returns, mask) host arrays"""
    g = gold()
    assert [tuple(s) for s in g["shapes"]] == shapes()
    key = "T%d_N%d" % (T, N)
    inp = {k: g[key + "/" + k] for k in INPUTS}
    vf, vs = [float(x) for x in g["val_fail_succ"]]
    for p, (gamma, lam) in enumerate(g["params"]):
        ret, mask = run(inp, float(gamma), float(lam), vf, vs)
        want, wmask = g["%s/returns%d" % (key, p)], g["%s/mask%d" % (key, p)]
        assert want.dtype == np.float32 and np.isfinite(want).all()
        assert same_bits(ret, want), (key, gamma, lam, np.abs(ret.astype(np.float64) - want).max())
        assert same_bits(mask, wmask), (key, gamma, lam)
        if gamma == 0:
            assert same_bits(ret, inp["rewards"])          # learning/ppo_agent.py:269-270


def test_fixture_covers_the_cases():
    g = gold()
    for T, N in shapes():
        d, tm, v = (g["T%d_N%d/%s" % (T, N, k)] for k in ("done", "terminate", "valid"))
        assert not d[:, 0].any() and d[0, 1] == 1                               # no done at all; done at t = 0
        assert d[T - 1, 2] == 1 and tm[T - 1, 2] == 1                           # done (Fail) at t = T - 1
        if T >= 5:
            assert d[1:4, N - 3 + 0 if N == 3 else 3].all() or N == 3           # consecutive dones (column 3; N = 3 has columns 0 .. 2 only)
        if N > 6 and T >= 5:
            assert sorted(set(tm[1:4, 3])) == [0, 1, 2]                         # Null, Fail and Succ ends
            assert v[3, 4] == 0 and d[1, 4] == 1 and (g["T%d_N%d/mask0" % (T, N)][:, 4] == [1, 1, 0, 0] + [1] * (T - 4)).all()      # invalid in the middle
            assert v[2, 5] == 0 and (g["T%d_N%d/mask0" % (T, N)][:3, 5] == 0).all() and (g["T%d_N%d/mask0" % (T, N)][3:, 5] == 1).all()      # invalid into t = 0


def run_emulator(lib):
    def run(inp, gamma, lam, vf, vs):
        T, N = inp["rewards"].shape
        a = {k: np.ascontiguousarray(v) for k, v in inp.items()}
        ret = np.full((T, N), np.nan, np.float32); mask = np.full((T, N), -1, np.int32)
        returns.td_lambda_returns(T, N, a["rewards"].ctypes.data, a["values"].ctypes.data, a["term_values"].ctypes.data, a["terminate"].ctypes.data, a["done"].ctypes.data,
                                  a["valid"].ctypes.data, gamma, lam, vf, vs, ret.ctypes.data, mask.ctypes.data, lib_path=lib)
        return ret, mask
    return run


def run_gpu(lib):
    import torch

    def run(inp, gamma, lam, vf, vs):
        a = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
        ret, mask = returns.td_lambda_returns_torch(a["rewards"], a["values"], a["term_values"], a["terminate"], a["done"], a["valid"], gamma, lam, vf, vs, lib_path=lib)
        return ret.cpu().numpy(), mask.cpu().numpy()
    return run


@pytest.mark.parametrize("T,N", shapes())
def test_td_lambda_returns_equal_the_reference_bit_for_bit_emulator(emu_lib, T, N):
    check_against_fixture(T, N, run_emulator(emu_lib))


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", shapes())
def test_td_lambda_returns_equal_the_reference_bit_for_bit_gpu(hip_lib, T, N):
    check_against_fixture(T, N, run_gpu(hip_lib))


def test_optional_arrays_emulator(emu_lib):
    """valid NULL = every episode valid (mask all ones, same returns); mask NULL = not written"""
    g = gold(); key = "T7_N65"
    a = {k: np.ascontiguousarray(g[key + "/" + k]) for k in INPUTS}
    vf, vs = [float(x) for x in g["val_fail_succ"]]
    ret = np.zeros((7, 65), np.float32); mask = np.full((7, 65), -1, np.int32)
    returns.td_lambda_returns(7, 65, a["rewards"].ctypes.data, a["values"].ctypes.data, a["term_values"].ctypes.data, a["terminate"].ctypes.data, a["done"].ctypes.data,
                              0, 0.95, 0.95, vf, vs, ret.ctypes.data, mask.ctypes.data, lib_path=emu_lib)
    assert same_bits(ret, g[key + "/returns0"]) and (mask == 1).all()
    ret2 = np.zeros((7, 65), np.float32)
    returns.td_lambda_returns(7, 65, a["rewards"].ctypes.data, a["values"].ctypes.data, a["term_values"].ctypes.data, a["terminate"].ctypes.data, a["done"].ctypes.data,
                              a["valid"].ctypes.data, 0.95, 0.95, vf, vs, ret2.ctypes.data, 0, lib_path=emu_lib)
    assert same_bits(ret2, ret)


def _argument_checks(lib_path):
    lib = load_library(lib_path)
    buf = np.zeros(16, np.float32); ibuf = np.zeros(16, np.int32); out = np.full(16, 7.0, np.float32)
    p, ip = buf.ctypes.data, ibuf.ctypes.data
    good = dict(T=2, N=4, rewards_ptr=p, values_ptr=p, term_values_ptr=p, terminate_ptr=ip, done_ptr=ip, valid_ptr=ip, gamma=0.9, td_lambda=0.9, val_fail=0.0, val_succ=1.0,
                returns_ptr=out.ctypes.data, mask_ptr=0, lib_path=lib_path)
    bad = [dict(T=0), dict(N=0), dict(T=-3), dict(rewards_ptr=0), dict(values_ptr=0), dict(term_values_ptr=0), dict(terminate_ptr=0), dict(done_ptr=0), dict(returns_ptr=0)]
    for b in bad:
        with pytest.raises(RuntimeError, match="dm_td_lambda_returns"):
            returns.td_lambda_returns(**dict(good, **b))
        assert b"dm_td_lambda_returns" in lib.dm_last_error()
    assert (out == 7.0).all()           # nothing was launched


def test_argument_checks_emulator(emu_lib):
    _argument_checks(emu_lib)


@pytest.mark.gpu
def test_argument_checks_gpu(hip_lib):
    """host addresses: every call is refused before a launch, so none is dereferenced"""
    _argument_checks(hip_lib)


@pytest.mark.gpu
def test_torch_convenience_checks_its_tensors(hip_lib):
    import torch
    T, N = 3, 4
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    ok = dict(rewards=f(T, N), values=f(T + 1, N), term_values=f(T, N), terminate=i(T, N), done=i(T, N), valid=i(T, N))
    for k, bad in (("values", f(T, N)), ("rewards", f(T, N).double()), ("term_values", f(N, T).t()), ("terminate", i(T, N).cpu()), ("valid", f(T, N))):
        with pytest.raises(ValueError):
            returns.td_lambda_returns_torch(**dict(ok, **{k: bad}), gamma=0.9, td_lambda=0.9, val_fail=0.0, val_succ=1.0, lib_path=hip_lib)
    ret, mask = returns.td_lambda_returns_torch(**dict(ok, done=torch.zeros((T, N), dtype=torch.bool, device="cuda")), gamma=0.9, td_lambda=0.9, val_fail=0.0, val_succ=1.0, lib_path=hip_lib)
    assert ret.shape == (T, N) and (mask == 1).all()


def numpy_recursion(r, v, tv, term, done, valid, gamma, lam, vf, vs):
    """the recursion of include/dm_hip.h in numpy float64 on host copies, one rounding to float32"""
    T, N = r.shape
    ret, mask = np.zeros((T, N)), np.ones((T, N), np.int32)
    r, v, tv = r.astype(np.float64), v.astype(np.float64), tv.astype(np.float64)
    for n in range(N):
        nxt, inv = 0.0, False
        for t in reversed(range(T)):
            d = bool(done[t, n])
            v_next = (vf if term[t, n] == 1 else vs if term[t, n] == 2 else tv[t, n]) if d else v[t + 1, n]
            if d or t == T - 1:
                cur = r[t, n] + gamma * v_next
            else:
                cur = r[t, n] + gamma * ((1.0 - lam) * v_next + lam * nxt)
            if d:
                inv = valid[t, n] == 0
            ret[t, n], mask[t, n], nxt = cur, 0 if inv else 1, cur
    return ret.astype(np.float32), mask


@pytest.mark.gpu
def test_rollout_to_critic_targets_end_to_end_gpu(hip_lib):
    """TorchVecEnv rollout (walk, 64 envs, 8 steps, episode timers of 0.1 .. 0.2 s, noisy actions) -> a random-init one-output critic on `obs` and on
    info["terminal_obs"] -> td_lambda_returns; equal, bit for bit, to the same recursion in numpy float64 on the host copies"""
    import torch
    from deepmimic_amd import model
    from deepmimic_amd.policy import Policy, random_weights
    from deepmimic_amd.vec_env import TorchVecEnv
    T, N = 8, 64
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), N, seed=3, lib_path=hip_lib)
    env.env.set_time_limits(0.1, 0.2)
    critic = Policy(random_weights(env.obs_dim, 1, seed=5, init_output_scale=1.0), lib_path=hip_lib)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def value(obs, out_row):
        critic.forward_device(obs.data_ptr(), N, out_row.data_ptr(), stream=stream)
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    rewards, values, term_values = torch.zeros((T, N), **f32), torch.zeros((T + 1, N), **f32), torch.zeros((T, N), **f32)
    terminate, done, valid = torch.zeros((T, N), **i32), torch.zeros((T, N), **i32), torch.zeros((T, N), **i32)
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    obs = env.reset()
    for t in range(T):
        value(obs, values[t])
        acts = 0.6 * torch.randn((N, env.act_dim), generator=gen, **f32)
        obs, r, d, info = env.step(acts)
        rewards[t], terminate[t], done[t], valid[t] = r, info["terminate"], d.to(torch.int32), info["valid"]
        value(info["terminal_obs"], term_values[t])          # rows of envs that did not end hold an older terminal row: finite, and never read
    value(obs, values[T])
    ret, mask = returns.td_lambda_returns_torch(rewards, values, term_values, terminate, done, valid, 0.95, 0.95, 0.0, 20.0, lib_path=hip_lib)
    h = [x.cpu().numpy() for x in (rewards, values, term_values, terminate, done, valid)]
    assert h[4].sum() >= N and ((h[4] != 0) & (h[3] == 0)).any()           # every env's timer ran out at least once: Null ends are in
    assert np.isfinite(h[1]).all() and np.isfinite(h[2]).all() and h[1].std() > 0
    want, wmask = numpy_recursion(*h, 0.95, 0.95, 0.0, 20.0)
    assert same_bits(ret.cpu().numpy(), want) and same_bits(mask.cpu().numpy(), wmask)
    critic.close(); env.close()
