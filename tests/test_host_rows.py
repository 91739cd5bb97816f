"""The host boundary of dm_host.cpp as the caller sees it: the per-env state accessors move a window of columns of a strided device table and must leave
every other column of the row as the interface documents it (kept, or zeroed), and the step entry points are one I/O path behind several C-ABI names.
Every body runs on the emulator build of the host code and, marked `gpu`, on libdm_hip.so: 4 envs, fp32 and fp64, at most one control step."""
import ctypes as C

import numpy as np
import pytest

from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv, _fp, _ip

DT = 1.0 / 600
N = 4
PRECS = [32, 64]


def _real(x, prec):
    """what a double reads back as after a round trip through the context's kernel precision"""
    x = np.asarray(x, np.float64)
    return x.astype(np.float32).astype(np.float64) if prec == 32 else x


def _goal_rows(env):
    return env.get_goal_state(), env.get_goal_aux(), env.get_clips()


# ---------------------------------------------------------------- goal-row isolation
def _goal_row_isolation(lib, prec):
    rng = np.random.default_rng(11)
    env = BatchEnv(model.load_asset("amp_heading_zombie"), N, precision=prec, lib_path=lib, seed=3); env.reset()
    g0, a0, c0 = _goal_rows(env)
    assert g0.shape == (N, 12) and a0.shape == (N, 8) and c0.shape == (N,)
    # goal state: its 12 columns exactly, nothing else of the row
    g1 = rng.standard_normal((N, 12))
    env.set_goal_state(g1)
    g, a, c = _goal_rows(env)
    assert np.array_equal(g, g1) and np.array_equal(a, a0) and np.array_equal(c, c0)
    # aux: 7 columns exactly; column 7 of the interface row reads 0 whatever was written
    a1 = rng.standard_normal((N, 8))
    env.set_goal_aux(a1)
    g, a, c = _goal_rows(env)
    assert np.array_equal(a[:, :7], a1[:, :7]) and np.all(a[:, 7] == 0.0)
    assert np.array_equal(g, g1) and np.array_equal(c, c0)
    # the draw key of env 1 only: envs 0, 2, 3 keep every bit, env 1's goal state and aux read zero
    env.set_env_keys([1], [12345])
    g, a, c = _goal_rows(env)
    for e in (0, 2, 3):
        assert np.array_equal(g[e], g1[e]) and np.array_equal(a[e, :7], a1[e, :7]) and a[e, 7] == 0.0 and c[e] == c0[e], e
    assert np.all(g[1] == 0.0) and np.all(a[1] == 0.0)


def _clip_isolation(lib, prec):
    env = BatchEnv(model.load_asset("amp_heading_clips4"), N, precision=prec, lib_path=lib, seed=3); env.reset()
    assert env.num_clips == 4
    g0, a0, c0 = _goal_rows(env)
    c1 = np.array([3, 1, 0, 2], np.int32)
    assert not np.array_equal(c1, c0)
    env.set_clips(c1)
    g, a, c = _goal_rows(env)
    assert np.array_equal(c, c1) and np.array_equal(g, g0) and np.array_equal(a, a0)
    for bad in ([0, 1, 4, 2], [0, -1, 1, 2]):
        cl = np.array(bad, np.int32)
        assert env.lib.dm_set_clips(env.h, _ip(cl)) == -1
        assert env.lib.dm_last_error() == b"clip id out of range"
        g, a, c = _goal_rows(env)
        assert np.array_equal(c, c1) and np.array_equal(g, g0) and np.array_equal(a, a0)


@pytest.mark.parametrize("prec", PRECS)
def test_goal_row_windows_are_isolated(emu_lib, prec):
    _goal_row_isolation(emu_lib, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_clip_column_is_isolated_and_range_checked(emu_lib, prec):
    _clip_isolation(emu_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_goal_row_windows_are_isolated_gpu(hip_lib, prec):
    _goal_row_isolation(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_clip_column_is_isolated_and_range_checked_gpu(hip_lib, prec):
    _clip_isolation(hip_lib, prec)


# ---------------------------------------------------------------- precision round trip
def _ball_round_trip(lib, prec):
    rng = np.random.default_rng(5)
    env = BatchEnv(model.load_asset("amp_dribble_zombie"), N, precision=prec, lib_path=lib, seed=3); env.reset()
    x = rng.standard_normal((N, 13))
    env.set_obj_state(x)
    got = env.get_obj_state()
    assert got.shape == (N, 13) and np.array_equal(got, _real(x, prec))


def _v2(lib, prec):
    env = BatchEnv(model.load_asset("humanoid3d_walk"), N, precision=prec, lib_path=lib, seed=3, physics=2)
    env.reset(kin_times=[0.1, 0.2, 0.3, 0.4], max_times=5.0)
    return env


def _manifold_round_trip(lib, prec):
    rng = np.random.default_rng(6)
    a = _v2(lib, prec); b = _v2(lib, prec)
    x = rng.standard_normal((N, a.J, 25))
    a.set_manifolds(x)
    got = a.get_manifolds()
    assert got.shape == (N, a.J, 25) and np.array_equal(got, _real(x, prec))
    # a write zeroes the pad columns of the device row: after an all-zero write the table is all zero, whatever it held before
    z = np.zeros((N, a.J, 25))
    a.set_manifolds(z); b.set_manifolds(z)
    a.update(DT, 1); b.update(DT, 1)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(a.get_manifolds(), b.get_manifolds())


@pytest.mark.parametrize("prec", PRECS)
def test_ball_state_round_trips_at_kernel_precision(emu_lib, prec):
    _ball_round_trip(emu_lib, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_manifolds_round_trip_and_zero_their_pad(emu_lib, prec):
    _manifold_round_trip(emu_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ball_state_round_trips_at_kernel_precision_gpu(hip_lib, prec):
    _ball_round_trip(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_manifolds_round_trip_and_zero_their_pad_gpu(hip_lib, prec):
    _manifold_round_trip(hip_lib, prec)


# ---------------------------------------------------------------- state pads
def _walk(lib, prec, **kw):
    env = BatchEnv(model.load_asset("humanoid3d_walk"), N, precision=prec, lib_path=lib, seed=3, **kw)
    env.reset(kin_times=[0.1, 0.2, 0.3, 0.4], max_times=5.0)
    return env


def _state_pads(lib, prec):
    """Column 5 of a clock row (borrowed-lane substeps) and column 7 of a kin row (fallback substeps) lie next to the windows of dm_set_state and count
    "since the last dm_set_state": the write zeroes them.  To see that, a counter is made non-zero first: every character is laid on its back just above
    the ground, where one control step of the two-per-wave kernel gathers more than 32 constraint rows in some pair and runs substeps on borrowed lanes (the 64-lane
    fallback is not reached by this scene, so its counter is 0 before and after)."""
    rng = np.random.default_rng(7)
    env = _walk(lib, prec)
    st = env.get_state()
    pose = st["pose"].copy(); pose[:, 1] = 0.2; pose[:, 3:7] = [np.sqrt(0.5), -np.sqrt(0.5), 0.0, 0.0]
    env.set_state(pose=pose, vel=np.zeros_like(st["vel"]))
    env.step(None, DT, 20, open_loop=True)
    assert np.any(env.debug("borrowed") > 0), env.debug("borrowed")
    kin = rng.standard_normal((N, 7)); clk = rng.uniform(0.0, 1.0, (N, 5))
    env.set_state(kin=kin, clocks=clk)
    assert np.all(env.debug("fallback") == 0.0) and np.all(env.debug("borrowed") == 0.0)
    st = env.get_state()
    assert st["kin"].shape == (N, 7) and np.array_equal(st["kin"], _real(kin, prec))
    assert st["clocks"].shape == (N, 5) and np.array_equal(st["clocks"], clk)


@pytest.mark.parametrize("prec", PRECS)
def test_set_state_zeroes_the_counter_columns(emu_lib, prec):
    _state_pads(emu_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_set_state_zeroes_the_counter_columns_gpu(hip_lib, prec):
    _state_pads(hip_lib, prec)


# ---------------------------------------------------------------- step I/O equivalence
def _outs(env):
    return dict(state=np.zeros((N, env.S), np.float32), reward=np.zeros(N, np.float32), terminate=np.zeros(N, np.int32),
                valid=np.zeros(N, np.int32), episode_end=np.zeros(N, np.int32))


def _step_io(lib, prec):
    rng = np.random.default_rng(8)
    a = _walk(lib, prec); b = _walk(lib, prec)
    act = (0.1 * rng.standard_normal((N, a.A))).astype(np.float32)
    # dm_step_batch is dm_step_batch_amp without AMP observations
    oa = a.step(act, DT, 20)
    ob = _outs(b)
    rc = b.lib.dm_step_batch_amp(b.h, _fp(act), C.c_double(DT), 20, _fp(ob["state"]), _fp(ob["reward"]), _ip(ob["terminate"]), _ip(ob["valid"]),
                                 _ip(ob["episode_end"]), None, 0)
    assert rc == 0, b.lib.dm_last_error()
    for k in ob:
        assert np.array_equal(oa[k], ob[k]), k
    assert np.all(np.isfinite(oa["state"])) and np.any(oa["state"] != 0)
    # need_new_action of dm_query is column 0 of the flag rows
    assert np.array_equal(a.query()["need_new_action"], a.get_state()["flags"][:, 0])
    # dm_step_envs over every env in another order: the rows of dm_step_batch, permuted (one character per wavefront on both sides: the subset launch
    # always runs that kernel, and the two packings sum in different orders)
    c = _walk(lib, prec, wave_packing=1); d = _walk(lib, prec, wave_packing=1)
    oc = c.step(act, DT, 20)
    ids = np.array([2, 0, 3, 1], np.int32)
    od = d.step_envs(ids, act[ids], DT, 20)
    for k in ("state", "reward", "terminate", "valid", "episode_end"):
        assert np.array_equal(od[k], oc[k][ids]), k
    assert np.array_equal(od["clocks"], c.get_state()["clocks"][ids])


@pytest.mark.parametrize("prec", PRECS)
def test_step_entry_points_are_one_path(emu_lib, prec):
    _step_io(emu_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_step_entry_points_are_one_path_gpu(hip_lib, prec):
    _step_io(hip_lib, prec)
