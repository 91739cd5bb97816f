"""The checks of tests/test_reset_where_at.py (CPU emulator) and tests/test_reset_where_at_gpu.py (device): `BatchEnv.reset_where_at` / `dm_reset_where_at`.

Byte-exact, by the method of tests/reset_where_common.py (snapshot(), goal rows, clips, perturbation rows, last goals and the returned rows):
* nothing given -- no arrays, or arrays of -1 / NaN -- is `reset_where(mask)`, on every case of reset_where_common.CASES and under DM-physics 2
* clips = 0 and a time is `dm_reset(ids, kin_times)` on a twin context, compared on snapshot() and on what query() returns afterwards; unselected envs keep every byte
* a time that is not given beside a given clip is duration[clip] x dm_rand01 (stream 0, streams.reset_rand01), and the time limit is the draw of stream 1

Against the oracle's reset (Oracle.reset_ex(time, max_time, clip, yaw)) with clip, time and yaw given.  The state a reset leaves is the kinematic pose of the clip at
the given time, lifted off the ground, and the origin that goes with it; the bounds are the ones the project holds the kinematic pose to (tests/link_state_common.py:
5e-6 for an fp32 context, 1e-11 for an fp64 one, velocities relative to max(1, |v|max)); get_state() hands the context's own numbers back as float64, so no float32
rounding term is added.  Clocks are compared exactly."""
import numpy as np

from deepmimic_amd import kin_query as kq
from deepmimic_amd import model, streams
from deepmimic_amd.core import BatchEnv
from link_state_common import TOL_KIN32, TOL_KIN64
from reset_where_common import CASES, SENTINEL, pair
from test_episode_reset import DT, SEED, STEPS, assert_same, extras, same_bits


def nothing_given_equals_reset_where(case, lib, prec, n, physics=1):
    a, b, amp = pair(case, lib, prec, n, physics)
    resets = 0
    for k in range(STEPS):
        outs = [env.step(None, DT, 20, auto_reset=False, end_early=True, open_loop=True, amp=amp) for env in (a, b)]
        done = (outs[0]["episode_end"] != 0) | (outs[0]["valid"] == 0)
        resets += int(done.sum())
        oa = a.reset_where(done, states=outs[0]["state"], goals=outs[0].get("goal"))
        # alternately: no arrays at all / arrays that give nothing
        given = {} if k % 2 == 0 else dict(clips=np.full(n, -1, np.int32), times=np.full(n, np.nan), yaw=np.full(n, np.nan))
        ob = b.reset_where_at(done, states=outs[1]["state"], goals=outs[1].get("goal"), **given)
        assert ob.pop("bad") == 0
        assert sorted(oa) == sorted(ob)
        for key in oa:
            assert same_bits(oa[key], ob[key]), (k, key)
        if a.G:
            assert same_bits(a.last_goals(), b.last_goals()), k
        assert_same(a.snapshot(), b.snapshot(), k)
        assert_same(extras(a), extras(b), k)
    assert resets >= 2 * n, resets
    a.close(); b.close()


def given_time_equals_dm_reset(case, lib, prec, n):
    a, b, amp = pair(case, lib, prec, n)
    for env in (a, b):
        for _ in range(2):
            env.step(None, DT, 20, auto_reset=False, end_early=True, open_loop=True, amp=amp)
    ids = np.arange(0, n, 2, dtype=np.int32)
    mask = np.zeros(n, np.int32); mask[ids] = 1
    kt = 0.05 + 0.11 * np.arange(n)
    before, xb = b.snapshot(), extras(b)
    a.reset(ids, kin_times=kt[ids])
    sent_s = np.full((n, b.S), SENTINEL, np.float32)
    sent_g = np.full((n, b.G), SENTINEL, np.float32) if b.G else None
    out = b.reset_where_at(mask, clips=np.zeros(n, np.int32), times=kt, states=sent_s, goals=sent_g)
    assert out["bad"] == 0
    assert_same(a.snapshot(), b.snapshot(), "snapshot"); assert_same(extras(a), extras(b), "extras")
    qa, qb = a.query(), b.query()
    for key in qa:
        assert same_bits(qa[key], qb[key]), key
    for key in ("state", "goal") if b.G else ("state",):
        assert same_bits(out[key][mask != 0], qa[key][mask != 0]), key                  # the rows the reset wrote are the new episode's
        assert (out[key][mask == 0] == SENTINEL).all(), key                             # the others keep their bytes
    after, xa = b.snapshot(), extras(b)
    for key in before:
        assert same_bits(np.asarray(after[key])[mask == 0], np.asarray(before[key])[mask == 0]), key
    for key in xb:
        assert same_bits(xa[key][mask == 0], xb[key][mask == 0]), key
    assert same_bits(after["clocks"][ids, 0], kt[ids])
    a.close(); b.close()


def time_limit_of(t, e, ep):
    tmin, tmax = float(t.cfg.time_lim_min), float(t.cfg.time_lim_max)
    return tmin + (tmax - tmin) * streams.reset_rand01(SEED, e, ep, 1) if tmax > tmin else tmax


def check_against_oracle(t, env, e, prec, kt, mt, clip, yaw, label):
    from oracle_lib import Oracle
    st = env.get_state()
    o = Oracle(t)
    if env._has_goal_row:
        o.goal_rng(SEED, e, 0)
    o.reset_ex(float(kt), float(mt), int(clip), float(yaw))
    p, v = o.sim_state()
    ko = o.kin_state()[2]
    tol = TOL_KIN32 if prec == 32 else TOL_KIN64
    errs = [np.abs(st["pose"][e] - p).max(), np.abs(st["vel"][e] - v).max() / max(1.0, np.abs(v).max()), np.abs(st["kin"][e][:3] - ko[:3]).max(),
            min(np.abs(st["kin"][e][3:] - ko[3:]).max(), np.abs(st["kin"][e][3:] + ko[3:]).max())]
    print("RESETAT %s env %d f%d: worst error / bound %.3f" % (label, e, prec, max(errs) / tol))
    assert max(errs) <= tol, (label, e, errs)
    assert st["clocks"][e, 0] == kt and st["clocks"][e, 1] == kt and st["clocks"][e, 2] == -kt and st["clocks"][e, 3] == 0 and st["clocks"][e, 4] == mt, st["clocks"][e]


def given_start_against_oracle(name, lib, prec, label):
    """clip, time and a non-zero yaw given (a plain scene takes the yaw too); every env selected"""
    t = model.load_asset(name)
    n = 4 if name == "amp_heading_clips4" else 3
    env = BatchEnv(t, n, precision=prec, lib_path=lib, seed=SEED)
    env.reset()
    env.step(None, DT, 20, open_loop=True)
    ep = env.get_state()["flags"][:, 2].copy()
    clips = (np.arange(n) % 2).astype(np.int32) if t.num_clips > 1 else np.zeros(n, np.int32)      # (the two looping clips of the dataset: they start upright)
    kt = 0.1 + 0.17 * np.arange(n)
    yaw = np.array([0.7, -2.1, 3.0, -0.4])[:n]
    out = env.reset_where_at(np.ones(n, np.int32), clips=clips, times=kt, yaw=yaw)
    assert out["bad"] == 0
    if env._has_goal_row:
        assert (env.get_clips() == clips).all()
    assert (env.get_state()["flags"][:, 2] == ep + 1).all()
    for e in range(n):
        check_against_oracle(t, env, e, prec, kt[e], time_limit_of(t, e, int(ep[e])), clips[e], yaw[e], label + " " + name)
    assert same_bits(out["state"], env.query()["state"])
    env.close()


def drawn_time_with_given_clip(lib, prec, label):
    """amp_heading_clips4, the clip given and nothing else: the time is duration[clip] x dm_rand01 (stream 0), the yaw the scene's rule (stream 4)"""
    t = model.load_asset("amp_heading_clips4")
    n = 4
    env = BatchEnv(t, n, precision=prec, lib_path=lib, seed=SEED)
    env.reset()
    ep = env.get_state()["flags"][:, 2].copy()
    dur, _ = env.clip_table()
    clips = np.array([1, 0, 1, 0], np.int32)
    out = env.reset_where_at(np.ones(n, np.int32), clips=clips)
    assert out["bad"] == 0 and (env.get_clips() == clips).all()
    clk = env.get_state()["clocks"]
    assert t.cfg.enable_rand_rot_reset
    for e in range(n):
        kt = dur[clips[e]] * streams.reset_rand01(SEED, e, int(ep[e]), 0)
        assert clk[e, 0] == kt, (e, clk[e, 0], kt)
        yaw = -np.pi + 2 * np.pi * streams.reset_rand01(SEED, e, int(ep[e]), 4)
        check_against_oracle(t, env, e, prec, kt, time_limit_of(t, e, int(ep[e])), clips[e], yaw, label + " drawn time")
    # the time given, clip and yaw not: the clip by weight (stream 3), the yaw 0 -- the rule dm_reset applies beside a given time
    from oracle_lib import Oracle
    ep = env.get_state()["flags"][:, 2].copy()
    kt = np.array([0.2, 0.3, 0.1, 0.25])
    out = env.reset_where_at(np.ones(n, np.int32), times=kt)
    o = Oracle(t)
    want = np.array([o.draw_clip(streams.reset_rand01(SEED, e, int(ep[e]), 3)) for e in range(n)], np.int32)
    assert out["bad"] == 0 and (env.get_clips() == want).all(), (env.get_clips(), want)
    for e in np.nonzero(want < 2)[0]:                              # (clips 2 and 3 start lying on the ground: stiff contacts, tests/test_goal_scenes.py)
        check_against_oracle(t, env, int(e), prec, kt[e], time_limit_of(t, int(e), int(ep[e])), want[e], 0.0, label + " drawn clip")
    env.close()


def invalid_inputs(lib, prec):
    """CPU emulator only: an env with an invalid value keeps every byte of its state and of its output rows, bad becomes 1, the valid envs of the call are reset"""
    for case in ("plain", "amp_heading_clips4"):
        a, b, amp = pair(case, lib, prec, 4)
        a.close()
        nc = max(1, b.num_clips)
        nan = np.full(4, np.nan)
        wrong = [dict(clips=[nc, 0, 0, 0]), dict(clips=[-2, 0, 0, 0]), dict(clips=[2 ** 30, 0, 0, 0]), dict(times=[-0.1, 0.2, 0.2, 0.2]), dict(times=[np.inf, 0.2, 0.2, 0.2]),
                 dict(times=[-np.inf, 0.2, 0.2, 0.2]), dict(yaw=[np.inf, 0.3, 0.3, 0.3]), dict(yaw=[-np.inf, 0.3, 0.3, 0.3], times=[0.1, 0.2, 0.2, 0.2])]
        for given in wrong:
            before, xb = b.snapshot(), extras(b)
            goals_before = b.last_goals() if b.G else None
            sent_s = np.full((4, b.S), SENTINEL, np.float32)
            sent_g = np.full((4, b.G), SENTINEL, np.float32) if b.G else None
            out = b.reset_where_at(np.array([1, 1, 0, 1], np.int32), states=sent_s, goals=sent_g, **given)
            assert out["bad"] == 1, given
            after, xa = b.snapshot(), extras(b)
            keep, fresh = np.array([0, 2]), np.array([1, 3])                   # env 0: invalid, env 2: not selected
            for key in before:
                assert same_bits(np.asarray(after[key])[keep], np.asarray(before[key])[keep]), (given, key)
            for key in xb:
                assert same_bits(xa[key][keep], xb[key][keep]), (given, key)
            assert (after["flags"][fresh, 2] == before["flags"][fresh, 2] + 1).all(), given       # the valid envs of the call started an episode
            assert (out["state"][keep] == SENTINEL).all() and not (out["state"][fresh] == SENTINEL).any(), given
            if b.G:
                assert (out["goal"][keep] == SENTINEL).all() and same_bits(b.last_goals()[keep], goals_before[keep]), given
        assert b.reset_where_at(np.ones(4, np.int32), clips=[nc - 1, -1, 0, -1], times=[0.0, np.nan, 0.1, 0.2], yaw=nan)["bad"] == 0      # the edges of the valid range
        b.close()


def refusals(lib, prec):
    import pytest
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=prec, lib_path=lib)
    env.reset()
    buf = np.zeros(64, np.float32)          # never written: every call below is refused before a launch
    a = buf.ctypes.data
    with pytest.raises(RuntimeError, match="dm_reset_where_at: null mask_dev"):
        kq.reset_where_at_device(env, 0, 0, 0, 0, a, 0, 0)
    with pytest.raises(RuntimeError, match="dm_reset_where_at: null states_dev"):
        kq.reset_where_at_device(env, a, 0, 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dm_reset_where_at: goals_dev on a scene without a goal"):
        kq.reset_where_at_device(env, a, 0, 0, 0, a, a, 0)
    from deepmimic_amd.core import TAPE_STRIDE
    env.set_draw_tape(np.zeros((env.N, TAPE_STRIDE)))
    with pytest.raises(RuntimeError, match="dm_reset_where_at: a draw tape is bound"):
        kq.reset_where_at_device(env, a, 0, 0, 0, a, 0, 0)
    env.set_draw_tape(None)
    assert env.lib.dm_reset_where_at(None, a, None, None, None, a, None, None) != 0
    assert (buf == 0).all()
    env.close()
