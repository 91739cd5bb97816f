"""`TorchVecEnv.state_pool()` and a start sampler's "slots" on the GPU (deepmimic_amd/vec_env.py, deepmimic_amd/state_pool.py): done envs with a slot start a new
episode at the stored state, the other done envs are reset exactly as without a pool; the torch pool is data (clone, state_dict through torch.save / load).  N = 4,
M = 5, episodes pinned to 0.1 s: every env ends in the same step."""
import io

import numpy as np
import pytest

from deepmimic_amd import model
from state_pool_common import record

pytestmark = pytest.mark.gpu
N, M, SEED = 4, 5, 17


def tables(asset="humanoid3d_walk", limit=0.1):
    t = model.load_asset(asset)
    t.cfg.time_lim_min = t.cfg.time_lim_max = limit
    return t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("asset", ["humanoid3d_walk", "amp_heading_clips4"])
def test_fixed_slots_for_some_done_envs(hip_lib, asset):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    kw = dict(seed=SEED, deferred_reset=True, episode_stats=True, lib_path=hip_lib)
    a, b = TorchVecEnv(tables(asset), N, **kw), TorchVecEnv(tables(asset), N, **kw)
    a.reset(); b.reset()
    pool = a.state_pool(M)
    i32 = dict(dtype=torch.int32, device=a.device)
    slots = [2, -1, 0, -1]
    fixed = torch.tensor(slots, **i32)
    act = torch.zeros((N, a.act_dim), device=a.device)
    ra, rb = a.step(act), b.step(act)
    age, finished = np.ones(N, int), int(ra[2].sum())
    age[ra[2].cpu().numpy()] = 0
    pool.save(torch.ones(N, **i32), torch.arange(N, **i32))                  # slots 0 .. 3: the envs after their first step
    a.set_start_sampler(lambda done, info: {"slots": fixed})
    stored = pool.data.cpu().numpy()
    real = np.float32
    own = np.zeros(N, bool)                                                  # envs of `a` that have started from the pool: on a path of their own from then on
    from_pool = plain = 0
    for k in range(8):                                                       # (the pinned limit ends every episode by the fourth step)
        before = a.env.get_state()["flags"][:, 2].copy()
        ra, rb = a.step(act), b.step(act)
        age += 1
        done, twin = ra[2].cpu().numpy(), ~own
        for x, y in ((ra[1], rb[1]), (ra[2], rb[2]), (ra[3]["terminal_obs"], rb[3]["terminal_obs"])):
            assert same(x[twin], y[twin]), k
        assert ra[3]["episode_length"].cpu().numpy()[done].tolist() == age[done].tolist(), k      # the finished episode, counted at its own length
        finished += int(done.sum())
        age[done] = 0                                                        # the new one starts at length 0
        sa, sb = a.env.snapshot(), b.env.snapshot()
        for e in np.nonzero(done)[0]:
            if slots[e] < 0:
                plain += 1
                continue
            from_pool += 1; own[e] = True                                    # from the pool: the slot's pose and clocks, a fresh timer, the next episode
            for key in ("pose", "vel", "tar", "kin"):
                assert sa[key][e].tobytes() == record(a.env, stored, slots[e], key, real)[:sa[key].shape[1]].astype(np.float64).tobytes(), (e, key)
            clk = record(a.env, stored, slots[e], "clock", np.float64)
            assert sa["clocks"][e, :3].tobytes() == clk[:3].tobytes() and sa["clocks"][e, 3] == 0.0 and sa["clocks"][e, 4] == 0.1
            assert sa["flags"][e, 2] == before[e] + 1 and sa["flags"][e, 3] == 1
        twin = ~own
        for key in sa:                                                       # the others: the twin without a pool, byte for byte
            assert np.ascontiguousarray(sa[key][twin]).tobytes() == np.ascontiguousarray(sb[key][twin]).tobytes(), (k, key)
        assert same(ra[0][twin], rb[0][twin])
        if a.goal_dim:
            assert same(a.goal[twin], b.goal[twin])
        if from_pool and plain:
            break
    assert from_pool and plain
    assert not same(ra[0][own], rb[0][own])
    obs, goal = a.obs.clone(), a.goal.clone() if a.goal_dim else None
    a._enter(); a._launch(0, 0, False)                                       # the zero-update launch
    if a.goal_dim:
        a.env.last_goals_device(a.goal.data_ptr())
        assert same(a.goal, goal)
    assert same(a.obs, obs)
    assert int(pool.bad.item()) == 0 and int(a.start_bad.item()) == 0
    totals = a.episode_totals()
    assert totals["episodes"] + totals["invalid"]["episodes"] == finished    # each finished episode was counted once
    a.close(); b.close()


def test_the_torch_pool_is_data(hip_lib):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    kw = dict(seed=SEED, deferred_reset=True, amp_obs=True, lib_path=hip_lib)
    a, b = TorchVecEnv(tables("amp_heading_clips4", 10.0), N, **kw), TorchVecEnv(tables("amp_heading_clips4", 10.0), N, **kw)
    a.reset(); b.reset()
    i32 = dict(dtype=torch.int32, device=a.device)
    every, ids = torch.ones(N, **i32), torch.arange(N, **i32)
    act = torch.zeros((N, a.act_dim), device=a.device)
    a.step(act)
    pool = a.state_pool(M).save(every, ids)
    want, obs, goal = a.env.snapshot(), a.obs.clone(), a.goal.clone()
    first = [x.clone() for x in a.step(act)[:2]]
    twin = pool.clone()
    assert twin.data.data_ptr() != pool.data.data_ptr() and same(twin.data, pool.data)
    pool.data.zero_()
    twin.restore(every.bool(), ids)                                          # (a bool mask is taken too)
    got = a.env.snapshot()
    assert all(np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in want)
    assert same(a.obs, obs) and same(a.goal, goal)                           # the restore wrote the env's own rows
    f = io.BytesIO()
    torch.save(twin.state_dict(), f)
    f.seek(0)
    pb = b.state_pool(M).load_state_dict(torch.load(f))
    pb.restore(every, ids)
    for x, y in zip(b.step(act)[:2], first):
        assert same(x, y)
    other = TorchVecEnv(tables("humanoid3d_walk"), N, seed=SEED, lib_path=hip_lib)
    with pytest.raises(ValueError, match="not a pool of this scene and precision"):
        other.state_pool(M).load_state_dict(twin.state_dict())
    with pytest.raises(ValueError, match="the pool holds"):
        b.state_pool(M + 1).load_state_dict(twin.state_dict())
    with pytest.raises(ValueError, match="mask must be"):
        twin.save(every.to(torch.int64), ids)
    for e in (a, b, other):
        e.close()


def test_no_pool_no_calls_and_the_value_errors(hip_lib, monkeypatch):
    import torch
    from deepmimic_amd import state_pool as sp
    from deepmimic_amd.vec_env import TorchVecEnv
    from test_time_warp import amp_walk
    calls = {"save_device": 0, "restore_device": 0}
    for name in calls:
        def counting(*args, _real=getattr(sp, name), _name=name, **kwargs):
            calls[_name] += 1
            return _real(*args, **kwargs)
        monkeypatch.setattr(sp, name, counting)
    env = TorchVecEnv(tables(), N, seed=SEED, deferred_reset=True, lib_path=hip_lib)
    i32 = dict(dtype=torch.int32, device=env.device)
    env.reset()
    env.set_start_sampler(lambda done, info: {})
    act = torch.zeros((N, env.act_dim), device=env.device)
    for _ in range(4):
        env.step(act)
    assert calls == {"save_device": 0, "restore_device": 0}
    none = torch.full((N,), -1, **i32)
    env.set_start_sampler(lambda done, info: {"slots": none})
    with pytest.raises(ValueError, match="slots need a pool"):
        env.step(act)
    pool = env.state_pool(M)
    pool.save(torch.ones(N, **i32), torch.arange(N, **i32))
    env.step(act)
    assert calls == {"save_device": 1, "restore_device": 1}
    env.set_start_sampler(lambda done, info: {"slots": none.to(torch.int64)})
    with pytest.raises(ValueError, match="start sampler's slots must be"):
        env.step(act)
    env.close()
    tw = TorchVecEnv(amp_walk(), N, seed=SEED, deferred_reset=True, time_warp=True, test_mode=True, lib_path=hip_lib)
    tw.reset()
    tw.state_pool(M)
    tw.set_start_sampler(lambda done, info: {"slots": none})
    with pytest.raises(ValueError, match="cannot be used with time_warp=True"):
        tw.step(torch.zeros((N, tw.act_dim), device=tw.device))
    tw.close()
