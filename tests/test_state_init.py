"""`VisitedStateStarts` (deepmimic_amd/state_init.py) on the GPU: N = 64 envs, a ring of M = 32 slots, 4 saves per step, episodes pinned to 0.1 s, 12 steps.  Two
samplers of one seed hand out the same tensors; a start fraction of 0 is the env without a sampler, byte for byte; with a fraction of 1 every done env stands at a
stored state afterwards; a PPOAgent trains on the env as it is, reproducibly."""
import numpy as np
import pytest

from deepmimic_amd import model
from state_pool_common import record
from test_agent import KINDS, M as MINI, T, differing, snap

pytestmark = pytest.mark.gpu
N, M, SAVES, STEPS, SEED = 64, 32, 4, 12, 17


def make_env(hip_lib, fraction=None, seed=3):
    from deepmimic_amd.state_init import VisitedStateStarts
    from deepmimic_amd.vec_env import TorchVecEnv
    t = model.load_asset("humanoid3d_walk")
    t.cfg.time_lim_min = t.cfg.time_lim_max = 0.1
    env = TorchVecEnv(t, N, seed=SEED, deferred_reset=True, lib_path=hip_lib)
    env.reset()
    sampler = None
    if fraction is not None:
        sampler = VisitedStateStarts(env, M, saves_per_step=SAVES, start_fraction=fraction, seed=seed)
        env.set_start_sampler(sampler)
    return env, sampler


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def actions(env, k):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(100 + k)
    return (0.1 * torch.randn((N, env.act_dim), generator=gen)).to(env.device)


def test_two_samplers_of_one_seed(hip_lib):
    (a, sa), (b, sb) = make_env(hip_lib, 0.5), make_env(hip_lib, 0.5)
    assert same(sa.pool.data, sb.pool.data) and bool(sa.pool.data.any(dim=1).all())      # every slot was filled at construction
    started = 0
    for k in range(STEPS):
        ra, rb = a.step(actions(a, k)), b.step(actions(b, k))
        for x, y in zip(ra[:3], rb[:3]):
            assert same(x, y), k
        assert same(sa.start_slots, sb.start_slots) and same(sa.pool.data, sb.pool.data), k
        started += int((sa.start_slots >= 0).sum())
        assert bool(((sa.start_slots >= 0) <= ra[2]).all())                  # only done envs start from the pool
    assert started > 0 and sa.cursor == (STEPS * SAVES) % M
    for env, s in ((a, sa), (b, sb)):
        assert int(env.start_bad.item()) == 0 and int(s.pool.bad.item()) == 0
        env.close()


def test_fraction_zero_is_the_env_without_a_sampler(hip_lib):
    (a, sa), (b, _) = make_env(hip_lib, 0.0), make_env(hip_lib, None)
    done = 0
    for k in range(STEPS):
        ra, rb = a.step(actions(a, k)), b.step(actions(b, k))
        for x, y in zip(ra[:3], rb[:3]):
            assert same(x, y), k
        assert bool((sa.start_slots == -1).all())
        done += int(ra[2].sum())
    assert done >= 2 * N
    x, y = a.env.snapshot(), b.env.snapshot()
    assert all(np.ascontiguousarray(x[key]).tobytes() == np.ascontiguousarray(y[key]).tobytes() for key in x)
    assert int(a.start_bad.item()) == 0 and int(sa.pool.bad.item()) == 0
    a.close(); b.close()


def test_fraction_one_starts_every_done_env_at_a_stored_state(hip_lib):
    a, sa = make_env(hip_lib, 1.0)
    done_total = 0
    for k in range(STEPS):
        _, _, done, _ = a.step(actions(a, k))
        d = done.cpu().numpy()
        if d.any():
            stored = sa.pool.data.cpu().numpy()
            clocks = {record(a.env, stored, s, "clock", np.float64)[0].tobytes() for s in range(M)}
            picked = sa.start_slots.cpu().numpy()
            st = a.env.get_state()
            assert (picked[d] >= 0).all() and (picked[~d] == -1).all()
            for e in np.nonzero(d)[0]:
                assert st["clocks"][e, 0].tobytes() in clocks, (k, e)                      # the kin clock of some slot
                assert st["clocks"][e, 0].tobytes() == record(a.env, stored, picked[e], "clock", np.float64)[0].tobytes() and st["clocks"][e, 3] == 0.0
            done_total += int(d.sum())
    assert done_total >= 2 * N
    assert int(a.start_bad.item()) == 0 and int(sa.pool.bad.item()) == 0
    a.close()


def test_constructor_refusals(hip_lib):
    from deepmimic_amd.state_init import VisitedStateStarts
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 4, seed=SEED, lib_path=hip_lib)
    env.reset()
    with pytest.raises(ValueError, match="deferred_reset=True"):
        VisitedStateStarts(env, 8)
    env.close()
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 4, seed=SEED, deferred_reset=True, lib_path=hip_lib)
    env.reset()
    with pytest.raises(ValueError, match="saves_per_step"):
        VisitedStateStarts(env, 8, saves_per_step=5)
    with pytest.raises(ValueError, match="start_fraction"):
        VisitedStateStarts(env, 8, start_fraction=1.5)
    env.close()


def ppo_with_sampler(hip_lib):
    from deepmimic_amd import agent
    env, sampler = make_env(hip_lib, 0.5)
    _, d = KINDS["ppo"]
    return agent.make_agent(env, agent.AgentConfig.from_dict(d), rollout_steps=T, seed=1, mini_batch_size=MINI), sampler


def test_ppo_agent_trains_reproducibly_with_the_sampler(hip_lib):
    (a, sa), (b, sb) = ppo_with_sampler(hip_lib), ppo_with_sampler(hip_lib)
    for _ in range(2):
        a.iterate(); b.iterate()
    assert sa.cursor == (2 * T * SAVES) % M
    assert differing(snap(a), snap(b)) == []
    assert a.rollout.reward.cpu().numpy().tobytes() == b.rollout.reward.cpu().numpy().tobytes() and same(sa.pool.data, sb.pool.data)
    assert int(a.env.start_bad.item()) == 0 and int(sa.pool.bad.item()) == 0
    a.env.close(); b.env.close()
