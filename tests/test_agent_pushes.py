"""`make_agent(..., push_fn=)` on the GPU (deepmimic_amd/agent.py, deepmimic_amd/pushes.py), at the sizes of tests/test_agent.py (N = 64, T = 8): one iteration with
a push sampler is the iteration composed by hand with the same pushes in front of every env.step; two agents of one seed hold the same bytes; without push_fn the
agent is the one tests/test_agent.py composes by hand."""
import pytest

from deepmimic_amd import model
from test_agent import KINDS, M, N, T, compose_iteration_by_hand, differing, snap

pytestmark = pytest.mark.gpu
SAMPLER = dict(interval=(2, 5), magnitude=(50.0, 150.0), duration=(0.05, 0.2), seed=3)


def make(kind, hip_lib, pushes=True, sampler=None, seed=1, env_seed=7):
    from deepmimic_amd import agent
    from deepmimic_amd.pushes import RandomPushes
    from deepmimic_amd.vec_env import TorchVecEnv
    asset, d = KINDS[kind]
    env = TorchVecEnv(model.load_asset(asset), N, seed=env_seed, amp_obs=kind == "amp", lib_path=hip_lib, pushes=pushes)
    fn = RandomPushes(env, **sampler) if sampler else None
    return agent.make_agent(env, agent.AgentConfig.from_dict(d), rollout_steps=T, seed=seed, mini_batch_size=M, push_fn=fn), fn


@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_one_iteration_with_pushes_is_composed_by_hand(hip_lib, kind):
    from deepmimic_amd.pushes import RandomPushes
    a, fn = make(kind, hip_lib, sampler=SAMPLER)
    seen = []
    fired = []

    def hook(info, t):
        seen.append((t, sorted(info)))
        push = fn(info, t)
        fired.append(push["mask"].clone())
        return push
    a.push_fn = hook
    a.iterate()
    assert [t for t, _ in seen] == list(range(T)) and sum(int(m.sum()) for m in fired) >= N      # (an interval of 2 .. 5 steps in 8: every env was pushed)
    assert seen[0][1] == sorted(["obs", "pushes"] + (["goal"] if a.G else [])) and {"obs", "pushes", "terminate", "valid", "terminal_obs"} <= set(seen[1][1])
    b, _ = make(kind, hip_lib)                                               # the same env and pieces, no hook: the pushes go in front of env.step by hand
    again, step = RandomPushes(b.env, **SAMPLER), b.env.step

    def pushed_step(actions):
        b.env.push(**again(None, None))
        return step(actions)
    b.env.step = pushed_step
    compose_iteration_by_hand(b, a.keys(0))
    assert differing(snap(a), snap(b)) == []
    assert a.env.env.get_perturb_state().tobytes() == b.env.env.get_perturb_state().tobytes()
    c, _ = make(kind, hip_lib)                                               # never pushed: another rollout
    c.iterate()
    assert "masters_actor" in differing(snap(a), snap(c))
    for x in (a, b, c):
        x.env.close()


def test_two_agents_of_one_seed_hold_the_same_bytes(hip_lib):
    runs = []
    for sampler_seed in (3, 3, 4):
        a, _ = make("ppo", hip_lib, sampler=dict(SAMPLER, seed=sampler_seed))
        a.iterate()
        runs.append(snap(a))
        a.env.close()
    assert differing(runs[0], runs[1]) == [] and "masters_actor" in differing(runs[0], runs[2])


def test_without_push_fn_the_agent_is_the_one_composed_by_hand(hip_lib):
    """push_fn=None on an env without pushes: the bytes of the iteration written out from the pieces, which knows nothing of pushes"""
    a, _ = make("ppo", hip_lib, pushes=False)
    assert a.push_fn is None and a.env.pushes is None
    a.iterate()
    b, _ = make("ppo", hip_lib, pushes=False)
    compose_iteration_by_hand(b, a.keys(0))
    assert differing(snap(a), snap(b)) == []
    a.env.close(); b.env.close()


def test_push_fn_needs_an_env_with_pushes(hip_lib):
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    asset, d = KINDS["ppo"]
    env = TorchVecEnv(model.load_asset(asset), N, seed=7, lib_path=hip_lib)
    with pytest.raises(ValueError, match="pushes=True"):
        agent.make_agent(env, agent.AgentConfig.from_dict(d), rollout_steps=T, seed=1, mini_batch_size=M, push_fn=lambda info, t: None)
    env.close()
