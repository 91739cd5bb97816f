"""`PPOAgent` / `AMPAgent` with `goal_fn` (deepmimic_amd/agent.py) on the GPU, at the shapes of tests/test_agent.py (N = 64, T = 8, M = 128).  The goal block is two
lookahead frames of the reference motion (TorchVecEnv(kin_lookahead=...)) in the character's heading frame: three link positions per frame relative to the
simulated root, G = 18.  Episodes are pinned to 0.1 s, so every env ends in its fourth and eighth step.

* a start sampler that gives nothing sees the end of the step before any env is reset: the goal computed from info there equals the goal computed from a fresh
  dm_kin_query / dm_link_state of the context, and no episode counter has moved
* rollout.terminal_goal[t] holds exactly those bytes (goal_fn on the end-of-step tensors, called when the done envs have been reset already); rollout.goal[t + 1] is
  goal_fn behind update_link_state(), equal to the goal of the context as it then stands: done envs in their new episode, the others the same bytes as before
* two agents of one seed hold the same bytes after two iterations and a test run; save_model reads back through Policy / Critic.from_checkpoint; the ValueErrors"""
import numpy as np
import pytest

from deepmimic_amd import model
from test_agent import AMP, M, N, PPO, T, differing, snap

pytestmark = pytest.mark.gpu
OFFSETS = (1.0 / 30, 2.0 / 30)
G = len(OFFSETS) * 3 * 3


def heading_frames(torch, links, ahead_links, pose, link_env):
    pos = ahead_links[:, :, links, 0:3] - pose[:, None, None, 0:3]              # [N, K, 3 links, 3]
    h = link_env[:, 6].reshape(-1, 1, 1)
    c, s = torch.cos(h), torch.sin(h)                                           # rot_y(-heading): the origin frame of the observation
    return torch.stack([c * pos[..., 0] - s * pos[..., 2], pos[..., 1], s * pos[..., 0] + c * pos[..., 2]], dim=-1).reshape(pos.shape[0], -1)


def make(kind, hip_lib, log=None, end_log=None, seed=1, **kw):
    """log: every goal_fn call appends its result, the goal computed from a fresh dm_kin_query / dm_link_state of the context, and the episode counters.
    end_log: a start sampler that gives nothing (the device draws, as without one) appends the same at the moment `step` calls it: the end of the step, before
    the done envs are reset."""
    import torch
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    t = model.load_asset("humanoid3d_walk")
    if kind == "amp":
        t.cfg.scene = "imitate_amp"
    t.cfg.time_lim_min = t.cfg.time_lim_max = 0.1
    env = TorchVecEnv(t, N, seed=7, amp_obs=kind == "amp", link_state=True, deferred_reset=True, kin_lookahead=OFFSETS, lib_path=hip_lib)
    links = [0, env.link_names.index("right_wrist"), env.env.J - 1]
    times = torch.tensor(OFFSETS, dtype=torch.float64, device=env.device)

    def of_info(info):
        return heading_frames(torch, links, info["kin_ahead_link_state"], info["pose"], info["link_env"])

    def of_context():
        direct, sim = env.kin_query(times), env.env.link_state(0)
        g = heading_frames(torch, links, direct["link_state"], torch.from_numpy(sim["pose"]).to(env.device), torch.from_numpy(sim["env"]).to(env.device))
        return dict(fresh=g.cpu().numpy(), ep=env.env.get_state()["flags"][:, 2].copy())

    def goal_fn(info):
        g = of_info(info)
        if log is not None:
            log.append(dict(of_context(), g=g.cpu().numpy().copy()))
        return g

    def sampler(done_i32, info):
        end_log.append(dict(of_context(), g=of_info(info).cpu().numpy().copy(), done=done_i32.cpu().numpy() != 0))
        return {}

    if end_log is not None:
        env.set_start_sampler(sampler)
    cfg = agent.AgentConfig.from_dict(dict(AMP if kind == "amp" else PPO))
    return agent.make_agent(env, cfg, rollout_steps=T, seed=seed, mini_batch_size=M, goal_fn=goal_fn, goal_dim=G, **kw)


@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_rollout_goals_come_from_the_right_moment(hip_lib, kind):
    log, end_log = [], []
    a = make(kind, hip_lib, log, end_log)
    assert a.G == G and a.g_norm is not None and len(log) == 1 and not end_log          # (the goal behind the first reset)
    ro = a.collect()
    assert len(log) == 1 + 2 * T and len(end_log) == T
    goal, term, done = ro.goal.cpu().numpy(), ro.terminal_goal.cpu().numpy(), ro.done.cpu().numpy() != 0
    assert goal.shape == (T + 1, N, G) and term.shape == (T, N, G) and np.isfinite(goal).all() and np.isfinite(term).all()
    assert goal[0].tobytes() == log[0]["g"].tobytes() == log[0]["fresh"].tobytes()
    assert done.any() and not done.all()
    for t in range(T):
        prev, at_end, end, new = log[2 * t], end_log[t], log[1 + 2 * t], log[2 + 2 * t]
        d = done[t]
        assert (at_end["done"] == d).all(), t
        # the end of the step, before the reset: the info tensors are the context's, no episode counter has moved
        assert at_end["g"].tobytes() == at_end["fresh"].tobytes() and (at_end["ep"] == prev["ep"]).all(), t
        # the terminal goal is goal_fn on those tensors -- though the done envs have been reset by the time it is called
        assert term[t].tobytes() == end["g"].tobytes() == at_end["g"].tobytes(), t
        assert (end["ep"][d] == prev["ep"][d] + 1).all() and (end["ep"][~d] == prev["ep"][~d]).all(), t
        # the goal the next action is taken from: behind update_link_state() the tensors are the context's again, done envs in their new episode
        assert goal[t + 1].tobytes() == new["g"].tobytes() == new["fresh"].tobytes() and (new["ep"] == end["ep"]).all(), t
        assert new["g"][~d].tobytes() == end["g"][~d].tobytes(), t        # the other envs recompute the same bytes
        if d.any():
            assert not (new["g"][d] == end["g"][d]).all(axis=1).any(), t
    assert goal.std() > 0
    a.env.close()


@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_two_agents_of_one_seed_hold_the_same_bytes(hip_lib, kind):
    a, b = make(kind, hip_lib), make(kind, hip_lib)
    for _ in range(2):
        ra, rb = a.iterate(), b.iterate()
    assert differing(snap(a), snap(b)) == []
    for x, y in ((a.rollout.goal, b.rollout.goal), (a.rollout.terminal_goal, b.rollout.terminal_goal), (a.rollout.reward, b.rollout.reward)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    st = a.g_norm.state_host()
    assert int(st["count"]) == 2 * T * N and np.abs(st["mean"]).max() > 0            # the goal normaliser recorded the goal block
    assert a.test(2) == b.test(2) and np.isfinite(a.test_return)
    a.env.close(); b.env.close()


@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_save_model_reads_back(hip_lib, kind, tmp_path):
    import torch
    from deepmimic_amd import tf_checkpoint as tfc
    from deepmimic_amd.heads import Critic
    from deepmimic_amd.policy import Policy
    a = make(kind, hip_lib)
    a.iterate()
    prefix = str(tmp_path / "out" / "agent0_model.ckpt")
    a.save_model(prefix)
    idx = tfc.read_index(prefix + ".index")
    want = tfc.agent_variables(a.S, a.G, a.A, a.AMP, gated=kind == "amp", reward_scale=kind == "amp")
    assert {n: (np.dtype(tfc.DTYPES[e["dtype"]]), tuple(e["shape"])) for n, e in idx.items() if n} == want
    ro, n = a.rollout, 33
    states, goals = ro.obs.reshape(-1, a.S)[5:5 + n].clone(), ro.goal.reshape(-1, G)[5:5 + n].clone()
    stream = torch.cuda.current_stream().cuda_stream

    def mode_actions(pol):
        out = torch.zeros((n, a.A), dtype=torch.float32, device=states.device)
        pol.forward_device_ex(states.data_ptr(), n, out.data_ptr(), goals.data_ptr(), G, sample=False, stream=stream)
        return out.cpu().numpy()
    loaded = Policy.from_checkpoint(prefix, lib_path=hip_lib)
    assert loaded.gated == (kind == "amp")
    actions = mode_actions(a.actor)
    assert np.isfinite(actions).all() and actions.std() > 0 and actions.tobytes() == mode_actions(loaded).tobytes()
    critic = Critic.from_checkpoint(prefix, val_fail=a.val_fail, val_succ=a.val_succ, lib_path=hip_lib)
    v_live, v_loaded = a.critic.eval_torch(states, goals).cpu().numpy(), critic.eval_torch(states, goals).cpu().numpy()
    assert np.isfinite(v_live).all() and v_live.std() > 0 and v_live.tobytes() == v_loaded.tobytes()
    c = make(kind, hip_lib, init_from=prefix)
    assert c.actor_tr.buf[0].cpu().numpy().tobytes() == a.actor_tr.buf[0].cpu().numpy().tobytes()
    assert mode_actions(c.actor).tobytes() == actions.tobytes()
    a.env.close(); c.env.close()


def test_value_errors(hip_lib):
    import torch
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    cfg = agent.AgentConfig.from_dict(dict(PPO))
    fn = lambda info: torch.zeros((8, 4), device="cuda")
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 8, seed=1, lib_path=hip_lib)
    with pytest.raises(ValueError, match="goal_fn needs TorchVecEnv\\(..., deferred_reset=True\\)"):
        agent.make_agent(env, cfg, rollout_steps=2, goal_fn=fn, goal_dim=4)
    with pytest.raises(ValueError, match="goal_dim without goal_fn"):
        agent.make_agent(env, cfg, rollout_steps=2, goal_dim=4)
    env.close()
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 8, seed=1, link_state=True, deferred_reset=True, lib_path=hip_lib)
    with pytest.raises(ValueError, match="goal_fn needs goal_dim >= 1"):
        agent.make_agent(env, cfg, rollout_steps=2, goal_fn=fn)
    with pytest.raises(ValueError, match="goal_fn's result must be a float32 tensor of shape \\(8, 5\\)"):
        agent.make_agent(env, cfg, rollout_steps=2, goal_fn=fn, goal_dim=5)
    env.close()
    env = TorchVecEnv(model.load_asset("amp_heading_zombie"), 8, seed=1, amp_obs=True, link_state=True, deferred_reset=True, lib_path=hip_lib)
    with pytest.raises(ValueError, match="goal_fn: the scene has a goal of its own"):
        agent.make_agent(env, agent.AgentConfig.from_dict(dict(AMP)), rollout_steps=2, goal_fn=fn, goal_dim=4)
    env.close()
