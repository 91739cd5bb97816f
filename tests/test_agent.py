"""deepmimic_amd/agent.py on the GPU: PPO on humanoid3d_walk (plain nets) and AMP on amp_heading_zombie (gated actor and critic, a 3-column goal), N = 64 envs,
T = 8 steps, minibatches of 128, the reference's widths; AMP stores of 300 rows (fewer than T x N = 512: appends overwrite) and discriminator batches of 32.
Everything is compared as bytes: the learner has no tolerance of its own to state, each piece is held to its arithmetic by its own tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

from deepmimic_amd import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, M = 8, 64, 128
PLAIN, GATED = "fc_2layers_1024units", "fc_2layers_gated_1024units"
EXP = {"ExpParamsBeg": {"Rate": 0.5, "Noise": 0.05}, "ExpParamsEnd": {"Rate": 0.5, "Noise": 0.05}}
# the stepsizes and coefficients of data/agents/ct_agent_humanoid_ppo.txt / ct_agent_humanoid_amp_tasks.txt; InitSamples 0: the first rollout trains
PPO = dict({"AgentType": "PPO", "ActorNet": PLAIN, "ActorStepsize": 2e-6, "ActorMomentum": 0.9, "ActorWeightDecay": 0.0005, "ActorInitOutputScale": 0.01,
            "CriticNet": PLAIN, "CriticStepsize": 0.0005, "CriticMomentum": 0.9, "Discount": 0.95, "BatchSize": 4096, "MiniBatchSize": 256, "Epochs": 1,
            "InitSamples": 0, "NormalizerSamples": 1000000, "RatioClip": 0.2, "NormAdvClip": 4, "TDLambda": 0.95, "ExpAnnealSamples": 64000000}, **EXP)
AMP = dict({"AgentType": "AMP", "ActorNet": GATED, "ActorStepsize": 4e-6, "ActorMomentum": 0.9, "ActorWeightDecay": 0.0005, "ActorInitOutputScale": 0.01,
            "CriticNet": GATED, "CriticStepsize": 2e-5, "CriticMomentum": 0.9, "Discount": 0.99, "BatchSize": 4096, "MiniBatchSize": 256, "Epochs": 1,
            "InitSamples": 0, "NormalizerSamples": 1000000, "RatioClip": 0.2, "NormAdvClip": 4, "TDLambda": 0.95, "TaskRewardLerp": 0.5, "DiscNet": PLAIN,
            "DiscInitOutputScale": 1, "DiscStepSize": 1e-5, "DiscMomentum": 0.9, "DiscWeightDecay": 0.0005, "DiscLogitRegWeight": 0.05, "DiscGradPenalty": 10,
            "DiscBatchSize": 32, "DiscStepsPerBatch": 2, "DiscExpertBufferSize": 300, "DiscAgentBufferSize": 300, "RewardScale": 2, "ExpAnnealSamples": 200000000}, **EXP)
KINDS = {"ppo": ("humanoid3d_walk", PPO), "amp": ("amp_heading_zombie", AMP)}


def make(kind, hip_lib, seed=1, env_seed=7, **over):
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    asset, d = KINDS[kind]
    cfg = agent.AgentConfig.from_dict(dict(d, **{k: v for k, v in over.items() if k[0].isupper()}))
    env = TorchVecEnv(model.load_asset(asset), N, seed=env_seed, amp_obs=kind == "amp", lib_path=hip_lib)
    return agent.make_agent(env, cfg, rollout_steps=T, seed=seed, mini_batch_size=M, **{k: v for k, v in over.items() if not k[0].isupper()})


def snap(a) -> dict:
    """the learner as bytes: every trainer's whole buffer (masters, momentum, last gradients), the normalisers' statistics, and for AMP the reward bounds and both
    stores with their state words"""
    out = {}
    for name, tr in a.trainers().items():
        out["masters_" + name] = tr.buf[0].cpu().numpy().tobytes(); out["buf_" + name] = tr.buf.cpu().numpy().tobytes()
    for k, n in a._state_norms().items():
        st = n.state_host()
        out["norm_" + k] = b"".join(np.asarray(st[f]).tobytes() for f in ("mean", "std", "mean_sq")) + np.int64(st["count"]).tobytes()
    if a.KIND == "AMP":
        out["bounds"] = a.amp.bounds.cpu().numpy().tobytes()
        for name, st in (("agent", a.agent_store), ("expert", a.expert_store)):
            out["store_state_" + name] = st.state.cpu().numpy().tobytes(); out["store_rows_" + name] = st.buf.cpu().numpy().tobytes()
    return out


def differing(x: dict, y: dict) -> list:
    assert x.keys() == y.keys()
    return [k for k in x if x[k] != y[k]]


def compose_iteration_by_hand(b, k):
    """Iteration 0 on agent b's freshly built pieces and its env, written out from the pieces' own interfaces in the order of INTEGRATION.md section 4 and keyed by
    `k` alone: no method of the agent's sampling or update code runs."""
    import torch
    from deepmimic_amd import ppo_batch, returns
    from deepmimic_amd.binding import stream_handle
    env, c, G, amp = b.env, b.cfg, b.G, b.KIND == "AMP"
    dev = env.device
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    obs_all, goal_all = torch.zeros((T + 1, N, b.S), **f32), (torch.zeros((T + 1, N, G), **f32) if G else None)
    tobs, tgoal, task = torch.zeros((T, N, b.S), **f32), (torch.zeros((T, N, G), **f32) if G else None), torch.zeros((T, N), **f32)
    terminate, done, valid, flags = (torch.zeros((T, N), **i32) for _ in range(4))
    act, logp = torch.zeros((T, N, b.A), **f32), torch.zeros((T, N), **f32)
    amp_all = torch.zeros((T, N, b.AMP), **f32) if amp else None
    stream = stream_handle(dev)
    norms = [b.s_norm] + ([b.g_norm] if G else []) + ([b.amp_norm] if amp else [])
    for n in norms:
        n.set_stream(stream)
    rate = c.exp_params(0)[0]
    for t in range(T):
        obs_all[t] = env.obs
        if G:
            goal_all[t] = env.goal
        b.actor.forward_device_ex(obs_all[t].data_ptr(), N, act[t].data_ptr(), goal_all[t].data_ptr() if G else 0, G, logp_ptr=logp[t].data_ptr(),
                                  exp_flags_ptr=flags[t].data_ptr(), exp_rate=rate, sample=True, seed=k["actor_seed"], step=k["actor_step0"] + t, stream=stream)
        _, r, d, info = env.step(act[t])
        task[t], terminate[t], done[t], valid[t], tobs[t] = r, info["terminate"], d.to(torch.int32), info["valid"], info["terminal_obs"]
        if G:
            tgoal[t] = info["terminal_goal"]
        if amp:
            amp_all[t] = info["amp_obs"]
        b.s_norm.record_device(obs_all[t].data_ptr(), N)
        if G:
            b.g_norm.record_device(goal_all[t].data_ptr(), N)
    obs_all[T] = env.obs
    if G:
        goal_all[T] = env.goal
    rewards, bounds = task, None
    if amp:                                              # the discriminator first (amp_agent.py:299-306)
        zero = torch.zeros((T + 1, N), **f32)
        _, mask0 = returns.td_lambda_returns_torch(task, zero, zero[:T], terminate, done, valid, c.discount, c.td_lambda, 0.0, 0.0)
        lists = ppo_batch.advantages_torch(task, zero, mask0)
        n_valid, _ = lists.counts_host()
        assert n_valid > 0
        packed = torch.zeros((T * N, b.AMP), **f32)
        b.agent_store.append_calls = b.expert_store.append_calls = k["append_call"]
        b.agent_store.append_batch(amp_all, lists, packed=packed)
        env.expert_draw_calls = k["expert_draw_call"]
        expert = env.amp_expert_draw(n_valid)
        b.expert_store.append(expert)
        b.amp_norm.record_device(packed.data_ptr(), n_valid); b.amp_norm.record_device(expert.data_ptr(), n_valid)
        for step in range(-(-c.disc_steps_per_batch * n_valid // c.disc_batch_size)):
            b.agent_store.sample_calls = b.expert_store.sample_calls = k["sample_call0"] + step
            agent_rows, expert_rows = b.agent_store.sample(c.disc_batch_size), b.expert_store.sample(c.disc_batch_size)
            b.disc_tr.grad(expert_rows, agent_rows, grad_penalty=c.disc_grad_penalty, logit_reg=c.disc_logit_reg_weight)
            b.disc_tr.step()
        rewards, _ = b.amp.update_from_disc(b.disc, amp_all, task, done, valid)
        bounds = b.amp
    ret, mask, values = returns.critic_returns_torch(b.critic, obs_all, goal_all, tobs, tgoal, terminate, done, valid, rewards, c.discount, c.td_lambda,
                                                     return_values=True, bounds=bounds)
    batch = ppo_batch.advantages_torch(ret, values, mask, flags, adv_eps=1e-5, norm_adv_clip=c.norm_adv_clip, val_min=0.0, val_max=1.0 / (1.0 - c.discount))
    goals = [goal_all[:T]] if G else []
    critic_cols, actor_cols = [obs_all[:T]] + goals + [batch.targets], [obs_all[:T]] + goals + [act, logp, batch.adv]
    offs = env.env.offsets_scales()
    count = 0
    for e, mb, cr, ar in batch.minibatches(M, c.epochs, k["gather_seed"], critic_cols, actor_cols):
        assert k["gather_epoch0"] == 0
        b.critic_tr.grad(cr[0], cr[-1], goals=cr[1] if G else None); b.critic_tr.step()
        assert ar is not None
        b.actor_tr.grad(ar[0], ar[-3], ar[-2], ar[-1], goals=ar[1] if G else None, ratio_clip=c.ratio_clip, bound_weight=10.0,
                        a_bound_min=offs["action_min"].astype(np.float32), a_bound_max=offs["action_max"].astype(np.float32))
        b.actor_tr.step()
        count += 1
    assert count == c.epochs * -(-batch.counts_host()[0] // M)
    for n in norms:                                      # rl_agent.py:540-542
        n.update()
    return batch.counts_host()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_one_iteration_is_the_pieces_composed_by_hand(hip_lib, kind):
    a = make(kind, hip_lib)
    start = snap(a)
    row = a.iterate()
    b = make(kind, hip_lib)                              # a second env of the same seed, the same freshly built pieces
    assert differing(snap(b), start) == []
    n_valid, n_exp = compose_iteration_by_hand(b, a.keys(0))
    assert differing(snap(a), snap(b)) == []
    moved = differing(snap(a), start)
    assert {"masters_actor", "masters_critic", "norm_s"} <= set(moved), moved
    if kind == "amp":
        assert {"masters_disc", "norm_g", "norm_amp", "bounds", "store_state_agent", "store_state_expert", "store_rows_agent"} <= set(moved), moved
        assert a.agent_store.state_host() == (300, n_valid) and row["Disc_Steps"] == -(-2 * n_valid // 32)
        assert np.isfinite([row[k] for k in ("Disc_Loss", "Disc_Reward_Mean", "Disc_Reward_Std", "Grad_Penalty")]).all()
    assert row["Samples"] == n_valid and 0 < n_exp < n_valid and row["Iteration"] == 0 and a.iteration == 1
    assert list(row)[:len(a.columns())] == list(a.columns())
    assert np.isfinite([row[k] for k in ("Critic_Loss", "Actor_Loss", "Clip_Frac", "Adv_Mean", "Adv_Std", "State_Mean", "State_Std")]).all() and row["Adv_Std"] > 0
    # the keys are a function of (seed, iteration, position)
    k0, k1, other = a.keys(0), a.keys(1), keys_of_seed(a, 2)
    assert k1["actor_step0"] == T and k1["append_call"] == 1 and k1["expert_draw_call"] == 1 and k1["gather_epoch0"] == 1 and k1["actor_seed"] == k0["actor_seed"]
    assert other["actor_seed"] != k0["actor_seed"] and other["gather_seed"] != k0["gather_seed"]
    assert len({k0[s] for s in ("actor_seed", "gather_seed", "agent_store_seed", "expert_store_seed")}) == 4


def keys_of_seed(a, seed):
    """keys(0) of an agent of another seed, without building one: keys read the seed, T, the epochs and the discriminator's step budget alone"""
    import copy
    other = copy.copy(a)
    other.seed = seed
    return other.keys(0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_three_iterations_are_reproducible(hip_lib, kind):
    runs = []
    for seed in (1, 1, 2):
        a = make(kind, hip_lib, seed=seed)
        rows = a.train(3)
        runs.append((snap(a), [{k: v for k, v in r.items() if k != "Wall_Time"} for r in rows]))
        a.env.close()
    assert differing(runs[0][0], runs[1][0]) == [] and runs[0][1] == runs[1][1]
    diff = differing(runs[0][0], runs[2][0])
    assert {"masters_actor", "masters_critic"} <= set(diff), diff


@pytest.mark.gpu
def test_exploration_schedule(hip_lib):
    import torch
    a = make("ppo", hip_lib, ExpAnnealSamples=2 * T * N, ExpParamsBeg={"Rate": 1, "Noise": 0.05}, ExpParamsEnd={"Rate": 0.2, "Noise": 0.05})
    rows = a.train(3)
    assert [r["Samples"] for r in rows] == [T * N, 2 * T * N, 3 * T * N]
    assert [r["Exp_Rate"] for r in rows] == [1.0, a.cfg.exp_params(T * N)[0], 0.2] and rows[1]["Exp_Rate"] == pytest.approx(0.6)
    assert [r["Exp_Noise"] for r in rows] == [0.05] * 3 and a.exp_rate == 0.2
    # Rate 1: every valid sample explored (the first of the three rollouts above was sampled at Rate 1)
    one = make("ppo", hip_lib, ExpParamsBeg={"Rate": 1, "Noise": 0.05}, ExpParamsEnd={"Rate": 1, "Noise": 0.05})
    one.iterate()
    batch = one.last_batch
    n_valid, n_exp = batch.counts_host()
    assert n_valid == n_exp == T * N and torch.equal(batch.valid_idx[:n_valid], batch.exp_idx[:n_exp])
    # Rate 0: no explored sample -- the critic learns, the actor does not move
    zero = make("ppo", hip_lib, ExpParamsBeg={"Rate": 0, "Noise": 0.05}, ExpParamsEnd={"Rate": 0, "Noise": 0.05})
    start = snap(zero)
    row = zero.iterate()
    assert zero.last_batch.counts_host() == (T * N, 0)
    moved = differing(snap(zero), start)
    assert "masters_critic" in moved and "buf_actor" not in moved and row["Actor_Loss"] == 0.0 and row["Critic_Loss"] > 0


@pytest.mark.gpu
def test_normaliser_freeze_and_init_samples(hip_lib):
    a = make("amp", hip_lib, NormalizerSamples=T * N)
    s0 = snap(a)
    a.iterate(); s1 = snap(a)
    a.iterate(); s2 = snap(a)
    a.iterate(); s3 = snap(a)
    norms = ("norm_s", "norm_g", "norm_amp")
    assert set(norms) <= set(differing(s0, s1)) and a.s_norm.count == T * N and a.amp_norm.count == 2 * T * N
    assert not set(norms) & set(differing(s1, s2)) and not set(norms) & set(differing(s2, s3)) and not a.recording
    assert "masters_actor" in differing(s2, s3)
    # InitSamples = 2 T N: two rollouts feed the normalisers (and the stores) only
    b = make("amp", hip_lib, InitSamples=2 * T * N)
    nets = ("buf_actor", "buf_critic", "buf_disc")
    t0 = snap(b)
    r0 = b.iterate(); t1 = snap(b)
    r1 = b.iterate(); t2 = snap(b)
    r2 = b.iterate(); t3 = snap(b)
    assert not set(nets) & set(differing(t0, t1)) and not set(nets) & set(differing(t1, t2)) and set(nets) <= set(differing(t2, t3))
    assert {"norm_s", "norm_amp", "store_state_agent"} <= set(differing(t0, t1)) and "bounds" not in differing(t0, t2)
    assert (r0["Samples"], r1["Samples"], r2["Samples"]) == (T * N, 2 * T * N, 3 * T * N) and r0["Disc_Steps"] == r1["Disc_Steps"] == 0 < r2["Disc_Steps"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_empty_rollout_changes_nothing(hip_lib, kind):
    """`valid` zeroed and every step made an episode end: each sample then belongs to an episode that ended invalid, so the rollout has no valid sample"""
    a = make(kind, hip_lib)
    ro = a.collect()
    ro.valid.zero_(); ro.done.fill_(1)
    before = snap(a)
    info = a.update(ro)
    assert info == dict(n_valid=0, n_exp=0, minibatches=0) and a.empty_rollouts == 1
    assert differing(snap(a), before) == []


@pytest.mark.gpu
def test_critic_learns_on_a_frozen_rollout(hip_lib):
    a = make("ppo", hip_lib, ActorStepsize=0.0, ActorWeightDecay=0.0, CriticStepsize=0.01)        # 0.01: the stepsize of tests/test_train.py's training case
    ro = a.collect()
    actor0 = a.actor_tr.buf[0].clone()
    losses = []
    for _ in range(10):
        info = a.update(ro)
        assert info["minibatches"] == -(-info["n_valid"] // M)
        losses.append(a.update_losses()["Critic_Loss"])
    print("Critic_Loss over ten updates of one rollout:", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert (a.actor_tr.buf[0] == actor0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_save_model_reads_back_bit_for_bit(hip_lib, kind, tmp_path):
    import torch
    from deepmimic_amd import tf_checkpoint as tfc
    from deepmimic_amd.heads import Critic, Discriminator
    from deepmimic_amd.policy import Policy
    a = make(kind, hip_lib)
    a.iterate()
    prefix = str(tmp_path / "out" / "agent0_model.ckpt")
    a.save_model(prefix)
    idx = tfc.read_index(prefix + ".index")
    want = tfc.agent_variables(a.S, a.G, a.A, a.AMP, gated=kind == "amp", reward_scale=kind == "amp")
    assert {n: (np.dtype(tfc.DTYPES[e["dtype"]]), tuple(e["shape"])) for n, e in idx.items() if n} == want
    tensors = tfc.read_tensors(prefix, verify_below=None)
    assert tensors["agent/main/actor/0/dense/kernel"].tobytes() == a.actor_tr.views()["w1"].cpu().numpy().tobytes()
    assert tensors["agent/resource/s_norm/count"].tolist() == [T * N] and tensors["agent/resource/s_norm/mean_ph"].tobytes() == tensors["agent/resource/s_norm/mean"].tobytes()
    ro, G, n = a.rollout, a.G, 33
    states = ro.obs.reshape(-1, a.S)[5:5 + n].clone()
    goals = ro.goal.reshape(-1, G)[5:5 + n].clone() if G else None
    stream = torch.cuda.current_stream().cuda_stream

    def mode_actions(pol):
        out = torch.zeros((n, a.A), dtype=torch.float32, device=states.device)
        pol.forward_device_ex(states.data_ptr(), n, out.data_ptr(), goals.data_ptr() if G else 0, G, sample=False, stream=stream)
        return out.cpu().numpy()
    loaded = Policy.from_checkpoint(prefix, lib_path=hip_lib)
    assert loaded.gated == (kind == "amp")
    actions = mode_actions(a.actor)
    assert np.isfinite(actions).all() and actions.std() > 0 and actions.tobytes() == mode_actions(loaded).tobytes()
    critic = Critic.from_checkpoint(prefix, val_fail=a.val_fail, val_succ=a.val_succ, lib_path=hip_lib)
    v_live, v_loaded = a.critic.eval_torch(states, goals).cpu().numpy(), critic.eval_torch(states, goals).cpu().numpy()
    assert np.isfinite(v_live).all() and v_live.std() > 0 and v_live.tobytes() == v_loaded.tobytes()
    if kind == "amp":
        assert tensors["agent/reward_scale"].tolist() == [2.0]
        rows = ro.amp_obs.reshape(-1, a.AMP)[5:5 + n].clone()
        disc = Discriminator.from_checkpoint(prefix, reward_scale=2.0, task_reward_lerp=0.5, lib_path=hip_lib)
        live, back = a.disc.eval_torch(rows, raw=True), disc.eval_torch(rows, raw=True)
        for x, y in zip(live, back):
            assert np.isfinite(x.cpu().numpy()).all() and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert live[1].std() > 0
    # a third agent started from the file holds the saved masters and statistics
    c = make(kind, hip_lib, init_from=prefix)
    assert c.actor_tr.buf[0].cpu().numpy().tobytes() == a.actor_tr.buf[0].cpu().numpy().tobytes()
    assert mode_actions(c.actor).tobytes() == actions.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "amp"])
def test_save_state_resumes_byte_for_byte(hip_lib, kind, tmp_path):
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    path = str(tmp_path / "learner.npz")
    first = make(kind, hip_lib)
    first.train(2)
    first.save_state(path)
    asset, _ = KINDS[kind]
    env = TorchVecEnv(model.load_asset(asset), N, seed=7, amp_obs=kind == "amp", lib_path=hip_lib)
    arm1 = agent.PPOAgent.load_state(env, first.cfg, path) if kind == "ppo" else agent.AMPAgent.load_state(env, first.cfg, path)
    assert arm1.iteration == 2 and arm1.samples == first.samples and differing(snap(arm1), snap(first)) == []
    rows1 = arm1.train(2)
    arm2 = make(kind, hip_lib)
    arm2.train(2)
    arm2.restart_envs(2)
    rows2 = arm2.train(2)
    assert differing(snap(arm1), snap(arm2)) == []
    strip = lambda rows: [{k: v for k, v in r.items() if k != "Wall_Time"} for r in rows]
    assert strip(rows1) == strip(rows2) and [r["Iteration"] for r in rows1] == [2, 3]
    with pytest.raises(ValueError, match="saved learner"):
        arm2._set_state(dict(np.load(path), kind=np.array("PG")))


@pytest.mark.gpu
def test_test_episodes(hip_lib):
    """on the AMP scene: its train-mode episode limit (0.5 s at this sample count) and its test-mode limit (20 s) differ, so the limits tell the mode"""
    a = make("amp", hip_lib)
    a.iterate()
    before = snap(a)
    env = a.env.env
    train_limits = model.timer_limits(env.tables.cfg, False, a.samples)
    assert env._timer[1:3] == train_limits != model.timer_limits(env.tables.cfg, True, a.samples)
    ret = a.test(4)
    assert np.isfinite(ret) and ret == a.test_return and ret >= 0.0
    assert differing(snap(a), before) == []
    assert env._timer[1:3] == train_limits                                                # the train-mode episode limits are back
    row = a.iterate()
    assert row["Test_Return"] == ret and row["Iteration"] == 1


@pytest.mark.gpu
def test_refusals(hip_lib):
    from deepmimic_amd import agent
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 8, seed=1, lib_path=hip_lib)
    with pytest.raises(ValueError, match="amp_obs=True"):
        agent.AMPAgent(env, agent.AgentConfig.from_dict(AMP), rollout_steps=2)
    with pytest.raises(ValueError, match="gates on the goal"):
        agent.PPOAgent(env, agent.AgentConfig.from_dict(dict(PPO, ActorNet=GATED)), rollout_steps=2)
    with pytest.raises(ValueError, match="AgentType AMP"):
        agent.PPOAgent(env, agent.AgentConfig.from_dict(AMP), rollout_steps=2)
    with pytest.raises(TypeError, match="unknown optimiser option"):
        agent.PPOAgent(env, agent.AgentConfig.from_dict(PPO), rollout_steps=2, lr=1.0)


@pytest.mark.gpu
def test_optimiser_options_reach_the_trainers_and_the_log(hip_lib):
    a = make("ppo", hip_lib, optimizer="adam", max_grad_norm=1.0, skip_nonfinite=True, betas=(0.8, 0.9), eps=1e-6)
    assert a.actor_tr.optimizer == "adam" and a.critic_tr.betas == (0.8, 0.9) and a.actor_tr.eps == 1e-6 and a.actor_tr.max_grad_norm == 1.0
    row = a.iterate()
    assert a.columns()[-2:] == ("Skipped_Steps", "Grad_Norm") and row["Skipped_Steps"] == 0 and row["Grad_Norm"] > 0


@pytest.mark.gpu
def test_command_line(hip_lib, tmp_path):
    """two iterations in a fresh child process, from an arg file with the keys of args/train_humanoid3d_walk_args.txt that the learner reads, on the packaged asset"""
    import json
    from deepmimic_amd import agent, tf_checkpoint as tfc
    (tmp_path / "agent.txt").write_text(json.dumps(dict(PPO, OutputIters=1, IntOutputIters=1, TestEpisodes=2)))
    (tmp_path / "args.txt").write_text("--scene imitate\n--agent_files agent.txt\n\n--output_path output\n--int_output_path output/intermediate\n")
    cmd = [sys.executable, "-m", "deepmimic_amd.agent", "--arg_file", "args.txt", "--data_root", str(tmp_path), "--asset", "humanoid3d_walk", "--num_envs", str(N),
           "--rollout_steps", str(T), "--iterations", "2", "--mini_batch_size", str(M), "--seed", "3"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Train_Return" in p.stdout and p.stdout.count("| %16s |" % "Iteration") == 2
    log = np.genfromtxt(str(tmp_path / "output" / "agent0_log.txt"), names=True)
    assert log["Iteration"].tolist() == [0.0, 1.0] and log["Samples"].tolist() == [T * N, 2 * T * N] and log.dtype.names == agent.LOG_COLUMNS
    assert log["Test_Return"][0] == 0.0 and log["Test_Return"][1] > 0.0          # TestEpisodes: two test episodes in front of iteration 1 (IntOutputIters = 1)
    w = tfc.actor_weights(str(tmp_path / "output" / "agent0_model.ckpt"))
    assert w["w1"].shape[1] == 1024 and np.isfinite(w["w1"]).all() and w["s_mean"].size == w["w1"].shape[0]
    assert sorted(os.listdir(tmp_path / "output" / "intermediate" / "agent0_models")) == [
        "agent0_int_model_%010d.ckpt.%s" % (i, s) for i in (0, 1) for s in ("data-00000-of-00001", "index")]
