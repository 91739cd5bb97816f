"""The device-resident sampler loop of INTEGRATION.md section 4 (tests/test_sampler_loop.py) on task scenes with the actor their agent files name: the gated
net (fc_2layers_gated_1024units), goal from the env as the policy's goal block, g_norm bound at column S.  GPU only: everything is device pointers."""
import numpy as np
import pytest

from deepmimic_amd import model


def _check_first_step(w, cat, A, a, lp, fl, info):
    """tests/test_sampler_loop.py _check_first_step with the gated float64 statement (tests/test_policy_gated.py gated_actor_f64) and its bounds"""
    from test_policy_kernels import FUSED_8_2, FUSED_8_4, coin_f64, noise_f64, HALF_LOG_2PI
    from test_policy_gated import gated_actor_f64
    from deepmimic_amd.policy import reference_forward
    n = cat.shape[0]
    assert info["gated"] and info["goal_dim"] == w["goal_dim"] and info["gated_fused"] and info["path"] in (FUSED_8_2, FUSED_8_4) and info["rows"] == n, info     # (path id, gated): the one-launch gated actor
    ex = coin_f64(77, np.arange(n), 0) < 0.5
    assert np.array_equal(fl != 0, ex)
    noise = np.where(ex[:, None], noise_f64(77, np.arange(n), 0, A), 0.0)
    add = noise * np.exp(w["logstd"].astype(np.float64)) * w["a_std"]
    want_64 = gated_actor_f64(w, cat, 10.0)["a"] + add
    want_bf = reference_forward(w, cat, s_clip=10.0, bf16=True)[0] + add
    scale = np.abs(want_64).max()
    assert np.abs(a - want_bf).max() < 2e-3 * scale, (np.abs(a - want_bf).max(), scale)
    assert np.abs(a - want_64).max() < 2e-2 * scale, (np.abs(a - want_64).max(), scale)
    want_lp = (-0.5 * noise ** 2 - w["logstd"]).sum(1) - A * HALF_LOG_2PI
    assert np.abs(lp - want_lp).max() < 2e-2 * max(1.0, np.abs(want_lp).max() / 10), np.abs(lp - want_lp).max()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["amp_heading_zombie", "amp_target_zombie"])
def test_device_resident_sampler_loop_gated_actor(hip_lib, scene):
    import torch
    from deepmimic_amd.normalizer import DeviceNormalizer
    from deepmimic_amd.policy import Policy, random_weights
    from deepmimic_amd.vec_env import TorchVecEnv
    t = model.load_asset(scene)
    n = 256
    env = TorchVecEnv(t, n, seed=3, lib_path=hip_lib)
    obs = env.reset()
    S, G, A = env.obs_dim, env.goal_dim, env.act_dim
    assert G > 0
    offs = env.env.offsets_scales()
    s_norm = DeviceNormalizer(S, groups_ids=offs["state_norm_groups"], clip=10.0, lib_path=hip_lib)
    s_norm.set_mean_std(-offs["state_offset"], 1.0 / offs["state_scale"])
    g_norm = DeviceNormalizer(G, clip=10.0, lib_path=hip_lib)
    w = random_weights(S + G, A, seed=1, gated_goal_dim=G)
    w["w1"][S:, :] = 0.0             # the goal reaches this net through the gate alone: what moves with g_norm below moved through the gate
    w["a_mean"] = -offs["action_offset"].astype(np.float32); w["a_std"] = (1.0 / offs["action_scale"]).astype(np.float32)
    actor = Policy(w, s_clip=10.0, lib_path=hip_lib)
    assert actor.info()["gated"] and actor.info()["goal_dim"] == G
    s_norm.bind_policy(actor)
    g_norm.bind_policy(actor, first_column=S)
    dev = obs.device
    actions = torch.zeros((n, A), device=dev); logp = torch.zeros(n, device=dev); flags = torch.zeros(n, dtype=torch.int32, device=dev)
    probe = [torch.zeros((n, A), device=dev), torch.zeros((n, A), device=dev)]
    goal = torch.zeros((n, G), device=dev)
    goal.copy_(torch.from_numpy(env.env.query_goal()).to(dev))
    iters, steps, explored = 3, 12, 0
    w_ref = dict(w); w_ref["s_mean"] = np.concatenate([s_norm.mean, g_norm.mean]); w_ref["s_std"] = np.concatenate([s_norm.std, g_norm.std])
    cat0 = np.concatenate([obs.cpu().numpy(), goal.cpu().numpy()], axis=1)
    for it in range(iters):
        for k in range(steps):
            actor.forward_device_ex(obs.data_ptr(), n, actions.data_ptr(), goals_ptr=goal.data_ptr(), goal_dim=G, logp_ptr=logp.data_ptr(),
                                    exp_flags_ptr=flags.data_ptr(), exp_rate=0.5, sample=True, seed=77, step=it * steps + k)
            explored += int(flags.sum().item())
            if it == 0 and k == 0:
                _check_first_step(w_ref, cat0, A, actions.cpu().numpy(), logp.cpu().numpy(), flags.cpu().numpy(), actor.info())
            obs, reward, done, info = env.step(actions)
            goal = info["goal"]
            s_norm.record_device(obs.data_ptr(), n)
            g_norm.record_device(goal.data_ptr(), n)
            assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(actions).all()) and bool(torch.isfinite(logp).all())
        s_norm.update(); s_norm.bind_policy(actor)
        # the mode action on the same observations and goals before and after g_norm alone is re-bound: the gate's input changed, with no further call
        actor.forward_device_ex(obs.data_ptr(), n, probe[0].data_ptr(), goals_ptr=goal.data_ptr(), goal_dim=G)
        g_norm.update(); g_norm.bind_policy(actor, first_column=S)
        actor.forward_device_ex(obs.data_ptr(), n, probe[1].data_ptr(), goals_ptr=goal.data_ptr(), goal_dim=G)
        assert g_norm.count == (it + 1) * steps * n and s_norm.count == (it + 1) * steps * n
        assert bool(torch.isfinite(probe[1]).all()) and float((probe[0] - probe[1]).abs().max().item()) > 0.0
    assert 0.4 < explored / (iters * steps * n) < 0.6
    assert np.isfinite(g_norm.mean).all() and g_norm.std.min() >= 0.02 and float(reward.mean().item()) >= 0.0
    g_norm.close(); env.close(); actor.close(); s_norm.close()
