"""`TorchVecEnv(..., link_state=True, deferred_reset=True)` on the GPU (deepmimic_amd/vec_env.py, deepmimic_amd/link_state.py): the step that resets finished envs
with dm_reset_where behind the link-state launches returns, byte for byte, what the step with the in-kernel auto-reset returns -- and its link-state rows describe the
END of the step for every env: until (and in) the first step in which an env ends they are the link state of a context that is stepped with the same actions and
never reset.  N = 4, 8 control steps, episodes pinned to 0.1 s (every env ends in its fourth and eighth step); plain, imitate_amp and a multi-clip goal scene."""
import numpy as np
import pytest

from deepmimic_amd import model

pytestmark = pytest.mark.gpu
N, STEPS, SEED = 4, 8, 17


def tables(scene):
    t = model.load_asset("amp_heading_clips4" if scene == "amp_heading_clips4" else "humanoid3d_walk")
    if scene == "imitate_amp":
        t.cfg.scene = "imitate_amp"
    t.cfg.time_lim_min = t.cfg.time_lim_max = 0.1
    return t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("scene", ["plain", "imitate_amp", "amp_heading_clips4"])
def test_deferred_step_equals_auto_reset_step(hip_lib, scene):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    amp = scene != "plain"
    kw = dict(seed=SEED, amp_obs=amp, episode_stats=True, lib_path=hip_lib)
    a = TorchVecEnv(tables(scene), N, **kw)
    b = TorchVecEnv(tables(scene), N, link_state=True, kin_link_state=True, deferred_reset=True, **kw)
    c = TorchVecEnv(tables(scene), N, link_state=True, **kw)           # stepped below through BatchEnv.step_device without auto-reset, never reset
    assert b.link_names == list(a.env.tables.joint_names) and len(b.link_names) == a.env.J
    oa, ob = a.reset(), b.reset()
    c.reset()
    assert same(oa, ob)
    gen = torch.Generator(device="cpu").manual_seed(3)
    keys = ["terminate", "valid", "goal", "terminal_obs", "terminal_goal", "episode_return", "episode_length"] + (["amp_obs"] if amp else [])
    ended_once, total_done = False, 0
    for k in range(STEPS):
        act = (0.1 * torch.randn((N, a.act_dim), generator=gen)).to(a.device)
        ra, rb = a.step(act), b.step(act)
        for name, x, y in (("obs", ra[0], rb[0]), ("reward", ra[1], rb[1]), ("done", ra[2], rb[2])):
            assert same(x, y), (k, name)
        for key in keys:
            assert (key in ra[3]) == (key in rb[3]), key
            if key in ra[3]:
                assert same(ra[3][key], rb[3][key]), (k, key)
        assert set(rb[3]) - set(ra[3]) == {"link_state", "link_env", "pose", "vel", "kin_link_state", "kin_link_env", "kin_pose", "kin_vel"}
        total_done += int(ra[2].sum())
        if not ended_once:
            c._enter()
            c.env.step_device(act.data_ptr(), c.obs.data_ptr(), c.reward.data_ptr(), c.terminate.data_ptr(), c.valid.data_ptr(), c.episode_end.data_ptr(),
                              timestep=c.timestep, n_updates=c.updates, auto_reset=False, end_early=True, amp_ptr=c.amp_obs.data_ptr() if amp else 0)
            want = c.update_link_state()
            for key in ("link_state", "link_env", "pose", "vel"):
                assert same(rb[3][key], want[key]), (k, key)
            assert same(c.reward, rb[1])
            ended_once = bool(ra[2].any())                                # this step included: the rows of the finished envs are their terminal state
    assert ended_once and total_done >= 2 * N, total_done
    for e in (a, b, c):
        e.close()


def test_options_off_launch_nothing_new(hip_lib, monkeypatch):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(tables("plain"), N, seed=SEED, lib_path=hip_lib)
    lib, calls = env.env.lib, {"dm_link_state": 0, "dm_reset_where": 0}
    for name in calls:
        real = getattr(lib, name)

        def counting(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    env.reset()
    act = torch.zeros((N, env.act_dim), device=env.device)
    for _ in range(4):
        _, _, _, info = env.step(act)
    assert calls == {"dm_link_state": 0, "dm_reset_where": 0}
    assert not any(k.endswith(("link_state", "link_env", "pose", "vel", "obj_state")) for k in info)
    with pytest.raises(RuntimeError, match="update_link_state needs"):
        env.update_link_state()
    env.close()
    # (the wrapper counts: the same steps with the options on go through both entry points)
    on = TorchVecEnv(tables("plain"), N, seed=SEED, link_state=True, kin_link_state=True, deferred_reset=True, lib_path=hip_lib)
    on.reset()
    for _ in range(4):
        on.step(act)
    assert calls == {"dm_link_state": 8, "dm_reset_where": 4}
    on.close()
