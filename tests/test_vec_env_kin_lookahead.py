"""`TorchVecEnv(..., kin_lookahead=...)`, `kin_query`, `clip_table` and `set_start_sampler` on the GPU (deepmimic_amd/vec_env.py, deepmimic_amd/kin_query.py): the
lookahead tensors of `step` and `update_link_state()` are what a direct dm_kin_query gives (and their frame at offset 0 is the kinematic link state of the same
step); a start sampler that returns a fixed (clip, time) puts the done envs there and leaves the others as a twin env without a sampler has them; with the options
off `step` goes through neither new entry point.  N = 4."""
import numpy as np
import pytest

from deepmimic_amd import model

pytestmark = pytest.mark.gpu
N, SEED = 4, 17
OFFSETS = (0.0, 1.0 / 30, 0.5)
PAIRS = (("kin_ahead_link_state", "link_state"), ("kin_ahead_link_env", "link_env"), ("kin_ahead_pose", "pose"), ("kin_ahead_vel", "vel"))


def tables(name, limit=None):
    t = model.load_asset(name)
    if limit is not None:
        t.cfg.time_lim_min = t.cfg.time_lim_max = limit
    return t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def count_calls(monkeypatch, lib, names):
    calls = {name: 0 for name in names}
    for name in names:
        real = getattr(lib, name)

        def counting(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    return calls


@pytest.mark.parametrize("name", ["humanoid3d_walk", "amp_heading_clips4"])
def test_lookahead_tensors_equal_a_direct_query(hip_lib, name):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(tables(name), N, seed=SEED, kin_link_state=True, deferred_reset=True, kin_lookahead=OFFSETS, lib_path=hip_lib)
    env.reset()
    J, P, K = env.env.J, env.env.P, len(OFFSETS)
    times = torch.tensor(OFFSETS, dtype=torch.float64, device=env.device)
    act = torch.zeros((N, env.act_dim), device=env.device)
    for k in range(2):
        _, _, done, info = env.step(act)
        assert info["kin_ahead_link_state"].shape == (N, K, J, 22) and info["kin_ahead_link_env"].shape == (N, K, 8)
        assert info["kin_ahead_pose"].shape == (N, K, P) and info["kin_ahead_vel"].shape == (N, K, P)
        for ahead, kin in PAIRS:                                       # the frame at offset 0 is the kinematic link state of the same launch position
            assert same(info[ahead][:, 0].contiguous(), info["kin_" + kin]), (k, ahead)
        live = ~done                                                   # (a done env has been reset behind the info tensors: they describe the end of its step)
        assert bool(live.any())
        direct = env.kin_query(times)
        host = env.env.kin_query(np.array(OFFSETS))
        for (ahead, key), hk in zip(PAIRS, ("links", "env", "pose", "vel")):
            assert same(info[ahead][live], direct[key][live]), (k, ahead)
            assert info[ahead][live].cpu().numpy().tobytes() == host[hk][live.cpu().numpy()].tobytes(), (k, ahead)
    before = {a: info[a].clone() for a, _ in PAIRS}
    env.step(act)
    assert not same(before["kin_ahead_pose"], info["kin_ahead_pose"])  # the same tensors, refreshed
    again = env.update_link_state()
    assert all(again[a] is info[a] for a, _ in PAIRS)
    # per-env absolute times on another clip of the dataset, in the clip's own frame
    dur, cdf = env.clip_table()
    assert dur.dtype == torch.float64 and dur.shape == (env.env.tables.num_clips,) and dur.device == env.obs.device and float(cdf[-1]) == 1.0
    clips = torch.zeros(N, dtype=torch.int32, device=env.device)
    t_abs = (0.25 * dur[0] * torch.arange(1, N + 1, device=env.device, dtype=torch.float64)).reshape(N, 1).contiguous()
    q = env.kin_query(t_abs, clips=clips, absolute=True, identity_origin=True)
    host = env.env.kin_query(t_abs.cpu().numpy(), clips=np.zeros(N, np.int32), absolute=True, identity_origin=True)
    assert q["pose"].shape == (N, 1, P) and q["pose"].cpu().numpy().tobytes() == host["pose"].tobytes()
    with pytest.raises(ValueError, match="times must be a contiguous float64"):
        env.kin_query(times.float())
    env.close()


def test_start_sampler_chooses_clip_and_time(hip_lib, monkeypatch):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    CLIP, TIME = 1, 0.3
    a = TorchVecEnv(tables("amp_heading_clips4", 0.1), N, seed=SEED, amp_obs=True, kin_link_state=True, deferred_reset=True, lib_path=hip_lib)
    b = TorchVecEnv(tables("amp_heading_clips4", 0.1), N, seed=SEED, amp_obs=True, kin_link_state=True, deferred_reset=True, lib_path=hip_lib)
    seen = []

    def sampler(done_i32, info):
        assert done_i32.dtype == torch.int32 and done_i32.shape == (N,) and "kin_link_state" in info
        seen.append(done_i32.clone())
        return {"clips": torch.full((N,), CLIP, dtype=torch.int32, device=a.device), "times": torch.full((N,), TIME, dtype=torch.float64, device=a.device)}

    with pytest.raises(ValueError, match="set_start_sampler needs deferred_reset=True"):
        TorchVecEnv(tables("humanoid3d_walk"), N, seed=SEED, lib_path=hip_lib).set_start_sampler(sampler)
    a.set_start_sampler(sampler)
    calls = count_calls(monkeypatch, a.env.lib, ("dm_reset_where", "dm_reset_where_at"))
    a.reset(); b.reset()
    act = torch.zeros((N, a.act_dim), device=a.device)
    done_total, b_steps = 0, 0
    for k in range(5):
        sa_before = a.env.get_state()
        _, _, done, _ = a.step(act)
        assert same(seen[-1] != 0, done)
        d = done.cpu().numpy()
        st, clips = a.env.get_state(), a.env.get_clips()
        assert (st["clocks"][d, 0] == TIME).all() and (clips[d] == CLIP).all(), (k, st["clocks"][:, 0], clips)
        assert (st["flags"][d, 2] == sa_before["flags"][d, 2] + 1).all() and (st["flags"][~d, 2] == sa_before["flags"][~d, 2]).all()
        done_total += int(d.sum())
        if done_total == int(d.sum()):                                 # up to and including the first step with a done env the twin saw the same episodes
            _, _, done_b, _ = b.step(act); b_steps += 1
            assert same(done, done_b)
            sb = b.env.get_state()
            for key in ("pose", "vel", "kin", "clocks", "flags"):      # the other envs are untouched: the step's own result, as the twin without a sampler has it
                assert st[key][~d].tobytes() == sb[key][~d].tobytes(), (k, key)
            if d.any():
                assert not (sb["clocks"][d, 0] == TIME).any()
    assert done_total >= N and calls == {"dm_reset_where": b_steps, "dm_reset_where_at": 5}      # (the twin's steps and this env's)
    assert int(a.start_bad.item()) == 0
    a.set_start_sampler(None)
    a.step(act)
    assert calls == {"dm_reset_where": b_steps + 1, "dm_reset_where_at": 5}
    a.close(); b.close()


def test_options_off_launch_nothing_new(hip_lib, monkeypatch):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(tables("humanoid3d_walk", 0.1), N, seed=SEED, link_state=True, kin_link_state=True, deferred_reset=True, lib_path=hip_lib)
    calls = count_calls(monkeypatch, env.env.lib, ("dm_kin_query", "dm_reset_where_at"))
    env.reset()
    act = torch.zeros((N, env.act_dim), device=env.device)
    for _ in range(4):
        _, _, _, info = env.step(act)
    env.update_link_state()
    assert calls == {"dm_kin_query": 0, "dm_reset_where_at": 0}
    assert not any(k.startswith("kin_ahead") for k in info)
    env.close()
    plain = TorchVecEnv(tables("humanoid3d_walk", 0.1), N, seed=SEED, lib_path=hip_lib)
    plain.reset()
    for _ in range(4):
        plain.step(act)
    assert calls == {"dm_kin_query": 0, "dm_reset_where_at": 0}
    with pytest.raises(RuntimeError, match="update_link_state needs"):
        plain.update_link_state()
    plain.close()
    # (the wrapper counts: the same steps with the options on go through both entry points)
    on = TorchVecEnv(tables("humanoid3d_walk", 0.1), N, seed=SEED, deferred_reset=True, kin_lookahead=(1.0 / 30,), lib_path=hip_lib)
    on.set_start_sampler(lambda done, info: {})
    on.reset()
    for _ in range(4):
        on.step(act)
    on.update_link_state()
    assert calls == {"dm_kin_query": 5, "dm_reset_where_at": 4}
    on.close()
