"""The observation of the moment an episode ended (include/dm_hip.h dm_set_terminal_outputs): a DM_AUTO_RESET launch overwrites the `states` / goal row of an env it
resets with the first observation of the next episode; with terminal buffers bound it first writes the row it had computed -- RecordState / RecordGoal at the update
that ended the episode -- into them, for the envs it resets and for no other.

Episodes are made short (episode timer U[0.1, 0.2] s: 3 .. 6 control steps) and the actions noisy, so that 8 control steps hold timer ends (terminate Null) and
falls (Fail, see DROPS) in every scene.  A: identity -- before every step context B takes over A's full state (snapshot / restore: dm_get_state / dm_set_state and the goal, aux,
object, perturbation and manifold rows; clips) and steps WITHOUT auto-reset under the same actions: its `states` / goal rows ARE the terminal rows, bit for bit, and the
rows of envs A did not reset still hold the sentinel.  B: no side effect -- a bound and an unbound context produce the same bits.  C: the oracle's RecordState /
RecordGoal of the ended env, inside the bounds the free-running parity tests hold `states` to.  D: the torch wrappers."""
import numpy as np
import pytest

import parity_common as pc
from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv

DT = pc.DT
STEPS = 8
# The noise alone fells nobody inside 0.2 s (measured: 0 falls in 640 env-steps at sigma 1.5; the root drops 0.2 m at most): before control steps 0 and 4 one env
# is put low enough for a fall contact ({step: env, modulo the batch} -- one character of a pair, so the two-per-wave kernel parks it while its mate goes on)
DROPS = {0: 1, 4: 2}
SENTINEL = 0x7fc12345                  # a quiet-NaN bit pattern no observation holds
# scene, envs, action noise (PD-target radians), seed.  64: two characters per wavefront; 3: an odd batch takes the one-per-wave kernel; dog: the tree class;
# heading: goal rows; dribble: the state row ends with the ball's 15 entries
CASES = [("humanoid3d_walk", 64, 1.5, 3), ("humanoid3d_walk", 3, 1.5, 4), ("dog3d_pace", 4, 1.5, 2), ("amp_heading_zombie", 8, 1.5, 5), ("amp_dribble_zombie", 4, 1.5, 1)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class DevBuf:
    """rows x width float32 of device memory filled with the sentinel: host memory for the emulator build, a torch tensor on the GPU"""

    def __init__(self, gpu, rows, width):
        self.gpu, self.shape = gpu, (rows, max(width, 1))
        if gpu:
            import torch
            self.torch = torch
            self.t = torch.zeros(self.shape, dtype=torch.int32, device="cuda")
        else:
            self.a = np.zeros(self.shape, np.uint32)
        self.fill()
        self.ptr = int(self.t.data_ptr()) if gpu else int(self.a.ctypes.data)

    def fill(self):
        if self.gpu:
            self.t.fill_(SENTINEL); self.torch.cuda.synchronize()
        else:
            self.a[:] = SENTINEL

    def bits(self):
        """the rows as uint32 (call after the step's outputs came back: the launch is complete)"""
        if self.gpu:
            self.torch.cuda.synchronize()
            return self.t.cpu().numpy().view(np.uint32).copy()
        return self.a.copy()


def short_episodes(env):
    env.set_time_limits(0.1, 0.2)
    env.reset()


def drop(env, e):
    """put env e's root at 0.35 of its height: links that count as a fall touch the ground at the next update"""
    pose = env.get_state()["pose"]
    pose[e, 1] *= 0.35
    env.set_state(pose=pose)


def clone_into(b, a):
    b.restore(a.snapshot())
    if a._has_goal_row:
        b.set_clips(a.get_clips())


def identity(lib, gpu, scene, n, sigma, seed, prec=32, physics=1):
    t = model.load_asset(scene)
    a, b = (BatchEnv(t, n, precision=prec, lib_path=lib, seed=seed, physics=physics) for _ in range(2))
    amp = a.amp_size > 0
    short_episodes(a)
    ts, tg = DevBuf(gpu, n, a.S), DevBuf(gpu, n, a.G)
    a.set_terminal_outputs(ts.ptr, tg.ptr if a.G else 0)
    rng = np.random.default_rng(seed)
    nulls = fails = invalid = 0
    for k in range(STEPS):
        if k in DROPS:
            drop(a, DROPS[k] % n)
        clone_into(b, a)
        acts = (sigma * rng.normal(size=(n, a.A))).astype(np.float32)
        ts.fill(); tg.fill()
        oa = a.step(acts, DT, 20, auto_reset=True, amp=amp)
        ob = b.step(acts, DT, 20, auto_reset=False, end_early=True, amp=amp)
        for key in ("reward", "terminate", "valid", "episode_end"):
            assert same_bits(oa[key], ob[key]), (scene, k, key)
        was_reset = (oa["episode_end"] != 0) | (oa["valid"] == 0)
        nulls += int(((oa["episode_end"] != 0) & (oa["terminate"] == 0) & (oa["valid"] != 0)).sum())
        fails += int((oa["terminate"] == 1).sum()); invalid += int((oa["valid"] == 0).sum())
        got = ts.bits()
        assert same_bits(got[was_reset], ob["state"].view(np.uint32)[was_reset]), (scene, k, "terminal_obs")
        assert (got[~was_reset] == SENTINEL).all(), (scene, k, "a row of an env that was not reset was written")
        assert same_bits(oa["state"][~was_reset], ob["state"][~was_reset]), (scene, k)
        if was_reset.any():                                  # `states` of a reset env: the first observation of the new episode, not the terminal one
            assert not same_bits(oa["state"][was_reset], ob["state"][was_reset]), (scene, k)
        gg = tg.bits()
        if a.G:
            assert same_bits(gg[was_reset][:, :a.G], ob["goal"][:, :a.G].view(np.uint32)[was_reset]), (scene, k, "terminal_goal")
            assert (gg[~was_reset] == SENTINEL).all(), (scene, k)
        else:
            assert (gg == SENTINEL).all()
    a.close(); b.close()
    print("%s n=%d: %d timer ends, %d falls, %d invalid" % (scene, n, nulls, fails, invalid))
    assert nulls >= 1 and fails >= 1, (scene, nulls, fails)


def no_side_effect(lib, gpu, scene, n, sigma, seed, prec=32, physics=1):
    t = model.load_asset(scene)
    a, b = (BatchEnv(t, n, precision=prec, lib_path=lib, seed=seed, physics=physics) for _ in range(2))
    amp = a.amp_size > 0
    for env in (a, b):
        short_episodes(env)
    ts, tg = DevBuf(gpu, n, a.S), DevBuf(gpu, n, a.G)
    a.set_terminal_outputs(ts.ptr, tg.ptr if a.G else 0)
    rng = np.random.default_rng(seed)
    ends = 0
    for k in range(STEPS):
        acts = (sigma * rng.normal(size=(n, a.A))).astype(np.float32)
        oa = a.step(acts, DT, 20, auto_reset=True, amp=amp)
        ob = b.step(acts, DT, 20, auto_reset=True, amp=amp)
        assert oa.keys() == ob.keys()
        for key in oa:                                       # state, reward, flags, amp_obs, goal
            assert same_bits(oa[key], ob[key]), (scene, k, key)
        sa, sb = a.snapshot(), b.snapshot()
        for key in sa:
            assert same_bits(sa[key], sb[key]), (scene, k, key)
        ends += int(((oa["episode_end"] != 0) | (oa["valid"] == 0)).sum())
    assert ends >= n // 2
    # without DM_AUTO_RESET the binding has no effect; unbound again, nothing is written
    ts.fill(); tg.fill()
    a.step(None, DT, 20, auto_reset=False, end_early=True, amp=amp)
    a.set_terminal_outputs(0, 0)
    for k in range(4):                                       # (every episode is at most 6 control steps long and most are under way: some end here)
        a.step(None, DT, 20, auto_reset=True, amp=amp)
    assert (ts.bits() == SENTINEL).all() and (tg.bits() == SENTINEL).all()
    a.close(); b.close()


@pytest.mark.parametrize("scene,n,sigma,seed", CASES)
def test_terminal_rows_are_what_a_step_without_reset_reports_emulator(emu_lib, scene, n, sigma, seed):
    identity(emu_lib, False, scene, n, sigma, seed)


@pytest.mark.parametrize("scene,n,sigma,seed", CASES)
def test_binding_changes_nothing_else_emulator(emu_lib, scene, n, sigma, seed):
    no_side_effect(emu_lib, False, scene, n, sigma, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n,sigma,seed", CASES)
def test_terminal_rows_are_what_a_step_without_reset_reports_gpu(hip_lib, scene, n, sigma, seed):
    identity(hip_lib, True, scene, n, sigma, seed)


@pytest.mark.gpu
def test_terminal_rows_under_physics_2_gpu(hip_lib):
    identity(hip_lib, True, "humanoid3d_walk", 8, 1.5, 6, physics=2)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n,sigma,seed", CASES)
def test_binding_changes_nothing_else_gpu(hip_lib, scene, n, sigma, seed):
    no_side_effect(hip_lib, True, scene, n, sigma, seed)


def test_binding_is_refused_where_it_cannot_hold(emu_lib):
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=32, lib_path=emu_lib)
    buf = DevBuf(False, 2, env.S)
    with pytest.raises(RuntimeError, match="goal"):
        env.set_terminal_outputs(buf.ptr, buf.ptr)           # terminal goals of a scene without goals
    with pytest.raises(RuntimeError, match="dm_set_terminal_outputs"):
        env.set_terminal_outputs(0, buf.ptr)                 # goals without states
    env.set_terminal_outputs(buf.ptr, 0); env.set_terminal_outputs(0, 0)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- C: the oracle
def walk_against_oracle(lib, gpu, prec, bound, steps, n=4, seed=5):
    """parity_common.auto_reset_rollout_compare with the terminal buffer bound: a free-running open-loop rollout through auto-resets whose every reset the oracle
    mirrors with the same counter-based draws; where the device reset an env, its terminal row is compared with the oracle's RecordState BEFORE the oracle's reset
    (relative to max(1, |state|), the metric of that routine)"""
    from deepmimic_amd import streams
    from oracle_lib import Oracle
    t = model.load_asset("humanoid3d_walk")
    t.cfg.time_lim_min, t.cfg.time_lim_max = 0.1, 0.2
    env = BatchEnv(t, n, precision=prec, lib_path=lib, seed=seed)
    env.reset()
    ts = DevBuf(gpu, n, env.S)
    env.set_terminal_outputs(ts.ptr, 0)
    ep = env.get_state()["flags"][:, 2].astype(np.int64)

    def draw(e, episode):
        return streams.reset_rand01(seed, e, episode, 0), 0.1 + (0.2 - 0.1) * streams.reset_rand01(seed, e, episode, 1)
    oracles = []
    for e in range(n):
        o = Oracle(t); u, mt = draw(e, int(ep[e]) - 1); o.reset(o.duration * u, mt); oracles.append(o)
    worst, ends = 0.0, 0
    for k in range(steps):
        ts.fill()
        out = env.step(None, DT, 20, open_loop=True, auto_reset=True)
        got = ts.bits()
        for e, o in enumerate(oracles):
            kp, _, _ = o.kin_state()
            o.set_action(o.pose_to_action(kp))
            o.control_step(20, DT)
            end = o.is_episode_end() or not o.check_valid_episode()
            assert bool(out["episode_end"][e]) == o.is_episode_end() and int(out["valid"][e]) == int(o.check_valid_episode())
            if end:
                so = o.record_state()
                worst = max(worst, np.abs(got[e].view(np.float32) - so).max() / max(1.0, np.abs(so).max())); ends += 1
                u, mt = draw(e, int(ep[e])); o.reset(o.duration * u, mt); ep[e] += 1
            else:
                assert (got[e] == SENTINEL).all()
    env.close()
    print("walk fp%d: %d ends, terminal row vs oracle %.2e (bound %.0e)" % (prec, ends, worst, bound))
    assert ends >= n and worst < bound, (ends, worst)


def goal_against_oracle(lib, gpu, prec, bound_state, bound_goal, steps, n, seed=5, monkeypatch=None):
    """parity_common.goal_rollout_compare (closed loop, every device draw mirrored) with the terminal buffers bound.  The routine asks an ended oracle
    `maybe_recovery_reset` before anything resets it: there the oracle's RecordState / RecordGoal of the moment are kept per env; a terminal row stays in the device
    buffer until the env ends again, so the last ones are compared after the rollout."""
    from oracle_lib import Oracle
    t = model.load_asset("amp_heading_zombie")
    t.cfg.time_lim_min, t.cfg.time_lim_max = 0.1, 0.2
    env_of, last, bufs = {}, {}, {}
    real_rng, real_rec = Oracle.goal_rng, Oracle.maybe_recovery_reset

    def goal_rng(self, seed_, env_id, draws=0):
        env_of[id(self)] = env_id
        return real_rng(self, seed_, env_id, draws)

    def maybe_recovery_reset(self, max_time=np.inf):
        last[env_of[id(self)]] = (self.record_state().copy(), self.record_goal().copy())
        return real_rec(self, max_time)
    monkeypatch.setattr(Oracle, "goal_rng", goal_rng); monkeypatch.setattr(Oracle, "maybe_recovery_reset", maybe_recovery_reset)

    def bind(env):
        bufs["env"], bufs["ts"], bufs["tg"] = env, DevBuf(gpu, n, env.S), DevBuf(gpu, n, env.G)
        env.set_terminal_outputs(bufs["ts"].ptr, bufs["tg"].ptr)
    w = pc.goal_rollout_compare(t, prec, lib, steps=steps, n=n, seed=seed, on_env=bind)
    assert w["resets"] >= n and (prec == 32 or w["flags_ok"]), w
    gs, gg = bufs["ts"].bits().view(np.float32), bufs["tg"].bits().view(np.float32)
    ws = wg = 0.0
    for e, (so, go) in last.items():
        ws = max(ws, np.abs(gs[e] - so).max() / max(1.0, np.abs(so).max())); wg = max(wg, np.abs(gg[e][:len(go)] - go).max())
    print("heading fp%d: %d envs ended (%d desynced), terminal row vs oracle %.2e (bound %.0e), goal %.2e (bound %.0e)" % (prec, len(last), w["desynced"], ws, bound_state, wg, bound_goal))
    assert len(last) >= n // 2 and ws < bound_state and wg < bound_goal, (ws, wg)


def test_terminal_row_matches_the_oracle_walk_emulator(emu_lib):
    walk_against_oracle(emu_lib, False, 64, 1e-5, steps=10)             # the free-running bound on `states`: tests/test_parity_emu.py:134 (ds.max() < 1e-5)


def test_terminal_row_matches_the_oracle_goal_scene_emulator(emu_lib, monkeypatch):
    # the free-running bounds of tests/test_goal_scenes.py:67 for this scene (tol = 1e-6): state < max(1e-5, 50 tol) = 5e-5, goal < 10 tol = 1e-5
    goal_against_oracle(emu_lib, False, 64, 5e-5, 1e-5, steps=10, n=4, monkeypatch=monkeypatch)


@pytest.mark.gpu
def test_terminal_row_matches_the_oracle_walk_gpu(hip_lib):
    walk_against_oracle(hip_lib, True, 64, 1e-5, steps=10)


@pytest.mark.gpu
def test_terminal_row_matches_the_oracle_goal_scene_gpu(hip_lib, monkeypatch):
    goal_against_oracle(hip_lib, True, 64, 5e-5, 1e-5, steps=10, n=4, monkeypatch=monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- D: the torch wrappers
def wrapper_case(make, hip_lib, scene, n):
    import torch
    t = model.load_asset(scene)
    env = make(t, n, seed=9, lib_path=hip_lib)
    ctxs = [env.env] if hasattr(env, "env") else env.g.envs
    ref = [BatchEnv(t, c.N, precision=32, lib_path=hip_lib, seed=9, env_id_offset=c._env_off) for c in ctxs]
    for c in ctxs:
        c.set_time_limits(0.1, 0.2)
    obs = env.reset()
    gen = torch.Generator(device="cuda"); gen.manual_seed(2)
    dones = 0
    for k in range(8):
        for c, r in zip(ctxs, ref):
            c.synchronize(); clone_into(r, c)
        acts = 1.5 * torch.randn((n, env.act_dim), generator=gen, dtype=torch.float32, device="cuda")
        obs, rew, done, info = env.step(acts)
        torch.cuda.synchronize()
        d = done.cpu().numpy()
        o0 = 0
        outs = []
        for c, r in zip(ctxs, ref):
            outs.append(r.step(acts[o0:o0 + c.N].cpu().numpy(), DT, 20, auto_reset=False, end_early=True, amp=r.amp_size > 0)); o0 += c.N
        want = np.concatenate([o["state"] for o in outs])
        assert same_bits(info["terminal_obs"].cpu().numpy()[d], want[d]), (scene, k)
        assert same_bits(obs.cpu().numpy()[~d], want[~d])
        if d.any():
            assert not same_bits(obs.cpu().numpy()[d], want[d])      # obs[done]: still the first observation of the new episode
            for c in ctxs:
                c.synchronize()
            q = np.concatenate([c.query()["state"] for c in ctxs])
            assert same_bits(obs.cpu().numpy()[d], q[d]), (scene, k)
        if env.goal_dim:
            wg = np.concatenate([o["goal"] for o in outs])[:, :env.goal_dim]
            assert same_bits(info["terminal_goal"].cpu().numpy()[d], wg[d]), (scene, k)
        else:
            assert "terminal_goal" not in info
        dones += int(d.sum())
    assert dones >= n
    for r in ref:
        r.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n", [("humanoid3d_walk", 8), ("amp_heading_zombie", 8)])
def test_torch_vec_env_hands_out_the_terminal_observation(hip_lib, scene, n):
    from deepmimic_amd.vec_env import TorchVecEnv
    wrapper_case(TorchVecEnv, hip_lib, scene, n)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n", [("humanoid3d_walk", 8), ("amp_heading_zombie", 8)])
def test_torch_vec_env_groups_hand_out_the_terminal_observation(hip_lib, scene, n):
    from deepmimic_amd.vec_env import TorchVecEnvGroups
    wrapper_case(lambda t, n_, **kw: TorchVecEnvGroups(t, n_, groups=2, **kw), hip_lib, scene, n)


@pytest.mark.gpu
def test_terminal_obs_can_be_switched_off(hip_lib):
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(model.load_asset("humanoid3d_walk"), 2, lib_path=hip_lib, terminal_obs=False)
    env.reset()
    _, _, _, info = env.step(torch.zeros((2, env.act_dim), dtype=torch.float32, device="cuda"))
    assert "terminal_obs" not in info and env.terminal_obs is None
    env.close()
