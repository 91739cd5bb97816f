"""The start of a new episode is written three times on the device: the auto-reset inside k_env_step, the one inside k_env_step_duo and
k_env_reset (the last two through one routine, reset_episode of dm_device.h; k_env_step keeps the same steps written out).  What they share is
pinned here: a context stepped with auto_reset=True and a second one stepped without, whose ended envs the test resets itself (dm_reset with
neither clip times nor time limits: every draw is the device's), hold the same bits after every control step -- character state, clocks,
flags, and with them the goal rows, the clip ids, the perturbation rows, the v2 ground manifolds and the AMP pose history (through the AMP
observation of the following step).  Pass 1 of the step kernels' emit loop hands back the observation (and goal) of the new episode: it equals
query() of the explicitly reset context.

Every comparison is an exact equality of the arrays' bytes.  The time limit is pinned to 0.1 s: sixty additions of 1/600 s stay one rounding
below it, so an episode of the plain scenes ends at the first update of its fourth control step (the early episode end cuts that step short on
both routes), and eight control steps hold two episodes.  The multi-clip goal scene also ends some earlier (two of its clips start lying on the
ground)."""
import numpy as np
import pytest

from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv

DT = 1.0 / 600
N, STEPS, SEED = 4, 8, 17       # two pairs of the two-per-wave kernel; two episodes each


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


def plain_tables():
    return model.load_asset("humanoid3d_walk")


def amp_perturbed_tables():
    t = model.load_asset("humanoid3d_walk")
    c = t.cfg
    c.scene = "imitate_amp"                     # the same asset as --scene imitate_amp: pose history, AMP instantiation of the kernels
    c.enable_rand_perturbs = True; c.perturb_time_min, c.perturb_time_max = 0.03, 0.06
    c.min_perturb, c.max_perturb = 100.0, 300.0; c.min_pertrub_duration, c.max_perturb_duration = 0.01, 0.05
    return t


def goal_tables():
    return model.load_asset("amp_heading_clips4")


def extras(env):
    """device rows beyond snapshot() (which holds goal row, aux block, perturbation row and manifolds where the scene has them)"""
    x = {}
    if env._has_goal_row:
        x["goal"] = env.get_goal_state(); x["aux"] = env.get_goal_aux(); x["clips"] = env.get_clips()
    if env.has_perturbs:
        x["pert"] = env.get_perturb_state()
    return x


def auto_reset_equals_explicit_reset(t, lib, prec, packing, physics=1, amp=False):
    a, b = (BatchEnv(t, N, precision=prec, lib_path=lib, seed=SEED, wave_packing=packing, physics=physics) for _ in range(2))
    for env in (a, b):
        env.set_time_limits(0.1, 0.1)
        env.reset()
    assert_same(a.snapshot(), b.snapshot(), "start")
    ends = np.zeros((STEPS, N), dtype=bool)
    for k in range(STEPS):
        oa = a.step(None, DT, 20, auto_reset=True, open_loop=True, amp=amp)
        ob = b.step(None, DT, 20, auto_reset=False, end_early=True, open_loop=True, amp=amp)
        ended = ob["episode_end"] != 0
        ends[k] = ended
        fresh = [key for key in ("state", "goal") if key in ob]      # pass 1 of the emit loop: observation (and goal) of the new episode
        for key in ob:                          # reward, flags and AMP observation are those of the finished step on both routes
            if key not in fresh:
                assert same_bits(oa[key], ob[key]), (k, key)
        for key in fresh:
            assert same_bits(oa[key][~ended], ob[key][~ended]), (k, key)
        if ended.any():
            b.reset(np.nonzero(ended)[0])
            q = b.query()
            for key in fresh:
                assert same_bits(oa[key][ended], q[key][ended]), (k, key, "emit pass 1")
        assert_same(a.snapshot(), b.snapshot(), k)
        assert_same(extras(a), extras(b), k)
    a.close(); b.close()
    return ends


CASES = [(p, v) for p in (1, 2) for v in (1, 2)]


def _plain(lib, prec, packing, physics):
    ends = auto_reset_equals_explicit_reset(plain_tables(), lib, prec, packing, physics)
    assert (ends == np.array([0, 0, 0, 1, 0, 0, 0, 1], dtype=bool)[:, None]).all(), ends      # the pinned limit: every episode ends in its fourth step


def _amp_perturbed(lib, prec, packing):
    ends = auto_reset_equals_explicit_reset(amp_perturbed_tables(), lib, prec, packing, amp=True)
    assert ends.sum() >= 2 * N, ends                    # (a push may end an episode earlier)


def _goal(lib, prec, packing):
    ends = auto_reset_equals_explicit_reset(goal_tables(), lib, prec, packing, amp=True)
    assert ends.sum() >= 2 * N, ends


@pytest.mark.parametrize("packing,physics", CASES)
def test_auto_reset_equals_explicit_reset_emulator(emu_lib, packing, physics):
    _plain(emu_lib, 64, packing, physics)


@pytest.mark.parametrize("packing", [1, 2])
def test_auto_reset_with_history_and_perturbs_emulator(emu_lib, packing):
    _amp_perturbed(emu_lib, 64, packing)


@pytest.mark.parametrize("packing", [1, 2])
def test_auto_reset_of_a_multi_clip_goal_scene_emulator(emu_lib, packing):
    _goal(emu_lib, 64, packing)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("packing,physics", CASES)
def test_auto_reset_equals_explicit_reset_gpu(hip_lib, packing, physics, prec):
    _plain(hip_lib, prec, packing, physics)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", [1, 2])
def test_auto_reset_with_history_and_perturbs_gpu(hip_lib, packing):
    _amp_perturbed(hip_lib, 32, packing)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", [1, 2])
def test_auto_reset_of_a_multi_clip_goal_scene_gpu(hip_lib, packing):
    _goal(hip_lib, 32, packing)
