"""The batched test-mode time-warp return of `--scene imitate_amp` on the device: the checks of tests/test_time_warp.py through libdm_hip.so, and the torch wrappers.
Only tests/golden/time_warp_vectors.npz is read for the alignment (the reference's recorded numbers)."""
import numpy as np
import pytest

from deepmimic_amd import model
from deepmimic_amd import time_warp as tw
from test_time_warp import (U32, HostSampler, amp_two_clips, amp_walk, check_alignment, check_end_to_end, check_sampler, check_selection, golden_dims, rollout)

pytestmark = pytest.mark.gpu


def gpu_runner(hip_lib, f64):
    import torch

    def run(samples, count, select, tsc=1.0):
        n, _, cap, dim = samples.shape
        dev = torch.device("cuda:0")
        s, c = torch.from_numpy(samples).to(dev), torch.from_numpy(count).to(dev)
        sel = torch.from_numpy(select).to(dev) if select is not None else None
        reward, cost = torch.full((n,), -77.0, dtype=torch.float32, device=dev), torch.full((n,), -77.0, dtype=torch.float64, device=dev)
        tw.align_device(n, cap, dim, f64, s.data_ptr(), c.data_ptr(), sel.data_ptr() if sel is not None else 0, reward.data_ptr(), cost.data_ptr(), tsc,
                        stream=torch.cuda.current_stream(dev).cuda_stream, device_id=0, lib_path=hip_lib)
        torch.cuda.synchronize(dev)
        return reward.cpu().numpy(), cost.cpu().numpy()
    return run


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_alignment_vs_reference_dtw_gpu(hip_lib, f64):
    for dim in golden_dims():
        check_alignment(gpu_runner(hip_lib, f64), dim, f64, "gpu")


def test_alignment_selection_and_determinism_gpu(hip_lib):
    check_selection(gpu_runner(hip_lib, True), 45, True)
    check_selection(gpu_runner(hip_lib, False), golden_dims()[1], False)


def fk_tolerance(tables, root_abs):
    """Bound on |device row - host rebuild| for the fp32 build, both evaluated on the device's own (float) state; u = 2^-24, first order.
      A joint-local rotation from a unit quaternion or an angle (quat_to_rot: three products and two additions per entry; dm_sincos within 2 u) is within 8 u per
      entry, the kinematic side's pose a few roundings more (frame blend, slerp, origin transform): 16 u for the base of either chain.  A frame product R_par A R_l
      adds, per level, two 3-term dot products on entries <= 1: 2 (3 + 2) u plus what it inherits twice over: eps_d <= 16 u (d + 1) ... doubled for the inherited
      part: eps_d = 32 u (d + 1).  A joint position p_j = p_par + R_par attach adds per level 3 eps_d |attach| from the frame, 3 u |attach| from the product and
      u |p| from the sum; the root-relative row one more subtraction.  Over a chain of depth D: D (3 eps_D L + 3 u L + u P) + u P with L the longest attach vector
      and P the largest coordinate in play (root position plus the character's reach)."""
    jm = np.asarray(tables.joint_mat)
    depth = np.zeros(jm.shape[0], int)
    for j in range(1, jm.shape[0]):
        depth[j] = depth[int(jm[j, model.JD_PARENT])] + 1
    D, L = int(depth.max()), float(np.linalg.norm(jm[:, model.JD_AX:model.JD_AZ + 1], axis=1).max())
    P = root_abs + D * L
    return D * (3 * 32 * U32 * (D + 1) * L + 3 * U32 * L + U32 * P) + U32 * P


def gpu_rollout(hip_lib, tables, n_envs, steps, precision):
    import torch
    from deepmimic_amd.core import BatchEnv
    dev = torch.device("cuda:0")
    env = BatchEnv(tables, n_envs, precision=precision, seed=3, test_mode=True, lib_path=hip_lib)
    env.reset()
    obj = tw.TimeWarp(env, tables, device=dev)
    assert obj.f64 == (precision == 64) and obj.dim == 3 * env.J and obj.capacity == 8
    stream = env.own_stream()                                        # the context's stream: sample and align run on it, in order with the step launches

    def sample(restart):
        obj.sample(torch.from_numpy(restart).to(dev))
        env.synchronize()
        return obj.samples.cpu().numpy().astype(np.float64), obj.count.cpu().numpy(), obj.overflow.cpu().numpy()

    def align(done):
        reward, _ = obj.align(torch.from_numpy(done).to(dev), stream=stream)
        env.synchronize()
        return reward.cpu().numpy()
    torch.cuda.synchronize(dev)
    rec = rollout(env, tables, steps, sample, align)
    obj.check_overflow()
    env.close()
    return rec, obj.capacity


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("clips", [False, True], ids=["one_clip", "two_clips"])
def test_sampler_and_end_to_end_gpu(hip_lib, precision, clips):
    """8 envs through two auto-resets.  fp64: 1e-9 as on the emulator.  fp32: the host rebuild starts from the device's own get_state(); the rows agree to the float
    forward-kinematics error (fk_tolerance), the reward to what that moves the alignment by -- a cell's mean point distance moves by at most the two rows' errors,
    2 sqrt(3) tol, a path has at most 2 n cells -- plus the float kernel's own bound (test_time_warp.float_bound) and the rounding of the float32 reward."""
    from test_time_warp import float_bound
    tables = amp_two_clips() if clips else amp_walk()
    rec, cap = gpu_rollout(hip_lib, tables, 8, 14, precision)
    if precision == 64:
        tol = 1e-9
        rtol = lambda n, want: 1e-9 + 0.5 * np.spacing(np.float32(want))
    else:
        tol = fk_tolerance(tables, max(r["root"] for r in rec))
        rtol = lambda n, want: 2 * n * 2 * np.sqrt(3.0) * tol + float_bound(3 * tables.num_joints, n, want) + 0.5 * np.spacing(np.float32(want))
    print("TIMEWARP gpu sampler f%d tolerance %.3e" % (precision, tol))
    check_sampler(rec, cap, tol)
    check_end_to_end(rec, cap, rtol)
    if clips:
        assert {int(c) for r in rec for c in r["clips"]} == {0, 1}


def test_torch_wrappers_time_warp_return_gpu(hip_lib):
    """TorchVecEnv(time_warp=True, episode_stats=True), 64 envs, 0.2 s episodes, 14 steps: info["time_warp_return"] is the host recomputation at every done and 0
    elsewhere; episode_totals() has the mean of those values; TorchVecEnvGroups with 2 groups is row for row identical."""
    import torch
    from deepmimic_amd.vec_env import TorchVecEnv, TorchVecEnvGroups
    from test_time_warp import float_bound
    tables = amp_walk()
    kw = dict(seed=5, time_warp=True, episode_stats=True, test_mode=True, lib_path=hip_lib)
    venv = TorchVecEnv(tables, 64, **kw)
    grp = TorchVecEnvGroups(tables, 64, groups=2, **kw)
    assert grp.G == 2
    venv.reset(); grp.reset()
    hs, cap = HostSampler(tables), venv.tw.capacity
    host = [None] * 64
    restart = np.ones(64, bool)
    actions = torch.zeros((64, venv.act_dim), device=venv.device)
    paid, root = [], 0.0
    for k in range(14):
        torch.cuda.synchronize()
        st, clips = venv.env.get_state(), venv.env.get_clips()
        root = max(root, float(np.abs(st["pose"][:, 0:3]).max()))
        for e in range(64):
            s, kr = hs.rows(st, clips, e)
            if restart[e]:
                host[e] = [[s, s], [kr, kr]]
            else:
                host[e][0].append(s); host[e][1].append(kr)
        _, reward, done, info = venv.step(actions)
        _, _, gdone, ginfo = grp.step(actions)
        torch.cuda.synchronize()
        twr, d, valid = info["time_warp_return"].cpu().numpy(), done.cpu().numpy(), info["valid"].cpu().numpy()
        assert twr.dtype == np.float32 and (reward == 0).all()       # `reward` stays what the launch wrote: 0 for imitate_amp
        assert np.array_equal(ginfo["time_warp_return"].cpu().numpy(), twr) and np.array_equal(gdone.cpu().numpy(), d)
        assert np.array_equal(ginfo["episode_return"].cpu().numpy(), info["episode_return"].cpu().numpy())
        tol = fk_tolerance(tables, root)
        for e in range(64):
            if not d[e]:
                assert twr[e] == 0
                continue
            a, b = np.array(host[e][0]), np.array(host[e][1])
            n = a.shape[0]
            want = model.time_warp_cost(a, b) + (cap - n)
            assert abs(float(twr[e]) - want) <= 2 * n * 2 * np.sqrt(3.0) * tol + float_bound(45, n, want) + 0.5 * np.spacing(np.float32(want)), (k, e, twr[e], want)
            if valid[e]:
                paid.append(float(twr[e]))
        restart = d
    venv.tw.check_overflow()
    for t in grp.tw:
        t.check_overflow()
    assert len(paid) >= 128
    tot, gtot = venv.episode_totals(), grp.episode_totals()
    assert tot["episodes"] == len(paid) == gtot["episodes"]
    assert abs(tot["mean_return"] - np.mean(paid)) <= 1e-12 * np.mean(paid) and abs(gtot["mean_return"] - tot["mean_return"]) <= 1e-12 * np.mean(paid)
    venv.close(); grp.close()


def test_torch_wrapper_refuses_a_scene_without_a_warper(hip_lib):
    from deepmimic_amd.vec_env import TorchVecEnv, TorchVecEnvGroups
    for cls in (TorchVecEnv, TorchVecEnvGroups):
        with pytest.raises(ValueError, match="time_warp=True: the scene is `imitate`"):
            cls(model.load_asset("humanoid3d_walk"), 8, time_warp=True, lib_path=hip_lib)
