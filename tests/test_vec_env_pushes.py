"""`TorchVecEnv(..., pushes=True)` and `pushes.RandomPushes` on the GPU (deepmimic_amd/vec_env.py, deepmimic_amd/pushes.py): info["pushes"] is BatchEnv.push_state(),
taken before the reset under deferred_reset; the tensors are converted on the device; an invalid row raises; the sampler is reproducible, depends on its seed and honours
a per-env magnitude tensor.  N = 64 envs, the size of tests/test_agent.py; episodes pinned to 0.1 s where a test wants every env to end in the same step."""
import numpy as np
import pytest

from deepmimic_amd import model

pytestmark = pytest.mark.gpu
N, SEED = 64, 7


def tables(limit=None):
    t = model.load_asset("humanoid3d_walk")
    if limit is not None:
        t.cfg.time_lim_min = t.cfg.time_lim_max = limit
    return t


def make(hip_lib, limit=None, **kw):
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(tables(limit), N, seed=SEED, lib_path=hip_lib, **kw)
    env.reset()
    return env


def some_pushes(env, duration=0.5):
    import torch
    dev = env.device
    e = torch.arange(N, device=dev)
    mask = (e % 3 != 1)
    links = (e % env.env.J).to(torch.int32)
    forces = torch.stack([1.0 + 0.125 * e, -0.0625 * e, 0.25 * e - 4.0], dim=1).to(torch.float32)        # (a few newtons: nobody falls)
    durations = torch.full((N,), duration, dtype=torch.float32, device=dev)
    return mask, links, forces, durations


def test_info_pushes_is_push_state(hip_lib):
    import torch
    t = tables()
    from deepmimic_amd.vec_env import TorchVecEnv
    env = TorchVecEnv(t, N, seed=SEED, lib_path=hip_lib, pushes=True)
    assert not t.cfg.task_pushes and env.env.tables.cfg.task_pushes and env.has_pushes       # the env's own copy of the config
    env.reset()
    assert tuple(env.pushes.shape) == (N, 2, 6) and env.pushes.dtype == torch.float32 and (env.pushes[:, :, 0] == -1).all()
    mask, links, forces, durations = some_pushes(env)
    env.push(mask, links, forces, durations)
    act = torch.zeros((N, env.act_dim), device=env.device)
    for k in range(3):
        if k == 1:
            env.push(~mask, links, -forces, durations, frame="heading")
        _, _, _, info = env.step(act)
        assert info["pushes"] is env.pushes
        got = info["pushes"].cpu().numpy()
        assert got.tobytes() == env.env.push_state().tobytes(), k
        sel = mask.cpu().numpy()
        assert (got[sel, 0, 0] == links.cpu().numpy()[sel]).all() and (got[sel, 0, 1:4] == forces.cpu().numpy()[sel]).all()
        assert np.abs(got[sel, 0, 5] - (k + 1) / 30).max() < 1e-6 and (got[~sel, 0, 0] >= 0).all() == (k >= 1)
    env.clear_pushes(mask)
    assert (env.env.push_state()[:, :, 0] >= 0).any(axis=1).tolist() == (~mask).cpu().numpy().tolist()
    env.clear_pushes()
    assert (env.env.push_state()[:, :, 0] == -1).all()
    env.reset()
    assert (env.pushes[:, :, 0] == -1).all()
    env.close()


def test_deferred_reset_shows_the_terminal_pushes(hip_lib):
    """episodes pinned to 0.1 s end in the fourth step: under deferred_reset the done envs show what was acting when the episode ended, the context's rows are
    cleared by the reset behind it; the auto-reset step shows the new episode's empty slots"""
    import torch
    a, b = make(hip_lib, 0.1, pushes=True, deferred_reset=True), make(hip_lib, 0.1, pushes=True)
    every = torch.ones(N, dtype=torch.int32, device=a.device)
    links = torch.full((N,), 2, dtype=torch.int32, device=a.device)
    forces = torch.tensor([15.0, 0.0, -5.0], dtype=torch.float64, device=a.device).expand(N, 3)
    durations = torch.full((N,), float("inf"), dtype=torch.float64, device=a.device)
    act = torch.zeros((N, a.act_dim), device=a.device)
    seen = 0
    for env in (a, b):
        env.push(every, links, forces, durations)
    for k in range(4):
        (_, _, da, ia), (_, _, db, ib) = a.step(act), b.step(act)
        assert torch.equal(da, db), k
        done = da.cpu().numpy()
        pa, pb = ia["pushes"].cpu().numpy(), ib["pushes"].cpu().numpy()
        assert (pa[:, 0, 0] == 2).all() and np.isinf(pa[:, 0, 4]).all() and (pa[:, 0, 5] > 0).all(), k       # every env, finished ones included
        assert (pb[done, :, 0] == -1).all() and pb[~done].tobytes() == pa[~done].tobytes(), k
        assert a.env.push_state().tobytes() == pb.tobytes(), k                # the deferred env's context behind its reset
        seen += int(done.sum())
        for env in (a, b):                                                    # the new episodes are pushed again
            env.push(da, links, forces, durations)
    assert seen >= N
    a.close(); b.close()


def test_masks_and_floats_are_converted_on_the_device(hip_lib):
    import torch
    a, b = make(hip_lib, pushes=True), make(hip_lib, pushes=True)
    mask, links, forces, durations = some_pushes(a, 0.25)
    a.push(mask, links, forces, durations)                                    # bool, float32
    b.push(mask.to(torch.int32), links, forces.to(torch.float64), durations.to(torch.float64), slots=torch.full((N,), -1, dtype=torch.int32, device=b.device))
    assert a.env.get_perturb_state().tobytes() == b.env.get_perturb_state().tobytes()
    with pytest.raises(ValueError, match="forces must be"):
        a.push(mask, links, forces.cpu(), durations)
    with pytest.raises(ValueError, match="links must be"):
        a.push(mask, links.to(torch.int64), forces, durations)
    with pytest.raises(ValueError, match="frame"):
        a.push(mask, links, forces, durations, frame="local")
    a.close(); b.close()


def test_a_bad_row_raises_and_an_env_without_rows_refuses(hip_lib):
    import torch
    env = make(hip_lib, pushes=True)
    mask, links, forces, durations = some_pushes(env)
    bad_links = links.clone(); bad_links[5] = env.env.J                       # (env 5 is selected: 5 % 3 == 2)
    before = env.env.get_perturb_state()
    with pytest.raises(ValueError, match="invalid value"):
        env.push(mask, bad_links, forces, durations)
    after = env.env.get_perturb_state()
    sel = mask.cpu().numpy().copy(); sel[5] = False
    assert after[5].tobytes() == before[5].tobytes() and (after[sel, 3] == links.cpu().numpy()[sel] + 1).all()      # the others were served
    env.clear_pushes()
    env.push(mask, bad_links, forces, durations, check=False)                 # no host read, no exception: the word stays for whoever asks
    assert int(env.push_bad.item()) == 1
    env.push(mask, links, forces, durations)                                  # check=True zeroes the word first
    assert int(env.push_bad.item()) == 0
    env.close()
    plain = make(hip_lib)
    assert not plain.has_pushes and plain.pushes is None
    with pytest.raises(ValueError, match="pushes=True"):
        plain.push(mask, links, forces, durations)
    with pytest.raises(ValueError, match="pushes=True"):
        plain.clear_pushes()
    _, _, _, info = plain.step(torch.zeros((N, plain.act_dim), device=plain.device))
    assert "pushes" not in info
    from deepmimic_amd.pushes import RandomPushes
    with pytest.raises(ValueError, match="pushes=True"):
        RandomPushes(plain)
    plain.close()


def test_random_pushes_are_reproducible_and_honour_the_magnitude_tensor(hip_lib):
    import torch
    from deepmimic_amd.pushes import RandomPushes
    a, b, c = (make(hip_lib, pushes=True) for _ in range(3))
    e = torch.arange(N, device=a.device, dtype=torch.float64)
    mags = [torch.stack([10.0 + 10.0 * e, 15.0 + 10.0 * e], dim=1).to(dt) for dt in (torch.float32, torch.float64, torch.float32)]     # disjoint ranges, one per env
    kw = dict(interval=(1, 3), duration=(0.05, 0.2), links=[0, 2, 5])
    sa, sb, sc = RandomPushes(a, magnitude=mags[0], seed=3, **kw), RandomPushes(b, magnitude=mags[1], seed=3, **kw), RandomPushes(c, magnitude=mags[2], seed=4, **kw)
    act = torch.zeros((N, a.act_dim), device=a.device)
    fired, differs = np.zeros(N, int), False
    for k in range(8):
        da, db, dc = sa(None, k), sb(None, k), sc(None, k)
        assert da["check"] is False
        for key in ("mask", "links", "forces", "durations"):
            assert torch.equal(da[key], db[key]), (k, key)
            differs |= not torch.equal(da[key], dc[key])
        m = da["mask"].cpu().numpy() != 0
        f, d, lk = da["forces"].cpu().numpy()[m], da["durations"].cpu().numpy()[m], da["links"].cpu().numpy()[m]
        lo, hi = mags[1].cpu().numpy()[m, 0], mags[1].cpu().numpy()[m, 1]
        norm = np.linalg.norm(f, axis=1)
        assert (norm >= lo * (1 - 1e-12)).all() and (norm <= hi * (1 + 1e-12)).all() and (d >= 0.05).all() and (d <= 0.2).all() and set(lk.tolist()) <= {0, 2, 5}
        for env, dd in ((a, da), (b, db)):
            env.push(**dd)
        # what the context stores: the newest force of every pushed env lies in that env's range
        rows = a.env.get_perturb_state()[m]
        newest = np.where((rows[:, 8] == 0)[:, None] & (rows[:, 3] > 0)[:, None], rows[:, 4:7], rows[:, 10:13])
        assert np.abs(np.linalg.norm(newest, axis=1) - norm).max() < 1e-9
        fired += m
        ra, rb = a.step(act), b.step(act)
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[3]["pushes"], rb[3]["pushes"]), k
    assert differs and (fired >= 2).all() and (fired < 8).any()              # an interval of 1 .. 3 steps: every env was pushed, not all of them at every step
    mags[0][:, 0] = 1000.0; mags[0][:, 1] = 1001.0                            # the curriculum: the task updates the tensor, the next call reads it
    d = sa(None, 8)
    m = d["mask"].cpu().numpy() != 0
    norm = np.linalg.norm(d["forces"].cpu().numpy()[m], axis=1)
    assert m.any() and (norm >= 1000.0 * (1 - 1e-6)).all() and (norm <= 1001.0 * (1 + 1e-6)).all()
    for env in (a, b, c):
        env.close()
