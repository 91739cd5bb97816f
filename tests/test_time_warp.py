"""The batched test-mode time-warp return of `--scene imitate_amp` (deepmimic_amd/time_warp.py, csrc/dm_time_warp.h, k_time_warp_sample of dm_device.h) on the CPU
emulator; tests/test_time_warp_gpu.py runs the same checks on the device.

* alignment: the golden vectors of tests/golden/make_time_warp_vectors.py -- random-walk sequences whose optimal path leaves the diagonal, sample counts
  {1, 2, 3, 63, 64, 65, 127, 128, 129, 130} mixed in one batch (strip hand-over, ramp-up, tail of the 64-row strips), dim 45 and the dog's 3J -- against the numbers
  the reference's compiled cDynamicTimeWarper gave for them.  Rows past an env's count hold NaN: they must never be read.
* sampler: 4 humanoid3d_walk envs as imitate_amp with 0.2 s episodes (6 control steps), stepped through two auto-resets, every appended row against the host rebuild
  of the drop-in (model.joint_world_positions / model.KinSampler on get_state()); once more on a two-clip dataset where every env samples its own clip.
* end to end, overflow, argument checks, the compiled kernels' resource remarks."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

from deepmimic_amd import model
from deepmimic_amd import time_warp as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "time_warp_vectors.npz")
U32, U64 = 2.0 ** -24, 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- alignment
def golden_batch(dim, dtype):
    """(samples [N, 2, capacity, dim] with NaN behind every env's count, count int32 [N], want float64 [N], capacity) of the golden file"""
    z = np.load(GOLDEN)
    cap, scale, count = int(z["capacity"][0]), float(z["scale"][0]), z["d%d/count" % dim].astype(np.int32)
    samples = np.full((count.size, 2, cap, dim), np.nan, dtype)
    at = 0
    for e, n in enumerate(count):
        samples[e, 0, :n] = z["d%d/sim" % dim][at:at + n] / scale
        samples[e, 1, :n] = z["d%d/kin" % dim][at:at + n] / scale
        at += n
    return samples, count, z["d%d/want" % dim].astype(np.float64), cap


def golden_dims():
    return [int(d) for d in np.load(GOLDEN)["dims"]]


def float_bound(dim, n, want):
    """Forward-error bound of the float kernel's cost against the exact one, from the operation count of one cell (u = 2^-24, first order):
      a coordinate difference rounds once (u); its square carries 2 u + u; the sum of the three squares two more additions: the radicand is within 5 u;
      the square root halves that and adds its own 1 ulp = 2 u (counted as tests/test_math_device.py counts sqrt and division): a point distance is within 4.5 u;
      the J distances are non-negative and added in order, a term passes through at most J - 1 additions: (J - 1) u more; the division by J is 1 ulp = 2 u.
    One cell d(i, j) is therefore within (J + 5.5) u of its exact value, RELATIVE (every term is non-negative).  The table is a min-plus recurrence in fp64: the
    computed cost is at most the computed sum along the true optimal path, <= (1 + eps) * want, and at least the smallest computed path sum, >= (1 - eps) * want --
    a per-cell relative error is not amplified; the 2 n fp64 additions of a path add 2 n 2^-53.  The bound is one notch above: (J + 6) u + 2 n 2^-53, times want."""
    return ((dim // 3 + 6) * U32 + 2 * n * U64) * want


def check_alignment(run, dim, f64, label):
    """run(samples, count, select) -> (reward float32 [N], cost float64 [N]); the golden batch through it, all asserts of the alignment check"""
    samples, count, want, cap = golden_batch(dim, np.float64 if f64 else np.float32)
    reward, cost = run(samples, count, None)
    err = np.abs(cost - want)
    bound = 1e-12 * np.maximum(1.0, want) if f64 else float_bound(dim, count, want)
    worst = int(np.argmax(err / np.where(bound > 0, bound, 1.0)))
    print("TIMEWARP %s dim %d %s: worst |cost - reference| %.3e at n = %d (bound %.3e, want %.6f)" % (label, dim, "f64" if f64 else "f32", err[worst], count[worst], bound[worst], want[worst]))
    assert np.isfinite(cost).all() and (err <= bound).all(), (err, bound)
    assert (cost[count == 1] == 0).all()
    # reward = cost + (capacity - n) * term_step_cost, one rounding to float
    assert np.array_equal(reward, (cost + (cap - count) * 1.0).astype(np.float32))
    # model.time_warp_cost on the same inputs.  numpy's mean adds the J distances pairwise, the kernel (and the reference) in order: equal to the bound the reference
    # itself is held to against it (tests/test_oracle_vs_ref.py), not bit for bit
    for e in np.flatnonzero(count > 1):
        host = model.time_warp_cost(samples[e, 0, :count[e]].astype(np.float64), samples[e, 1, :count[e]].astype(np.float64))
        assert abs(cost[e] - host) <= (1e-12 * max(1.0, host) if f64 else float_bound(dim, count[e], host)), (e, cost[e], host)
    return samples, count, reward, cost


def check_selection(run, dim, f64):
    """unselected rows read 0; selected rows do not depend on their neighbours' data; two runs give the same bytes"""
    samples, count, want, cap = golden_batch(dim, np.float64 if f64 else np.float32)
    reward, cost = run(samples, count, None)
    again = run(samples, count, None)
    assert reward.tobytes() == again[0].tobytes() and cost.tobytes() == again[1].tobytes()
    select = (np.arange(count.size) % 2).astype(np.int32)
    other = samples.copy()
    other[select == 0] = np.nan                                      # the unselected envs' data must not be read ...
    cnt2 = count.copy(); cnt2[select == 0] = cap                      # ... whatever their count says
    r2, c2 = run(other, cnt2, select)
    assert (r2[select == 0] == 0).all() and (c2[select == 0] == 0).all()
    assert r2[select == 1].tobytes() == reward[select == 1].tobytes() and c2[select == 1].tobytes() == cost[select == 1].tobytes()


def emu_runner(emu_lib, f64):
    def run(samples, count, select, tsc=1.0):
        n, _, cap, dim = samples.shape
        reward, cost = np.full(n, -77.0, np.float32), np.full(n, -77.0)
        tw.align_device(n, cap, dim, f64, samples.ctypes.data, count.ctypes.data, select.ctypes.data if select is not None else 0, reward.ctypes.data, cost.ctypes.data,
                        tsc, lib_path=emu_lib)
        return reward, cost
    return run


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_alignment_vs_reference_dtw(emu_lib, f64):
    for dim in golden_dims():
        check_alignment(emu_runner(emu_lib, f64), dim, f64, "emu")


def test_alignment_selection_and_determinism(emu_lib):
    check_selection(emu_runner(emu_lib, True), 45, True)
    check_selection(emu_runner(emu_lib, False), golden_dims()[1], False)


def test_alignment_no_samples_and_term_step_cost(emu_lib):
    """n == 0: reward 0, as the drop-in answers; the shortfall is paid at term_step_cost"""
    samples, count, want, cap = golden_batch(45, np.float64)
    count = count.copy(); count[0] = 0
    reward, cost = emu_runner(emu_lib, True)(samples, count, None, 0.25)
    assert reward[0] == 0 and cost[0] == 0
    assert np.array_equal(reward[1:], (cost[1:] + (cap - count[1:]) * 0.25).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- sampler / end to end
def amp_walk(limit=0.2):
    t = model.load_asset("humanoid3d_walk")
    t.cfg.scene = "imitate_amp"
    t.cfg.time_lim_min = t.cfg.time_lim_max = t.cfg.time_end_lim_min = t.cfg.time_end_lim_max = limit     # 0.2 s: 6 control steps
    return t


def amp_two_clips():
    """walk + spinkick as one dataset forced to imitate_amp (tests/test_facade.py test_imitate_amp_time_warp_multi_clip)"""
    a, b = amp_walk(), model.load_asset("humanoid3d_spinkick")
    t = copy.deepcopy(a)
    t.frames = np.concatenate([a.frames, b.frames])
    t.clip_starts = np.array([0, a.frames.shape[0], a.frames.shape[0] + b.frames.shape[0]], np.int32)
    t.clip_weights = np.array([0.5, 0.5]); t.clip_loops = np.array([int(a.loop), int(b.loop)], np.int32)
    return t


class HostSampler:
    """what the drop-in's _tw_sample does (compat/DeepMimicCore), for env e of a BatchEnv state: (sim row, kin row)"""

    def __init__(self, tables):
        self.t, self.samplers = tables, {}

    def data(self, pose):                                            # BuildTimeWarpData
        jp = model.joint_world_positions(self.t, pose)
        out = jp - jp[0]
        out[0] = (0.0, jp[0][1], 0.0)
        return out.reshape(-1)

    def rows(self, st, clips, e):
        clip = int(clips[e]) if self.t.num_clips > 1 else 0
        if clip not in self.samplers:
            self.samplers[clip] = model.KinSampler(self.t, clip)
        kin = st["kin"][e]
        return self.data(st["pose"][e]), self.data(self.samplers[clip].pose(float(st["clocks"][e][0]), kin[0:3], kin[3:7]))


def rollout(env, tables, steps, sample, align, capacity=None):
    """`steps` control steps with zero actions and auto-reset.  Before every step: sample(restart) -> (samples, count, overflow) as host arrays, and the host rebuild
    of every env's rows from get_state(); behind it align(done) -> reward.  Returns one record per step."""
    host, hs = [None] * env.N, HostSampler(tables)
    cap = tw.buffer_size(tables.cfg, tables.query_rate) if capacity is None else capacity
    restart = np.ones(env.N, np.int32)
    rec = []
    for _ in range(steps):
        st, clips = env.get_state(), env.get_clips()
        samples, count, overflow = sample(restart)
        for e in range(env.N):
            s, k = hs.rows(st, clips, e)
            if restart[e]:
                host[e] = [[s, s], [k, k]]                           # ResetTimeWarper's sample and the first PreUpdate's
            elif len(host[e][0]) < cap:
                host[e][0].append(s); host[e][1].append(k)
        out = env.step(np.zeros((env.N, env.A), np.float32), auto_reset=True)
        done = ((out["episode_end"] != 0) | (out["valid"] == 0)).astype(np.int32)
        reward = align(done)
        rec.append(dict(samples=samples.copy(), count=count.copy(), overflow=int(overflow[0]), restart=restart.copy(), done=done, reward=reward.copy(), clips=clips.copy(),
                        host=[[np.array(h[0]), np.array(h[1])] for h in host], root=np.abs(st["pose"][:, 0:3]).max()))
        restart = done
    return rec


def emu_rollout(emu_lib, tables, n_envs, steps, capacity=None, seed=3):
    from deepmimic_amd.core import BatchEnv
    env = BatchEnv(tables, n_envs, precision=64, seed=seed, test_mode=True, lib_path=emu_lib)
    env.reset()
    cap = tw.buffer_size(tables.cfg, tables.query_rate) if capacity is None else capacity
    elem, dim = tw.dims(env)
    assert (elem, dim) == (8, 3 * env.J)
    samples, count, overflow = np.zeros((n_envs, 2, cap, dim)), np.zeros(n_envs, np.int32), np.zeros(1, np.int32)
    reward = np.zeros(n_envs, np.float32)

    def sample(restart):
        tw.sample_device(env, samples.ctypes.data, count.ctypes.data, restart.ctypes.data, cap, overflow.ctypes.data)
        return samples, count, overflow

    def align(done):
        tw.align_device(n_envs, cap, dim, True, samples.ctypes.data, count.ctypes.data, done.ctypes.data, reward.ctypes.data, 0, lib=env.lib)
        return reward
    rec = rollout(env, tables, steps, sample, align, capacity)
    env.close()
    return rec, cap


@pytest.fixture(scope="module")
def walk_rollout(emu_lib):
    return emu_rollout(emu_lib, amp_walk(), 4, 14)


@pytest.fixture(scope="module")
def clips_rollout(emu_lib):
    return emu_rollout(emu_lib, amp_two_clips(), 4, 14)


def check_sampler(rec, cap, tol):
    """every step's buffers against the host rebuild; counts run 2, 3, ... and return to 2 on the step after `done`"""
    prev, dones = None, 0
    for k, r in enumerate(rec):
        assert r["overflow"] == 0
        for e in range(r["count"].size):
            n = int(r["count"][e])
            assert n == (2 if r["restart"][e] else prev[e] + 1), (k, e, n)
            hs, hk = r["host"][e]
            assert hs.shape[0] == n
            assert np.abs(r["samples"][e, 0, :n] - hs).max() <= tol and np.abs(r["samples"][e, 1, :n] - hk).max() <= tol, (k, e)
            if r["restart"][e]:
                assert np.array_equal(r["samples"][e, :, 0], r["samples"][e, :, 1])
        prev = r["count"]; dones += int(r["done"].sum())
    assert rec[0]["restart"].all() and dones >= 2 * rec[0]["count"].size          # two auto-resets of every env
    return dones


def check_end_to_end(rec, cap, tol):
    """reward at the `done` steps = model.time_warp_cost of the host-rebuilt samples + (capacity - n); 0 elsewhere"""
    seen = 0
    for r in rec:
        for e in range(r["done"].size):
            if not r["done"][e]:
                assert r["reward"][e] == 0
                continue
            hs, hk = r["host"][e]
            want = model.time_warp_cost(hs, hk) + (cap - hs.shape[0])
            assert abs(float(r["reward"][e]) - want) <= tol(hs.shape[0], want), (e, r["reward"][e], want)
            assert r["reward"][e] >= cap - hs.shape[0]                # the alignment cost is not negative
            seen += 1
    assert seen >= 2 * rec[0]["done"].size


def test_sampler_vs_host_rebuild(walk_rollout):
    rec, cap = walk_rollout
    assert cap == 8
    check_sampler(rec, cap, 1e-9)
    assert [int(r["count"][0]) for r in rec[:8]] == [2, 3, 4, 5, 6, 7, 2, 3]


def test_sampler_multi_clip_every_env_its_own_clip(clips_rollout):
    rec, cap = clips_rollout
    check_sampler(rec, cap, 1e-9)
    assert {int(c) for r in rec for c in r["clips"]} == {0, 1}       # both clips were sampled
    assert any(len(set(r["clips"].tolist())) == 2 for r in rec)       # ... side by side in one launch


def test_end_to_end_reward_at_done(walk_rollout, clips_rollout):
    for rec, cap in (walk_rollout, clips_rollout):
        # float32 reward of an fp64 cost: one rounding of a number below 8, plus the 1e-9 of the issue
        check_end_to_end(rec, cap, lambda n, want: 1e-9 + 0.5 * np.spacing(np.float32(want)))


def test_overflow_is_flagged_and_nothing_is_written(emu_lib):
    """capacity 4 over 6 steps: the overflow word is set, count stays at 4, and once every env's block is full no byte of the buffer moves any more -- a row written
    past an env's sim rows would land in its kin rows, one past its kin rows in the next env's block or, for the last env, in the canary rows behind the buffer"""
    from deepmimic_amd.core import BatchEnv
    t = amp_walk()
    env = BatchEnv(t, 4, precision=64, seed=3, test_mode=True, lib_path=emu_lib)
    env.reset()
    cap, dim = 4, 3 * env.J
    buf = np.full(4 * 2 * cap * dim + 2 * dim, -77.0)               # two canary rows behind the last env's block
    samples = buf[:4 * 2 * cap * dim].reshape(4, 2, cap, dim)
    count, overflow, restart = np.zeros(4, np.int32), np.zeros(1, np.int32), np.ones(4, np.int32)
    full = None
    for k in range(6):
        tw.sample_device(env, samples.ctypes.data, count.ctypes.data, restart.ctypes.data, cap, overflow.ctypes.data)
        restart[:] = 0
        assert list(count) == [min(2 + k, cap)] * 4 and int(overflow[0]) == (1 if k > 2 else 0)
        if k == 2:
            full = buf.copy()
            assert not (samples == -77.0).any()
        if k > 2:
            assert buf.tobytes() == full.tobytes()
        env.step(np.zeros((4, env.A), np.float32))
    assert (buf[-2 * dim:] == -77.0).all()
    env.close()


def test_time_warp_class_raises_on_overflow():
    """TimeWarp.check_overflow: the reference throws in AddSample0; the Python layer raises when it reads the word (no device needed for the rule itself)"""
    class Word:
        def __init__(self, v): self.v = v
        def item(self): return self.v
    obj = tw.TimeWarp.__new__(tw.TimeWarp)
    obj.capacity, obj.overflow = 4, Word(0)
    obj.check_overflow()
    obj.overflow = Word(1)
    with pytest.raises(RuntimeError, match="Time warper buffer overflow, capacity: 4"):
        obj.check_overflow()


def test_buffer_size_is_the_build_time_warper_formula():
    t = amp_walk(20.0)
    assert tw.buffer_size(t.cfg, t.query_rate) == 602
    t.cfg.time_lim_max = 0.5; t.cfg.time_end_lim_max = 0.21
    assert tw.buffer_size(t.cfg, 30.0) == 17                        # ceil(30 * max(0.5, 0.21)) + 2
    t.cfg.enable_test_time_warp = False
    assert tw.buffer_size(t.cfg, 30.0) is None and "enable_test_time_warp" in tw.why_no_warper(t.cfg)
    t = model.load_asset("humanoid3d_walk")
    assert tw.buffer_size(t.cfg, 30.0) is None and "imitate_amp" in tw.why_no_warper(t.cfg)
    t = amp_walk(); t.cfg.time_lim_max = np.inf
    assert tw.buffer_size(t.cfg, 30.0) is None and "finite" in tw.why_no_warper(t.cfg)


def test_arguments_are_refused_by_name(emu_lib):
    from deepmimic_amd.core import BatchEnv, load_library
    lib = load_library(emu_lib)
    s, c, r = np.zeros((1, 2, 4, 6)), np.full(1, 2, np.int32), np.full(1, -77.0, np.float32)
    ok = dict(n_envs=1, capacity=4, dim=6, f64=True, samples_ptr=s.ctypes.data, count_ptr=c.ctypes.data, select_ptr=0, reward_ptr=r.ctypes.data, lib=lib)
    for change, msg in ((dict(samples_ptr=0), "dm_time_warp_align: null argument"), (dict(count_ptr=0), "dm_time_warp_align: null argument"),
                        (dict(reward_ptr=0), "dm_time_warp_align: null argument"), (dict(capacity=1), "dm_time_warp_align: capacity must be >= 2"),
                        (dict(dim=7), "dm_time_warp_align: dim must be a positive multiple of 3"), (dict(dim=0), "dm_time_warp_align: dim must be a positive multiple of 3"),
                        (dict(n_envs=0), "dm_time_warp_align: n_envs must be >= 1"), (dict(samples_ptr=s.ctypes.data + 4), "dm_time_warp_align: misaligned pointer"),
                        (dict(capacity=30000), "dm_time_warp_align: capacity and dim need more LDS")):
        with pytest.raises(RuntimeError, match=msg):
            tw.align_device(**dict(ok, **change))
    assert r[0] == -77.0                                             # a refused call launches nothing
    tw.align_device(**ok)
    assert r[0] == 2.0                                               # (two all-zero samples: cost 0 + 2 missing)
    env = BatchEnv(amp_walk(), 1, precision=64, lib_path=emu_lib)
    dim = 3 * env.J
    s, c, o = np.zeros((1, 2, 4, dim)), np.zeros(1, np.int32), np.zeros(1, np.int32)
    for args, msg in (((0, c.ctypes.data, 0, 4, o.ctypes.data), "dm_time_warp_sample: null argument"), ((s.ctypes.data, 0, 0, 4, o.ctypes.data), "dm_time_warp_sample: null argument"),
                      ((s.ctypes.data, c.ctypes.data, 0, 4, 0), "dm_time_warp_sample: null argument"), ((s.ctypes.data, c.ctypes.data, 0, 1, o.ctypes.data), "dm_time_warp_sample: capacity must be >= 2")):
        with pytest.raises(RuntimeError, match=msg):
            tw.sample_device(env, *args)
    assert c[0] == 0 and not s.any()
    assert lib.dm_time_warp_sample(None, None, None, None, 4, None) != 0 and b"dm_time_warp_sample: null ctx" in lib.dm_last_error()
    assert lib.dm_time_warp_dims(None, None) != 0 and b"dm_time_warp_dims: null argument" in lib.dm_last_error()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- resources
def host_resource_remarks(tmp_path_factory):
    """the resource remarks of dm_host.o: those the build left, or of one object rebuilt with the Makefile's flags where build/ is absent"""
    csrc = os.path.join(ROOT, "deepmimic_amd", "csrc")
    path = os.path.join(csrc, "build", "dm_host.o.res")
    if not os.path.exists(path):
        d = str(tmp_path_factory.mktemp("tw_res"))
        subprocess.check_call(["make", "-s", "-C", csrc, "OBJDIR=" + d, os.path.join(d, "dm_host.o")])
        path = os.path.join(d, "dm_host.o.res")
    return open(path).read()


def test_align_kernels_use_no_scratch(tmp_path_factory):
    txt = host_resource_remarks(tmp_path_factory)
    blocks = re.split(r"remark: Function Name: ", txt)
    mine = [b for b in blocks if re.match(r"\S*k_time_warp_align", b)]
    assert len(mine) == 2, "one float and one double instantiation"
    for b in mine:
        fig = {k: int(re.search(pat, b).group(1)) for k, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
                                                                 ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))}
        print("TIMEWARP resources %s %r" % (b.split()[0], fig))
        assert fig["spill"] == 0 and fig["sspill"] == 0 and fig["scratch"] == 0 and fig["vgprs"] <= 128, fig
