"""The checks of tests/test_kin_query.py (CPU emulator) and tests/test_kin_query_gpu.py (device): `BatchEnv.kin_query` / `dm_kin_query` against `dm_link_state`
(which = 1), against itself under its flags, and against the oracle's cKinCharacter::CalcPose / CalcVel and forward kinematics.  Every function takes the library
path and the precision.  N = 3 (4 for the multi-clip dataset), K in {1, 3}.

Byte-exact, no tolerance: an offset of 0 is dm_link_state(which = 1) on all four outputs; frame k of a K = 3 call is the K = 1 call with that offset; rows of N = 3
are three N = 1 contexts; TIMES_PER_ENV with identical rows is the shared form; TIMES_ABSOLUTE with clock + offset (the same float64 addition on the host) is the
relative call; each output alone between sentinels and two runs give the same bytes.

Against the oracle, at the bounds of tests/link_state_common.py (`within`, unchanged): pose and velocity against Oracle.kin_eval(t), links / COM / heading against
Skel on the emitted pose, as link_state_common.kin_side does.  Times per env: one control step ahead, just past the end of the current cycle, just before clip time
0, exactly a key-frame time, two cycles ahead; for a clip that does not loop also past its end, where the velocity is exactly 0."""
import numpy as np

import link_state_common as lc
from deepmimic_amd import kin_query as kq
from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv

DT = 1.0 / 600
SEED = 17
ORDER = ("links", "env", "pose", "vel")
ORACLE_ASSETS = ("humanoid3d_walk", "dog3d_pace", "amp_strike_punch", "amp_heading_clips4", "amp_dribble_zombie")
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def n_of(name):
    return 4 if name == "amp_heading_clips4" else 3


def make_env(name, precision, lib, n=None, steps=2):
    """a context of `name` a few control steps into its episodes (device-drawn starts: every env at its own clip time, a multi-clip env on its own clip)"""
    t = model.load_asset(name)
    env = BatchEnv(t, n_of(name) if n is None else n, precision=precision, lib_path=lib, seed=SEED)
    env.reset(max_times=np.inf)
    for _ in range(steps):
        env.step(None, DT, 20, open_loop=True)
    return t, env


def assert_same(a, b, what):
    for k in ORDER:
        assert lc.same_bits(a[k], b[k]), (what, k)


def frame(out, k):
    return {key: out[key][:, k] for key in ORDER}


def zero_offset_equals_link_state(name, lib, precision):
    t, env = make_env(name, precision, lib)
    want = env.link_state(1)
    one = env.kin_query([0.0])
    assert one["links"].shape == (env.N, 1, env.J, 22) and one["env"].shape == (env.N, 1, 8) and one["pose"].shape == (env.N, 1, env.P)
    assert all(one[k].dtype == np.float32 for k in ORDER)
    assert_same(frame(one, 0), want, "K = 1")
    three = env.kin_query([0.0, 0.0, 0.0])
    for k in range(3):
        assert_same(frame(three, k), want, "K = 3, frame %d" % k)
    assert (three["links"][..., 21] == 0).all() and (three["env"][..., 7] == 0).all()
    env.close()


def frames_and_flags(name, lib, precision):
    t, env = make_env(name, precision, lib)
    offs = np.array([1.0 / 30, -0.25, 0.7])
    three = env.kin_query(offs)
    for k in range(3):                                          # frame k of a K = 3 call == the K = 1 call with that offset
        assert_same(frame(three, k), frame(env.kin_query(offs[k:k + 1]), 0), "frame %d" % k)
    assert not lc.same_bits(three["pose"][:, 0], three["pose"][:, 1])
    per_env = env.kin_query(np.tile(offs, (env.N, 1)))          # TIMES_PER_ENV with identical rows == the shared form
    assert_same(per_env, three, "per env")
    clk = env.get_state()["clocks"][:, 0]
    absolute = env.kin_query(clk[:, None] + offs[None, :], absolute=True)      # the same float64 addition on the host
    assert_same(absolute, three, "absolute")
    again = env.kin_query(offs)                                 # the query changed nothing in the context
    assert_same(again, three, "again")
    env.close()


def rows_equal_single_env_contexts(lib, precision):
    t, env = make_env("humanoid3d_walk", precision, lib)
    offs = np.array([1.0 / 30, -0.25, 0.7])
    full, st = env.kin_query(offs), env.get_state()
    for e in range(env.N):
        one = BatchEnv(t, 1, precision=precision, lib_path=lib)
        one.reset(kin_times=st["clocks"][e:e + 1, 0], max_times=np.inf)
        one.set_state(pose=st["pose"][e], vel=st["vel"][e], tar=st["tar"][e], kin=st["kin"][e], clocks=st["clocks"][e], flags=st["flags"][e])
        o1 = one.kin_query(offs)
        for k in ORDER:
            assert lc.same_bits(o1[k][0], full[k][e]), (e, k)
        one.close()
    env.close()


def shapes(lib, precision, alloc):
    """alloc(array) -> (address, read() -> numpy array): device memory holding a copy of `array`.  Each output alone between sentinels; two runs."""
    t, env = make_env("humanoid3d_walk", precision, lib)
    N, J, P, PAD, SENT = env.N, env.J, env.P, 7, -77.0
    for K in (1, 3):
        widths = {"links": K * J * 22, "env": K * 8, "pose": K * P, "vel": K * P}
        times = alloc(np.array([1.0 / 30, -0.25, 0.7][:K], dtype=np.float64))

        def run(names):
            bufs = {k: alloc(np.full(PAD + N * widths[k] + PAD, SENT, np.float32)) for k in names}
            kq.kin_query_device(env, K, times[0], 0, 0, *[bufs[k][0] + 4 * PAD if k in bufs else 0 for k in ORDER])
            env.synchronize()
            return {k: bufs[k][1]() for k in names}

        full = run(ORDER)
        for k in ORDER:
            body = full[k][PAD:PAD + N * widths[k]]
            assert (full[k][:PAD] == SENT).all() and (full[k][PAD + N * widths[k]:] == SENT).all(), (K, k)      # sentinels in front of the first and behind the last row
            assert not (body == SENT).any(), (K, k)
            assert lc.same_bits(run((k,))[k], full[k]), (K, k)                                                    # each output alone, the others NULL
        again = run(ORDER)
        assert all(lc.same_bits(again[k], full[k]) for k in ORDER), K
        host = env.kin_query([1.0 / 30, -0.25, 0.7][:K])
        assert all(lc.same_bits(host[k].ravel(), full[k][PAD:PAD + N * widths[k]]) for k in ORDER), K
    env.close()


def oracle_for(t, env, e, st, clip, origin=None):
    """an oracle put on env e of `env` (its clip `clip`), optionally about another origin"""
    from oracle_lib import Oracle
    o = Oracle(t)
    if env._has_goal_row:
        o.goal_rng(SEED, e, 0)
        o.reset_ex(float(st["clocks"][e, 0]), np.inf, int(clip), 0.0)
    o.set_full_state(st["pose"][e], st["vel"][e], st["tar"][e], st["kin"][e] if origin is None else origin, st["clocks"][e], st["flags"][e])
    return o


def times_of(t, clip, clk):
    """the absolute clip times of one env (module text) and the indices of those at or past the end of a clip that does not loop"""
    ks = model.KinSampler(t, int(clip))
    dur = t.clip_duration(int(clip))
    cyc = np.floor(clk / dur)
    times = [clk + 1.0 / 30, (cyc + 1) * dur + 1e-3, -1e-3, float(ks.times[3]), clk + 2 * dur]
    rest = []
    if not ks.loop:
        times += [-0.05, dur, dur + 0.05]
        rest = [len(times) - 2, len(times) - 1]
    return times, rest, ks.loop


def check_frame(sk, o, tm, out, e, k, precision):
    kp, kv = o.kin_eval(float(tm))
    pose, vel = out["pose"][e, k], out["vel"][e, k]
    w = [lc.within(pose, kp, precision), lc.within(vel, kv, precision, vel=True)]
    # links of the emitted float32 pose at the fp32 bound; an fp64 context also against the oracle's own pose at the fp64 bound (link_state_common.kin_side)
    for p, v, prec in ((pose.astype(np.float64), vel.astype(np.float64), 32),) + (((kp, kv, 64),) if precision == 64 else ()):
        jw, bw = sk.world_trans(p)
        com, comv = sk.com(p, v)
        w.append(lc.check_links(out["links"][e, k], out["env"][e, k], bw, jw, sk.link_vel(p, v), com, comv, prec))
    want = sk.origin_trans(pose.astype(np.float64))[0:9].reshape(3, 3)
    assert np.abs(lc.rot_y(-float(out["env"][e, k, 6])) - want).max() < lc.TOL_KIN32
    return max(w)


def chunks(K):
    """a list of K times as calls of 3 and 1"""
    i, out = 0, []
    while i < K:
        n = 3 if K - i >= 3 else 1
        out.append((i, n)); i += n
    return out


def query_chunked(env, times, **kw):
    """times [N, K] through calls of K = 3 and K = 1, stitched"""
    parts = [env.kin_query(times[:, i:i + n], absolute=True, **kw) for i, n in chunks(times.shape[1])]
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in ORDER}


def against_oracle(name, lib, precision, label):
    from ref_lib import Components, Skel
    t, env = make_env(name, precision, lib)
    sk = Skel(Components("orc"), t)
    st = env.get_state()
    clips = env.get_clips() if env._has_goal_row else np.zeros(env.N, np.int32)
    if name == "amp_heading_clips4":
        assert len(set(int(c) for c in clips)) >= 2, clips
    per_env = [times_of(t, clips[e], float(st["clocks"][e, 0])) for e in range(env.N)]
    K = max(len(p[0]) for p in per_env)
    times = np.array([p[0] + [p[0][0]] * (K - len(p[0])) for p in per_env])
    out = query_chunked(env, times)
    ident = query_chunked(env, times, identity_origin=True)
    worst = 0.0
    for e in range(env.N):
        o, oi = oracle_for(t, env, e, st, clips[e]), oracle_for(t, env, e, st, clips[e], origin=IDENTITY)
        for k, tm in enumerate(per_env[e][0]):
            worst = max(worst, check_frame(sk, o, tm, out, e, k, precision), check_frame(sk, oi, tm, ident, e, k, precision))
        for k in per_env[e][1]:                                   # at and past the end of a clip that does not loop: at rest, exactly
            assert (out["vel"][e, k] == 0).all() and (ident["vel"][e, k] == 0).all(), (e, k)
    if name == "amp_strike_punch":
        assert not per_env[0][2], "amp_strike_punch is expected not to loop (read from the tables)"
    if name == "humanoid3d_walk":
        assert per_env[0][2]
    print("KINQUERY %s %s f%d: worst error / bound %.3f" % (label, name, precision, worst))
    env.close()


def other_clip_against_oracle(lib, precision, label):
    """amp_heading_clips4: clips_dev names the NEXT clip of the dataset for every env, about the env's own origin"""
    from ref_lib import Components, Skel
    name = "amp_heading_clips4"
    t, env = make_env(name, precision, lib)
    sk = Skel(Components("orc"), t)
    st = env.get_state()
    other = ((env.get_clips() + 1) % t.num_clips).astype(np.int32)
    per_env = [times_of(t, other[e], float(st["clocks"][e, 0]))[0][:3] for e in range(env.N)]
    times = np.array(per_env)
    out = env.kin_query(times, clips=other, absolute=True)
    own = env.kin_query(times, absolute=True)
    assert not lc.same_bits(out["pose"], own["pose"])
    worst = 0.0
    for e in range(env.N):
        o = oracle_for(t, env, e, st, other[e])
        for k, tm in enumerate(per_env[e]):
            worst = max(worst, check_frame(sk, o, tm, out, e, k, precision))
    print("KINQUERY %s %s f%d other clip: worst error / bound %.3f" % (label, name, precision, worst))
    env.close()


def invalid_inputs(lib, precision):
    """CPU emulator only: a non-finite time or a clip id outside the dataset gives NaN rows for that (env, k) and leaves every other row alone"""
    t, env = make_env("amp_heading_clips4", precision, lib)
    N = env.N
    good = env.kin_query(np.tile([0.1, 0.2, 0.3], (N, 1)), absolute=True)
    times = np.tile([0.1, 0.2, 0.3], (N, 1))
    times[0, 1], times[1, 2], times[2, 0] = np.nan, np.inf, -np.inf
    out = env.kin_query(times, absolute=True)
    bad = ~np.isfinite(times)
    for k in ORDER:
        flat = out[k].reshape(N, 3, -1)
        assert np.isnan(flat[bad]).all(), k
        assert lc.same_bits(flat[~bad], good[k].reshape(N, 3, -1)[~bad]), k
    rel = env.kin_query([np.nan])                                  # a relative NaN offset, shared by all envs
    assert all(np.isnan(rel[k]).all() for k in ORDER)
    clips = env.get_clips().astype(np.int32)
    same = env.kin_query(np.tile([0.1, 0.2, 0.3], (N, 1)), clips=clips, absolute=True)
    for k in ORDER:
        assert lc.same_bits(same[k], good[k]), k                   # clips_dev naming the env's own clip == NULL
    for wrong in (-1, t.num_clips, 2 ** 30, -2 ** 31):
        c = clips.copy(); c[1] = wrong
        out = env.kin_query(np.tile([0.1, 0.2, 0.3], (N, 1)), clips=c, absolute=True)
        for k in ORDER:
            assert np.isnan(out[k][1]).all(), (wrong, k)
            assert lc.same_bits(np.delete(out[k], 1, axis=0), np.delete(good[k], 1, axis=0)), (wrong, k)
    env.close()


def refusals(lib, precision):
    import pytest
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=precision, lib_path=lib)
    env.reset()
    buf = np.zeros(64, np.float64)          # never written or read: every call below is refused before a launch
    a = buf.ctypes.data
    with pytest.raises(RuntimeError, match="dm_kin_query: null times_dev"):
        kq.kin_query_device(env, 1, 0, 0, 0, a, 0, 0, 0)
    for K in (0, -1, 65):
        with pytest.raises(RuntimeError, match="dm_kin_query: K must be in"):
            kq.kin_query_device(env, K, a, 0, 0, a, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dm_kin_query: unknown flag bits"):
        kq.kin_query_device(env, 1, a, 0, 8, a, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dm_kin_query: clips_dev needs DM_KIN_TIMES_ABSOLUTE"):
        kq.kin_query_device(env, 1, a, a, kq.TIMES_PER_ENV, a, 0, 0, 0)
    assert env.lib.dm_kin_query(None, 1, a, None, 0, None, None, None, None) != 0
    assert (buf == 0).all()
    env.close()
