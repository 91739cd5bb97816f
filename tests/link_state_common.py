"""The checks of tests/test_link_state.py (CPU emulator) and tests/test_link_state_gpu.py (device): `BatchEnv.link_state` / `dm_link_state` against the reference's
golden vectors, the oracle's forward kinematics and the context's own state.  Every function takes the library path and the precision.

Bounds.  precision 32: the project's bound for the "links" tap (tests/test_ref_golden.py: tol_kin = 5e-6, velocities relative to max(1, |v|max)) -- the tap holds
the same numbers.  precision 64: the outputs are float32 roundings of an fp64 computation that the project holds to 1e-11 against the reference, so
|out - ref| <= 2^-24 |ref| + 1e-11 (one rounding to nearest of a value within 1e-11 of ref; for velocities the 1e-11 is relative to max(1, |v|max), as the tap's)."""
import numpy as np

import parity_common as pc
from deepmimic_amd import link_state as ls
from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv

GOLDEN_SCENES = ("humanoid3d_walk", "dog3d_pace", "humanoid3d_spinkick")
TOL_KIN32, TOL_KIN64, U32 = 5e-6, 1e-11, 2.0 ** -24
DT = 1.0 / 600


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def within(out, ref, precision, vel=False):
    """out (float32) against ref (float64) under the module's bound; returns the worst ratio error / bound"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, np.abs(ref).max()) if vel else 1.0
    bound = TOL_KIN32 * scale if precision == 32 else U32 * np.abs(ref) + TOL_KIN64 * scale
    err = np.abs(out - ref)
    assert (err <= bound).all(), (float(err.max()), float(np.max(bound)))
    return float(np.max(err / bound))


def golden_env(name, precision, lib, n=None):
    """a context holding the golden states of `name`, set as parity_common.check_device_vs_ref_golden sets them: (env, G)"""
    g = pc.ref_golden()
    G = lambda k: g["%s/%s" % (name, k)]
    n = G("pose").shape[0] if n is None else n
    env = BatchEnv(model.load_asset(name), n, precision=precision, lib_path=lib)
    tk = G("kin_time")[:n]
    clocks = np.stack([tk, tk, np.zeros(n), np.zeros(n), np.full(n, np.inf)], axis=1)
    flags = np.tile(np.array([[1, 0, 1, 1]], dtype=np.int32), (n, 1))
    env.reset(kin_times=tk, max_times=np.inf)
    env.set_state(pose=G("pose")[:n], vel=G("vel")[:n], tar=G("tar")[:n], kin=G("kin_origin")[:n], clocks=clocks, flags=flags)
    return env, G


def check_links(links, envrow, body_world, joint_world, link_vel, com, com_vel, precision):
    """one env: links [J, 22] and env [8] against the reference's (or the oracle's) forward kinematics of the same pose"""
    w = [within(links[:, 0:3], body_world[:, 9:12], precision), within(links[:, 3:12], body_world[:, 0:9], precision),
         within(links[:, 18:21], joint_world[:, 9:12], precision), within(links[:, 12:18], link_vel, precision, vel=True),
         within(envrow[0:3], com, precision), within(envrow[3:6], com_vel, precision, vel=True)]
    return max(w)


def sim_side_vs_reference(lib, precision, label):
    for name in GOLDEN_SCENES:
        env, G = golden_env(name, precision, lib)
        out = env.link_state(0)
        assert out["links"].dtype == np.float32 and out["links"].shape == (env.N, env.J, 22) and out["env"].shape == (env.N, 8)
        worst = 0.0
        for e in range(env.N):
            worst = max(worst, check_links(out["links"][e], out["env"][e], G("body_world")[e], G("joint_world")[e], G("link_vel")[e], G("com")[e], G("com_vel")[e], precision))
        print("LINKSTATE %s %s f%d sim: worst error / bound %.3f" % (label, name, precision, worst))
        # pose / vel: the float32 rounding of the state that was set, exactly (fp32 context: the state is stored as float32)
        assert same_bits(out["pose"], G("pose").astype(np.float32)) and same_bits(out["vel"], G("vel").astype(np.float32))
        assert (out["links"][:, :, 21] == 0).all() and (out["env"][:, 7] == 0).all()      # (the state was set with an empty contact mask)
        env.close()


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def heading_vs_origin_trans(lib, precision):
    from ref_lib import Components, Skel
    orc = Components("orc")
    for name in GOLDEN_SCENES:
        env, G = golden_env(name, precision, lib)
        sk = Skel(orc, env.tables)
        out = env.link_state(0)
        for e in range(env.N):
            want = sk.origin_trans(G("pose")[e])[0:9].reshape(3, 3)
            got = rot_y(-float(out["env"][e, 6]))
            assert np.abs(got - want).max() < TOL_KIN32, (name, e, np.abs(got - want).max())
        env.close()


def kin_side(lib, precision, label):
    from ref_lib import Components, Skel
    orc = Components("orc")
    for name in GOLDEN_SCENES:
        env, G = golden_env(name, precision, lib)
        sk = Skel(orc, env.tables)
        out = env.link_state(1)
        worst = 0.0
        for e in range(env.N):
            kp, kv = G("kin_pose")[e], G("kin_vel")[e]
            # the rule of the kin_pose / kin_vel taps (pose absolute, velocity relative to max(1, |v|max)); fp64: + the rounding of the output to float32
            within(out["pose"][e], kp, precision); within(out["vel"][e], kv, precision, vel=True)
            # the link state is the forward kinematics of the emitted float32 pose: the oracle's Skel on exactly that pose, the bounds of the simulated side.
            # An fp32 context computed on these very numbers.  An fp64 context computed on its fp64 pose, of which the emitted one is the float32 rounding
            # (2^-24 per pose element, times a lever arm of the order of 1 m in a link position): the emitted pose gets the fp32 bound there, and the fp64 bound is
            # asked of the forward kinematics of the golden kinematic pose, which the outputs above hold the device's own within 1e-11 of.
            p, v = out["pose"][e].astype(np.float64), out["vel"][e].astype(np.float64)
            jw, bw = sk.world_trans(p)
            com, comv = sk.com(p, v)
            worst = max(worst, check_links(out["links"][e], out["env"][e], bw, jw, sk.link_vel(p, v), com, comv, 32))
            if precision == 64:
                jw, bw = sk.world_trans(kp)
                com, comv = sk.com(kp, kv)
                worst = max(worst, check_links(out["links"][e], out["env"][e], bw, jw, sk.link_vel(kp, kv), com, comv, 64))
        assert (out["links"][:, :, 21] == 0).all()
        print("LINKSTATE %s %s f%d kin: worst error / bound %.3f" % (label, name, precision, worst))
        env.close()


def kin_side_multi_clip(lib, precision):
    """amp_heading_clips4, N = 4: every env's kinematic pose is the one of its own clip -- Oracle.kin_state() of an oracle put on that env with its clip"""
    from oracle_lib import Oracle
    t = model.load_asset("amp_heading_clips4")
    env = BatchEnv(t, 4, precision=precision, lib_path=lib, seed=17)
    env.reset()
    clips = env.get_clips()
    assert len(set(int(c) for c in clips)) >= 2, clips
    st, out = env.get_state(), env.link_state(1)
    for e in range(env.N):
        o = Oracle(t)
        o.goal_rng(17, e, 0)
        o.reset_ex(float(st["clocks"][e, 0]), np.inf, int(clips[e]), 0.0)
        o.set_full_state(st["pose"][e], st["vel"][e], st["tar"][e], st["kin"][e], st["clocks"][e], st["flags"][e])
        kp, kv, _ = o.kin_state()
        within(out["pose"][e], kp, precision); within(out["vel"][e], kv, precision, vel=True)
    env.close()


def contact_column(lib, precision):
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 3, precision=precision, lib_path=lib, seed=3)
    env.reset()
    env.step(None, DT, 20, open_loop=True)
    mask = env.get_state()["flags"][:, 1]
    bits = ((mask[:, None] >> np.arange(env.J)[None, :]) & 1).astype(np.float32)
    assert bits.any() and not bits.all(), mask                     # on the flags, not on the output: some link touches the ground, some link does not
    assert same_bits(env.link_state(0)["links"][:, :, 21], bits)
    assert (env.link_state(1)["links"][:, :, 21] == 0).all()
    env.close()


def free_body(lib, precision):
    env = BatchEnv(model.load_asset("amp_dribble_zombie"), 2, precision=precision, lib_path=lib, seed=5)
    env.reset()
    env.step(None, DT, 20, open_loop=True, amp=True)
    assert ls.dims(env) == (env.J, 22, 8, env.P, 13)
    out = env.link_state(0)
    assert same_bits(out["obj"], env.get_obj_state().astype(np.float32))
    assert "obj" not in env.link_state(1)
    env.close()


def shapes(lib, precision, alloc):
    """alloc(array) -> (address, read() -> numpy array): device memory holding a copy of `array`"""
    t = model.load_asset("humanoid3d_walk")
    env, G = golden_env("humanoid3d_walk", precision, lib, n=3)
    assert ls.dims(env) == (env.J, 22, 8, env.P, 0)
    J, P, N, PAD = env.J, env.P, env.N, 7
    widths = {"links": J * 22, "env": 8, "pose": P, "vel": P}
    order = ("links", "env", "pose", "vel")

    def run(which, names):
        bufs = {k: alloc(np.full(N * widths[k] + PAD, -77.0, np.float32)) for k in names}
        ls.link_state_device(env, which, *[bufs[k][0] if k in bufs else 0 for k in order])
        env.synchronize()
        return {k: bufs[k][1]() for k in names}

    for which in (0, 1):
        full = run(which, order)
        for k in order:
            assert (full[k][N * widths[k]:] == -77.0).all(), k                # sentinels behind the last row
            assert not (full[k][:N * widths[k]] == -77.0).all(), k
            alone = run(which, (k,))                                          # each output alone, the others NULL
            assert same_bits(alone[k], full[k]), (which, k)
        again = run(which, order)                                             # two runs, the same bytes
        assert all(same_bits(again[k], full[k]) for k in order)
        # row e of the N = 3 context == the single row of an N = 1 context in the same state
        st = env.get_state()
        for e in range(N):
            one = BatchEnv(t, 1, precision=precision, lib_path=lib)
            one.reset(kin_times=st["clocks"][e:e + 1, 0], max_times=np.inf)
            one.set_state(pose=st["pose"][e], vel=st["vel"][e], tar=st["tar"][e], kin=st["kin"][e], clocks=st["clocks"][e], flags=st["flags"][e])
            o1 = one.link_state(which)
            for k in order:
                assert same_bits(o1[k].ravel(), full[k][e * widths[k]:(e + 1) * widths[k]]), (which, e, k)
            one.close()
    env.close()


def refusals(lib, precision):
    import pytest
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=precision, lib_path=lib)
    env.reset()
    buf = np.zeros(64, np.float32)          # never written: every call below is refused before a launch
    for which in (-1, 2):
        with pytest.raises(RuntimeError, match="dm_link_state: which must be 0"):
            ls.link_state_device(env, which, 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dm_link_state: obj_dev on a context without a free body"):
        ls.link_state_device(env, 0, 0, 0, 0, 0, buf.ctypes.data)
    with pytest.raises(RuntimeError, match="dm_reset_where: null mask_dev"):
        ls.reset_where_device(env, 0, buf.ctypes.data, 0)
    with pytest.raises(RuntimeError, match="dm_reset_where: null states_dev"):
        ls.reset_where_device(env, buf.ctypes.data, 0, 0)
    with pytest.raises(RuntimeError, match="dm_reset_where: goals_dev on a scene without a goal"):
        ls.reset_where_device(env, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    from deepmimic_amd.core import TAPE_STRIDE
    env.set_draw_tape(np.zeros((env.N, TAPE_STRIDE)))
    with pytest.raises(RuntimeError, match="dm_reset_where: a draw tape is bound"):
        ls.reset_where_device(env, buf.ctypes.data, buf.ctypes.data, 0)
    env.set_draw_tape(None)
    assert (buf == 0).all()
    env.close()
