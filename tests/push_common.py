"""The checks of tests/test_push_where.py for task-chosen pushes (include/dm_hip.h dm_push_where / dm_push_state, deepmimic_amd/pushes.py), through BatchEnv.push /
clear_pushes / push_state: host arrays, so every check runs on the CPU emulator and on the device.  The rows a push writes are compared byte for byte with rows built by
hand (`slot_row` of tests/test_perturbs.py) and handed in through set_perturb_state; what the step kernels do with the rows is theirs and stays held by
tests/test_perturbs.py.  Open-loop steps throughout."""
import ctypes as C
import math

import numpy as np
import pytest

from deepmimic_amd import model, pushes, streams
from deepmimic_amd.core import BatchEnv
from oracle_lib import Oracle
from test_episode_reset import assert_same, extras, same_bits
from test_perturbs import active, perturbed, slot_row
from test_physics_validity import box_tables

DT = 1.0 / 600
G = 9.8
SEED = 17
PT_TIMER, PT_NEXT, PT_DRAWS, PT_KSEED = 0, 1, 2, 15      # dm_types.h
# (asset, N, wave_packing, physics) of check 2: two per wavefront, one per wavefront (odd N), packing 1, the dog (large class), DM-physics v2
SHAPES = [("humanoid3d_walk", 4, 0, 1), ("humanoid3d_walk", 3, 0, 1), ("humanoid3d_walk", 4, 1, 1), ("dog3d_pace", 2, 0, 1), ("humanoid3d_walk", 4, 0, 2)]


def push_tables(asset="humanoid3d_walk"):
    t = model.load_asset(asset)
    t.cfg.task_pushes = True
    return t


def make(lib, prec, n=4, asset="humanoid3d_walk", packing=0, physics=1, limit=None, seed=SEED, tables=None):
    env = BatchEnv(tables if tables is not None else push_tables(asset), n, precision=prec, lib_path=lib, seed=seed, wave_packing=packing, physics=physics)
    if limit is not None:
        env.set_time_limits(limit, limit)
    env.reset()
    return env


def step(env, n=20, auto_reset=False):
    return env.step(None, DT, n, auto_reset=auto_reset, end_early=True, open_loop=True)


def slots_of(row):
    """the two slots of a perturbation row as push_state shows them (float64)"""
    out = np.zeros((2, 6))
    for i in range(2):
        s = row[3 + 6 * i: 9 + 6 * i]
        out[i] = [s[0] - 1, s[1], s[2], s[3], s[4], s[5]] if s[0] > 0 else [-1, 0, 0, 0, 0, 0]
    return out


def assert_state_shows_rows(env):
    rows, ps = env.get_perturb_state(), env.push_state()
    assert ps.dtype == np.float32 and ps.shape == (env.N, 2, 6)
    want = np.array([slots_of(r) for r in rows]).astype(np.float32)
    assert same_bits(ps, want)


# ---------------------------------------------------------------------------------------------------------------- 1: closed form
def closed_form(lib, prec, tol):
    """tests/test_perturbs.py::_device_box with the forces placed by BatchEnv.push: dv = f / m n dt + g k dt, no angular velocity"""
    t = box_tables(mass=10.0); t.cfg.task_pushes = True
    env = BatchEnv(t, 2, precision=prec, lib_path=lib, wave_packing=1, seed=5)
    assert env.has_pushes
    env.reset(kin_times=[0.0] * 2, max_times=np.inf)
    rows = env.get_perturb_state()
    assert (rows[:, PT_TIMER] == 0).all() and np.isinf(rows[:, PT_NEXT]).all() and (rows[:, 3] == 0).all() and (rows[:, 9] == 0).all()
    st = env.get_state(); P = st["pose"].copy(); P[:, 1] = 50.0
    env.set_state(pose=P, vel=st["vel"])
    f = np.array([20.0, 5.0, -10.0])
    assert env.push([1, 1], 0, f, 0.0492) == 0                             # acts for ceil(0.0492 / dt) = 30 updates
    assert env.push([0, 1], 0, -0.5 * f, 0.0192) == 0                      # env 1, two at once: 12 updates of f / 2, then f
    step(env, 40)
    v = env.get_state()["vel"]
    g = np.array([0, -G, 0]) * 40 * DT
    assert np.abs(v[0, :3] - (f / 10 * 30 * DT + g)).max() < tol, v[0, :3]
    assert np.abs(v[1, :3] - (f / 10 * (30 - 0.5 * 12) * DT + g)).max() < tol, v[1, :3]
    assert np.abs(v[:, 3:6]).max() < tol
    rows = env.get_perturb_state()
    assert (rows[:, 3] == 0).all() and (rows[:, 9] == 0).all() and np.abs(rows[:, PT_TIMER] - 40 * DT).max() < 1e-12 and np.isinf(rows[:, PT_NEXT]).all()
    assert (env.push_state()[:, :, 0] == -1).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2: the host route, byte for byte
def equals_host_route(lib, prec, asset, n, packing, physics):
    """context A is pushed by dm_push_where, context B gets hand-built rows through set_perturb_state: the same rows at once, the same bytes after three control steps
    through an auto-reset (time limit 0.08 s: every episode ends inside the third step and the reset clears what still acts, the +inf push included)"""
    a, b = (make(lib, prec, n, asset, packing, physics, limit=0.08) for _ in range(2))
    J = a.J
    rng = np.random.default_rng(3)
    mask = np.ones(n, np.int32); mask[1] = 0                               # env 1 is left out
    links = rng.integers(0, J, n).astype(np.int32)
    forces = rng.normal(size=(n, 3)) * 80.0                                # (arbitrary doubles: stored as given)
    durs = np.array([0.0492, 0.3, np.inf, 0.02])[:n]
    before = a.get_perturb_state()
    assert a.push(mask, links, forces, durs) == 0
    rows = b.get_perturb_state()
    assert same_bits(rows, before)
    for e in range(n):
        if mask[e]:
            rows[e] = slot_row(timer=rows[e, 0], nxt=rows[e, 1], draws=rows[e, 2], slots=[(links[e], forces[e], durs[e], 0.0)])
    b.set_perturb_state(rows)
    got = a.get_perturb_state()
    assert same_bits(got, b.get_perturb_state()) and same_bits(got[1], before[1])
    links2 = ((links + 1) % J).astype(np.int32)                             # a second force beside the first, on the envs with an even index
    mask2 = (np.arange(n) % 2 == 0).astype(np.int32)
    assert a.push(mask2, links2, -forces, 0.05) == 0
    for e in range(n):
        if mask2[e]:
            rows[e] = slot_row(timer=rows[e, 0], nxt=rows[e, 1], draws=rows[e, 2], slots=[(links[e], forces[e], durs[e], 0.0), (links2[e], -forces[e], 0.05, 0.0)])
    b.set_perturb_state(rows)
    assert same_bits(a.get_perturb_state(), b.get_perturb_state())
    ended = np.zeros(n, bool)
    for k in range(3):
        oa, ob = step(a, auto_reset=True), step(b, auto_reset=True)
        assert_same(oa, ob, k)
        assert_same(a.get_state(), b.get_state(), k)
        assert_same(extras(a), extras(b), k)
        ended |= oa["episode_end"] != 0
    assert ended.all() and (a.push_state()[:, :, 0] == -1).all()
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 3: the slot rule and clearing
def slot_rule(lib, prec):
    env = make(lib, prec, 4)
    n, f = 4, np.array([[10.0, 0, 0], [0, 20.0, 0], [0, 0, 30.0], [5.0, 5.0, 5.0]])
    all_, free = np.ones(n, np.int32), np.zeros((n, 6)); free[:, 0] = -1
    base = env.get_perturb_state()
    # both free: the lowest index
    assert env.push(all_, [1, 2, 3, 4], f, [0.5, 0.2, 0.5, 0.2]) == 0
    ps = env.push_state().astype(np.float64)
    assert (ps[:, 0, 0] == [1, 2, 3, 4]).all() and same_bits(ps[:, 0, 1:4], f) and same_bits(ps[:, 1], free)
    # one busy: the free one -- here with a NULL slots array, then with -1 (env 3 is cleared first)
    assert env.push(all_, 5, 2 * f, [0.2, 0.5, 0.2, 0.5]) == 0
    assert env.push([0, 0, 0, 1], -1, 0.0, 0.0, slots=1) == 0
    assert env.push([0, 0, 0, 1], 5, 2 * f, 0.5, slots=-1) == 0
    ps = env.push_state().astype(np.float64)
    assert (ps[:, 0, 0] == [1, 2, 3, 4]).all() and (ps[:, 1, 0] == 5).all() and same_bits(ps[:, 1, 1:4], 2 * f)
    assert_state_shows_rows(env)
    # both busy: one control step later elapsed is 20 dt in both, the slot nearest its end is the one with the smaller duration: slot 1 of envs 0 and 2, slot 0 of 1 and 3
    step(env)
    ps = env.push_state().astype(np.float64)
    assert np.abs(ps[:, :, 5] - 20 * DT).max() < 1e-6 and (ps[:, :, 0] >= 0).all()
    assert env.push(all_, 7, 3 * f, 1.0) == 0
    ps = env.push_state().astype(np.float64)
    for e in range(n):
        new, old = (1, 0) if e % 2 == 0 else (0, 1)
        assert ps[e, new, 0] == 7 and same_bits(ps[e, new, 1:4], 3 * f[e]) and ps[e, new, 4] == 1.0 and ps[e, new, 5] == 0.0, e
        assert ps[e, old, 0] == (e + 1 if old == 0 else 5) and abs(ps[e, old, 5] - 20 * DT) < 1e-6, e
    assert_state_shows_rows(env)
    # explicit slots override the rule: slot 1 of envs 0 and 2 would be the last to end now
    assert env.push([1, 0, 1, 0], 9, f, 0.01, slots=[1, 0, 1, 0]) == 0
    ps = env.push_state()
    assert (ps[[0, 2], 1, 0] == 9).all() and (ps[[0, 2], 0, 0] == [1, 3]).all() and (ps[[1, 3], :, 0] != 9).all()
    # clearing: slot 0 of env 0, slot 1 of env 1, both of env 2; env 3 is not selected
    keep = env.get_perturb_state()
    assert env.push([1, 1, 1, 0], -1, 0.0, 0.0, slots=[0, 1, -1, -1]) == 0
    rows, ps = env.get_perturb_state(), env.push_state()
    assert (ps[0, :, 0] == [-1, 9]).all() and (ps[1, :, 0] == [7, -1]).all() and (ps[2, :, 0] == [-1, -1]).all() and same_bits(rows[3], keep[3])
    want = keep.copy(); want[0, 3] = 0; want[1, 9] = 0; want[2, 3] = 0; want[2, 9] = 0       # only the link word of a freed slot changes, as pert_reset frees it
    assert same_bits(rows, want)
    assert env.clear_pushes([0, 0, 0, 1]) == 0 and (env.push_state()[:, :, 0] == [[-1, 9], [7, -1], [-1, -1], [-1, -1]]).all()
    assert env.clear_pushes() == 0 and (env.push_state()[:, :, 0] == -1).all()
    rows = env.get_perturb_state()
    assert same_bits(rows[:, [PT_NEXT, PT_DRAWS, PT_KSEED]], base[:, [PT_NEXT, PT_DRAWS, PT_KSEED]]) and np.abs(rows[:, PT_TIMER] - 20 * DT).max() < 1e-12
    env.close()
    # two calls, the same bytes: on two contexts of one seed, and the same call once more (the rule then names the other slot)
    a, b = make(lib, prec, 4), make(lib, prec, 4)
    for e_ in (a, b):
        step(e_)
        e_.push(all_, [1, 2, 3, 4], f, 0.3, frame="heading")
    assert same_bits(a.get_perturb_state(), b.get_perturb_state())
    a.push(all_, [1, 2, 3, 4], f, 0.3, frame="heading")
    rows = a.get_perturb_state()
    assert same_bits(rows[:, 3:9], rows[:, 9:15]) and (rows[:, 3] == [2, 3, 4, 5]).all()
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 4: the heading frame
def heading_of(q):
    """calc_heading of dm_math.h in float64: the heading of the root rotation (w, x, y, z)"""
    w, x, y, z = q
    u, v = np.array([x, y, z]), np.array([1.0, 0.0, 0.0])
    uv = 2.0 * np.cross(u, v)
    d = v + w * uv + np.cross(u, uv)
    return math.atan2(-d[2], d[0])


def heading_frame(lib, prec):
    """the stored force is rot_y(h) f within 64 eps(Real) |f|: a few ulps each for atan2, sincos and the products.
    Largest error seen, in units of eps(Real) |f|: emulator fp64 0.00 (numpy's own libm), fp32 0.80; MI355X fp64 1.88, fp32 1.16."""
    n = 4
    env = make(lib, prec, n)
    out = env.reset_where_at(np.ones(n, np.int32), times=[0.0, 0.3, 0.6, 0.9], yaw=[0.0, 0.7, -2.1, 3.0])
    assert out["bad"] == 0
    q = env.get_state()["pose"][:, 3:7]
    h = np.array([heading_of(q[e]) for e in range(n)])
    assert len({round(x, 3) for x in h}) == n                               # four different headings
    f = np.array([[120.0, 30.0, -45.0], [-80.0, 0.0, 15.0], [1.0, 2.0, 3.0], [0.0, -50.0, 250.0]])
    assert env.push(np.ones(n, np.int32), 2, f, 0.1, frame="heading") == 0
    got = env.get_perturb_state()[:, 4:7]
    c, s = np.cos(h), np.sin(h)
    want = np.stack([c * f[:, 0] + s * f[:, 2], f[:, 1], -s * f[:, 0] + c * f[:, 2]], axis=1)
    eps = np.finfo(np.float32 if prec == 32 else np.float64).eps
    err = np.abs(got - want).max(axis=1) / (eps * np.linalg.norm(f, axis=1))
    print("heading frame, precision %d: largest error %.2f eps |f|" % (prec, err.max()))
    assert (err < 64).all(), err
    # a heading of exactly 0 (the identity root rotation): the bytes of a world push
    twin = make(lib, prec, n)
    for e_ in (env, twin):
        st = e_.get_state(); P = st["pose"].copy(); P[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
        e_.set_state(pose=P, vel=st["vel"]); e_.clear_pushes()
    fr = np.array([[20.0, 5.0, -10.0], [-1.5, 0.25, 8.0], [100.0, -3.0, 0.5], [7.0, 7.0, 7.0]])       # (exact in float32)
    assert env.push(np.ones(n, np.int32), 3, fr, 0.2, frame="heading") == 0 and twin.push(np.ones(n, np.int32), 3, fr, 0.2, frame="world") == 0
    assert same_bits(env.get_perturb_state()[:, 3:15], twin.get_perturb_state()[:, 3:15])
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 5: lifetime
def lifetime_in_updates(lib, prec):
    """a push acts for ceil(duration / dt) whole updates, across control steps: counted as the updates that advance its elapsed time in push_state"""
    n = 4
    env = make(lib, prec, n)
    durs = np.array([0.0492, 0.0192, 0.0, np.inf])
    assert env.push(np.ones(n, np.int32), 1, [30.0, 0.0, 10.0], durs) == 0
    acted, last = np.zeros(n, int), env.push_state()[:, 0, 5].copy()
    assert (last == 0).all()
    for chunk in (20, 20, 5):                                               # two control steps and a part of the third, one update per call
        for _ in range(chunk):
            step(env, 1)
            ps = env.push_state()
            now = np.where(ps[:, 0, 0] >= 0, ps[:, 0, 5], last)
            acted += now > last
            last = now
    assert (acted == [math.ceil(0.0492 / DT), math.ceil(0.0192 / DT), 0, 45]).all() and math.ceil(0.0492 / DT) == 30, acted
    ps = env.push_state()
    assert (ps[:3, :, 0] == -1).all() and ps[3, 0, 0] == 1 and np.isinf(ps[3, 0, 4]) and abs(ps[3, 0, 5] - 45 * DT) < 1e-6
    env.close()


def resets_and_pool(lib, prec):
    """an auto-reset and reset_where clear the pushes as every scene reset does; a NEW_EPISODE restore brings the pushes of the slot; a REWIND repeats a pushed rollout"""
    n = 4
    env = make(lib, prec, n, limit=0.1)
    every = np.ones(n, np.int32)
    f = np.array([40.0, 0.0, -25.0])
    assert env.push(every, 0, f, np.inf) == 0
    ended = np.zeros(n, bool)
    for k in range(4):                                                      # (0.1 s: the episodes end at the first update of the fourth step)
        out = step(env, auto_reset=True)
        ended |= out["episode_end"] != 0
        assert (env.push_state()[~ended, 0, 0] == 0).all() and (env.push_state()[ended, :, 0] == -1).all(), k
    assert ended.all()
    assert env.push(every, 2, f, np.inf) == 0
    env.reset_where([1, 0, 1, 0])
    assert (env.push_state()[:, 0, 0] == [-1, 2, -1, 2]).all()
    # the pool: env 1's record, pushed, goes to slot 0; a new episode from it on env 0 brings the push, elapsed time included
    step(env)
    pool, bad = env.state_save(env.state_pool(2), [0, 1, 0, 0], np.zeros(n, np.int32))
    stored = env.push_state()[1].copy()
    assert bad == 0 and stored[0, 0] == 2 and stored[0, 5] > 0
    env.clear_pushes()
    assert env.state_restore(pool, [1, 0, 0, 0], np.zeros(n, np.int32), new_episode=True)["bad"] == 0
    ps = env.push_state()
    assert same_bits(ps[0], stored) and (ps[1:, :, 0] == -1).all()
    # rewind: the pushed rollout again, bit for bit
    env.set_time_limits(10.0, 10.0)
    env.reset()
    assert env.push(every, [1, 4, 7, 10], [f, -f, 2 * f, 0.5 * f], [0.0492, 0.3, np.inf, 0.02], frame="heading") == 0
    ids = np.arange(n, dtype=np.int32)
    pool, bad = env.state_save(env.state_pool(n), every, ids)
    first = [step(env) for _ in range(3)]
    end = env.snapshot()
    assert env.state_restore(pool, every, ids)["bad"] == 0
    for k in range(3):
        assert_same(step(env), first[k], ("rewound", k))
    assert_same(env.snapshot(), end, "rewound")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6: nothing fires by itself
def nothing_fires(lib, prec, packing):
    """a task_pushes context that is never pushed against enable_rand_perturbs with an interval of 1e9 s: the same bytes over five control steps with auto-resets"""
    t1 = model.load_asset("humanoid3d_walk"); c = t1.cfg
    c.enable_rand_perturbs = True; c.perturb_time_min = c.perturb_time_max = 1e9
    a = make(lib, prec, 4, packing=packing, limit=0.1)
    b = make(lib, prec, 4, packing=packing, limit=0.1, tables=t1)
    assert a.has_pushes and b.has_pushes
    resets = 0
    for k in range(5):
        ep0, d0 = a.get_state()["flags"][:, 2].copy(), a.get_perturb_state()[:, PT_DRAWS].copy()
        oa, ob = step(a, auto_reset=True), step(b, auto_reset=True)
        assert_same(oa, ob, k); assert_same(a.get_state(), b.get_state(), k)
        ra, rb = a.get_perturb_state(), b.get_perturb_state()
        assert np.isinf(ra[:, PT_NEXT]).all() and (rb[:, PT_NEXT] == 1e9).all()
        ra[:, PT_NEXT] = rb[:, PT_NEXT] = 0
        assert same_bits(ra, rb) and (ra[:, 3] == 0).all() and (ra[:, 9] == 0).all()
        began = a.get_state()["flags"][:, 2] - ep0
        assert (ra[:, PT_DRAWS] - d0 == began).all(), k                   # one draw per reset (ResetRandPertrub), none anywhere else
        resets += int(began.sum())
    assert resets >= 4
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 7: beside the random schedule, against the oracle
def mirror_push(o, link, f, dur):
    """what dm_push_where does to a row, done to the oracle's: a free slot, else the slot nearest its end"""
    row = o.perturb_state()
    keys = [1e300 if row[3 + 6 * i] == 0 else row[8 + 6 * i] - row[7 + 6 * i] for i in range(2)]
    i = 0 if keys[0] >= keys[1] else 1
    row[3 + 6 * i: 9 + 6 * i] = [link + 1, f[0], f[1], f[2], dur, 0.0]
    o.set_perturb_state(row)


def with_the_random_schedule(lib, prec, packing, steps=24, n=4, seed=21):
    """tests/test_perturbs.py::rollout_with_perturbs with a task push every third step, mirrored into each oracle at the same moment"""
    t = perturbed(model.load_asset("humanoid3d_walk"))
    env = BatchEnv(t, n, precision=prec, lib_path=lib, wave_packing=packing, seed=seed)
    d0 = env.get_perturb_state()[:, 2]
    env.reset()
    ep = env.get_state()["flags"][:, 2].astype(np.int64)
    oracles = []
    for e in range(n):
        o = Oracle(t); o.goal_rng(seed, e); o.set_perturb_state(slot_row(draws=d0[e]))
        o.reset(o.duration * streams.reset_rand01(seed, e, int(ep[e]) - 1, 0), np.inf)
        oracles.append(o)
    rng = np.random.default_rng(5)
    dr, ds = np.zeros((steps, n)), np.zeros((steps, n))
    hits, both, resets, pushed, rows_ok = 0, 0, 0, 0, True
    for k in range(steps):
        if k % 3 == 0:
            links, f, dur = rng.integers(0, env.J, n).astype(np.int32), rng.normal(size=(n, 3)) * 60.0, rng.uniform(0.01, 0.03, n)
            assert env.push(np.ones(n, np.int32), links, f, dur) == 0
            for e, o in enumerate(oracles):
                mirror_push(o, int(links[e]), f[e], dur[e])
            rows = env.get_perturb_state()
            for e, o in enumerate(oracles):
                rows_ok &= active(rows[e]) == active(o.perturb_state())
            pushed += n
        out = env.step(None, DT, 20, open_loop=True, auto_reset=True)
        rows = env.get_perturb_state()
        for e, o in enumerate(oracles):
            kp, _, _ = o.kin_state()
            o.set_action(o.pose_to_action(kp))
            o.control_step(20, DT)
            dr[k, e] = abs(float(out["reward"][e]) - o.calc_reward())
            # (the reference's manager is a list without a bound, the device has two slots: the task's pushes are short -- 6 to 18 updates -- so that a drawn
            # force does not meet two others in this rollout)
            assert o.num_perturbs() <= 2, (k, e)
            assert bool(out["episode_end"][e]) == o.is_episode_end() and int(out["terminate"][e]) == o.check_terminate(), (k, e)
            if o.is_episode_end():
                o.reset(o.duration * streams.reset_rand01(seed, e, int(ep[e]), 0), np.inf)
                ep[e] += 1; resets += 1
            so = o.record_state()
            ds[k, e] = np.abs(out["state"][e] - so).max() / max(1.0, np.abs(so).max())
            ro = o.perturb_state()
            rows_ok &= bool(np.abs(rows[e][:3] - ro[:3]).max() < 1e-9) and active(rows[e]) == active(ro)
            hits += len(active(ro)) > 0; both += len(active(ro)) == 2
    env.close()
    return dr, ds, rows_ok, hits, both, resets, pushed


# ---------------------------------------------------------------------------------------------------------------- 8: invalid and refused
def invalid_kinds(J):
    """(name, {argument: value of the bad env})"""
    return [("link J", dict(links=J)), ("link -2", dict(links=-2)), ("force nan", dict(forces=[1.0, np.nan, 0.0])), ("force inf", dict(forces=[np.inf, 0.0, 0.0])),
            ("force -inf", dict(forces=[0.0, 0.0, -np.inf])), ("duration < 0", dict(durations=-0.01)), ("duration nan", dict(durations=np.nan)),
            ("slot 2", dict(slots=2)), ("slot -2", dict(slots=-2))]


def invalid_input(lib, prec):
    n = 4
    env = make(lib, prec, n)
    assert env.push(np.ones(n, np.int32), 1, [5.0, 6.0, 7.0], 0.4) == 0     # something to keep
    for name, bad in invalid_kinds(env.J):
        for mask in ([0, 0, 1, 0], [1, 1, 1, 1]):                           # alone, and mixed with valid envs
            args = dict(links=np.full(n, 3, np.int32), forces=np.tile([9.0, 8.0, 7.0], (n, 1)), durations=np.full(n, 0.25), slots=np.full(n, -1, np.int32))
            key, val = next(iter(bad.items()))
            args[key][2] = val
            before = env.get_perturb_state()
            assert env.push(mask, args["links"], args["forces"], args["durations"], args["slots"]) == 1, name
            after = env.get_perturb_state()
            assert same_bits(after[2], before[2]), name                     # the invalid env keeps every byte
            for e in (0, 1, 3):
                if mask[e]:
                    assert after[e, 9] == 4.0 and same_bits(after[e, 10:15], np.array([9.0, 8.0, 7.0, 0.25, 0.0])) and same_bits(after[e, :9], before[e, :9]), (name, e)
                else:
                    assert same_bits(after[e], before[e]), (name, e)
            assert env.push(np.ones(n, np.int32), -1, 0.0, 0.0, slots=1) == 0       # slot 1 free again
    # a clearing row is held to the same rules; an unselected env may hold anything
    assert env.push([0, 0, 1, 0], -1, [np.nan, 0.0, 0.0], 0.0) == 1 and env.push([1, 1, 0, 1], [1, 1, 99, 1], [[1.0, 0, 0], [1.0, 0, 0], [np.nan] * 3, [1.0, 0, 0]], 0.1) == 0
    env.close()


def refusals(lib, prec):
    env = make(lib, prec, 2)
    N = env.N
    mask, links, forces, durs = np.ones(N, np.int32), np.zeros(N, np.int32), np.zeros((N, 3)), np.zeros(N)
    ptr, fetch = env._dev_arrays({"mask": ((N,), np.int32), "links": ((N,), np.int32), "forces": ((N, 3), np.float64), "durs": ((N,), np.float64), "out": ((N, 2, 6), np.float32)},
                                 {"mask": mask, "links": links, "forces": forces, "durs": durs})
    good = [ptr["mask"], ptr["links"], ptr["forces"], ptr["durs"]]
    before = env.get_perturb_state()
    for i, what in enumerate(("mask_dev", "links_dev", "forces_dev", "durations_dev")):
        args = list(good); args[i] = 0
        with pytest.raises(RuntimeError, match="dm_push_where: null " + what):
            pushes.push_where_device(env, *args)
    with pytest.raises(RuntimeError, match="dm_push_where: unknown flag bits"):
        pushes.push_where_device(env, *good, flags=2)
    with pytest.raises(RuntimeError, match="dm_push_state: null out_dev"):
        pushes.push_state_device(env, 0)
    assert env.lib.dm_push_where(None, *[C.c_void_p(p) for p in good], None, 0, None) != 0 and b"dm_push_where: null ctx" in env.lib.dm_last_error()
    assert env.lib.dm_push_state(None, C.c_void_p(ptr["out"])) != 0 and b"dm_push_state: null ctx" in env.lib.dm_last_error()
    with pytest.raises(ValueError, match="frame"):
        env.push(mask, links, forces, durs, frame="body")
    assert same_bits(env.get_perturb_state(), before)
    plain = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=prec, lib_path=lib, seed=SEED)
    assert not plain.has_pushes
    with pytest.raises(RuntimeError, match="dm_push_where: the context has no perturbation rows"):
        plain.push(mask, links, forces, durs)
    with pytest.raises(RuntimeError, match="dm_push_state: the context has no perturbation rows"):
        plain.push_state()
    env.close(); plain.close()
