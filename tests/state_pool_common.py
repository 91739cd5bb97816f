"""The checks of tests/test_state_pool.py (CPU emulator) and tests/test_state_pool_gpu.py (device) for the device state pool (include/dm_hip.h dm_state_save /
dm_state_restore, deepmimic_amd/state_pool.py), through BatchEnv.state_pool / state_save / state_restore.  Everything is compared byte for byte: a pool moves
records, it computes nothing; the rows a restore emits are the rows of a zero-update launch.  Open-loop steps, and a time limit of 10 s so that no episode ends
inside the compared steps (check 5 pins 0.1 s where it wants resets).  The pool is data with a documented layout (state_pool.dims), so the checks read the columns
the host interface does not expose -- the draw keys, the draw counters, the pose history -- out of a saved record."""
import math

import numpy as np

from deepmimic_amd import model
from deepmimic_amd import state_pool as sp
from deepmimic_amd.core import BatchEnv
from reset_where_common import CASES, SENTINEL
from test_episode_reset import DT, SEED, assert_same, extras, same_bits

M = 5
GS_DRAWS, GS_CLIP, GS_KSEED, GS_KON, GS_WIDTH = 11, 12, 20, 21, 24       # dm_types.h
PT_DRAWS, PT_KSEED, PT_WIDTH = 2, 15, 16
# (case, physics) of checks 1 and 2
SCENES = [(c, 1) for c in CASES] + [("plain", 2)]


def make(case, lib, prec, n, physics=1, packing=0, limit=10.0):
    tables, amp = CASES[case]
    env = BatchEnv(tables(), n, precision=prec, lib_path=lib, seed=SEED, physics=physics, wave_packing=packing)
    env.set_time_limits(limit, limit)
    env.reset()
    return env, amp


def step(env, amp, n=20):
    return env.step(None, DT, n, auto_reset=False, open_loop=True, amp=amp)


def everything(env, amp):
    """the host's view of a context: snapshot(), the rows beside it, the last goals and the AMP observation of the stored history"""
    x = {"snap." + k: v for k, v in env.snapshot().items()}
    x.update({"extra." + k: v for k, v in extras(env).items()})
    if env.G:
        x["last_goals"] = env.last_goals()
    if amp:
        x["query_amp"] = env.query_amp()
    return x


def record(env, pool, slot, seg, dtype):
    """segment `seg` of a slot as an array of `dtype`"""
    d = sp.dims(env)
    offs = sorted(d["offsets"].values()) + [d["slot_bytes"]]
    o = d["offsets"][seg]
    return np.frombuffer(pool[slot, o:offs[offs.index(o) + 1]].tobytes(), dtype)


def own_record(env, e, seg, dtype):
    """segment `seg` of env e's current record (saved into a scratch pool)"""
    pool, bad = env.state_save(env.state_pool(1), np.arange(env.N) == e, np.zeros(env.N, np.int32))
    assert bad == 0
    return record(env, pool, 0, seg, dtype)


def steps_for(case, env):
    """three steps; in the perturbed scene as many as hold a perturbation draw for certain"""
    if case != "amp_perturbed":
        return 3
    return max(3, int(math.ceil(env.tables.cfg.perturb_time_max / (20 * DT))) + 1)


def rewind(case, lib, prec, n, physics=1, packing=0):
    """check 1: returns every byte it compared, for check 8"""
    a, amp = make(case, lib, prec, n, physics, packing)
    b, _ = make(case, lib, prec, n, physics, packing)
    ns = steps_for(case, a)
    for env in (a, b):
        for _ in range(2):
            step(env, amp)
    every, ids = np.ones(n, np.int32), np.arange(n, dtype=np.int32)
    pool, bad = a.state_save(a.state_pool(M), every, ids)
    assert bad == 0
    at_save, snap_b = everything(a, amp), b.snapshot()
    if a.has_perturbs:
        draws0 = a.get_perturb_state()[:, PT_DRAWS].copy()
    first = [step(a, amp) for _ in range(ns)]
    for _ in range(ns):
        step(b, amp)
    if a.has_perturbs and case == "amp_perturbed":
        assert (a.get_perturb_state()[:, PT_DRAWS] > draws0).all()      # a perturbation was drawn inside the compared steps
    assert not same_bits(a.snapshot()["pose"], at_save["snap.pose"])
    out = a.state_restore(pool, every, ids)
    assert out["bad"] == 0
    assert_same(everything(a, amp), at_save, "rewound")
    b.restore(snap_b)
    for k in range(ns):
        oa, ob = step(a, amp), step(b, amp)
        assert_same(oa, first[k], ("again", k))
        assert_same(ob, first[k], ("host route", k))
    a.close(); b.close()
    return [pool.tobytes()] + [v.tobytes() for o in first for v in o.values()] + [np.ascontiguousarray(v).tobytes() for v in at_save.values()]


def emitted_rows(case, lib, prec, n, physics=1):
    """check 2"""
    a, amp = make(case, lib, prec, n, physics)
    for _ in range(2):
        step(a, amp)
    ids = np.arange(n, dtype=np.int32)
    pool, _ = a.state_save(a.state_pool(M), np.ones(n, np.int32), ids)
    step(a, amp)
    mask = (np.arange(n) % 2 == 1).astype(np.int32)
    sent_s = np.full((n, a.S), SENTINEL, np.float32)
    sent_g = np.full((n, a.G), SENTINEL, np.float32) if a.G else None
    both = a.state_restore(pool, mask, ids, states=sent_s, goals=sent_g)
    only_s = a.state_restore(pool, mask, ids, states=sent_s, want_goals=False)
    assert "goal" not in only_s and same_bits(only_s["state"], both["state"])
    if a.G:
        own = a.last_goals()
        only_g = a.state_restore(pool, mask, ids, goals=sent_g, want_states=False)
        assert "state" not in only_g and same_bits(only_g["goal"], both["goal"]) and same_bits(a.last_goals(), own)
    none = a.state_restore(pool, mask, ids, want_states=False, want_goals=False)
    assert sorted(none) == ["bad"]
    before = a.snapshot()
    ref = a.step(None, DT, 0, auto_reset=False, open_loop=False, amp=False)      # the zero-update launch
    sel = mask != 0
    assert same_bits(both["state"][sel], ref["state"][sel]) and (both["state"][~sel] == SENTINEL).all()
    if a.G:
        assert same_bits(both["goal"][sel], ref["goal"][sel]) and (both["goal"][~sel] == SENTINEL).all()
    assert_same(a.snapshot(), before, "zero-update launch")
    a.close()


def across_envs(lib, prec, n, packing=0):
    """check 3, the plain scene: slot 2 holds env 0; envs 1 and 3 (N = 3: env 1) take it"""
    a, amp = make("plain", lib, prec, n, packing=packing)
    for _ in range(2):
        step(a, amp)
    pool, _ = a.state_save(a.state_pool(M), np.arange(n) == 0, np.full(n, 2, np.int32))
    assert not pool[[0, 1, 3, 4]].any() and pool[2].any()             # one slot written
    before = a.snapshot()
    mask = (np.arange(n) % 2 == 1).astype(np.int32)
    a.state_restore(pool, mask, np.full(n, 2, np.int32))
    after = a.snapshot()
    took, kept = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
    for key in before:
        assert same_bits(after[key][kept], before[key][kept]), key
        for e in took:
            assert same_bits(after[key][e], before[key][0]), (key, e)
    real = np.float32 if prec == 32 else np.float64
    for seg, width in (("tau", None), ("kin", 7), ("flag", 4)):                 # what snapshot() leaves out; column 7 of kin is the env's own counter
        r0 = own_record(a, 0, seg, np.int32 if seg == "flag" else real)
        for e in took:
            assert same_bits(own_record(a, e, seg, np.int32 if seg == "flag" else real)[:width], r0[:width]), (seg, e)
    act = np.zeros((n, a.A), np.float32) + np.linspace(-0.2, 0.2, a.A, dtype=np.float32)     # equal action rows
    out = a.step(act, DT, 20, auto_reset=False, open_loop=False)
    for e in took:
        assert same_bits(out["state"][e], out["state"][0]) and same_bits(out["reward"][e], out["reward"][0]), e
    if len(kept) > 1:
        assert not same_bits(out["state"][kept[1]], out["state"][0])
    a.close()


def own_keys(lib, prec):
    """check 3, the per-env items: after dm_set_env_keys on env 1 a restore of env 0's record leaves env 1's draw keys its own (goal row and perturbation row)"""
    for case, seg, cols in (("amp_heading_clips4", "goal", (GS_KSEED, GS_KON)), ("amp_perturbed", "pert", (PT_KSEED,))):
        a, amp = make(case, lib, prec, 4)
        a.set_env_keys([1], [4242])
        a.reset()
        for _ in range(2):
            step(a, amp)
        mine, other = own_record(a, 1, seg, np.float64), own_record(a, 0, seg, np.float64)
        assert all(mine[c] != other[c] for c in cols)
        pool, _ = a.state_save(a.state_pool(M), np.arange(4) == 0, np.full(4, 2, np.int32))
        a.state_restore(pool, np.array([0, 1, 0, 1], np.int32), np.full(4, 2, np.int32))
        now = own_record(a, 1, seg, np.float64)
        keep = np.zeros(now.size, bool); keep[list(cols)] = True
        assert same_bits(now[keep], mine[keep]) and same_bits(now[~keep], other[~keep]), case
        assert same_bits(own_record(a, 3, seg, np.float64), other), case      # env 3 has the context's key, as env 0
        a.close()


def pool_is_data(lib, prec):
    """check 4 on the host arrays (the torch pool: tests/test_vec_env_state_pool.py): a copy of the pool, a second context of the scene, another scene's pool"""
    a, amp = make("amp_heading_clips4", lib, prec, 4)
    b, _ = make("amp_heading_clips4", lib, prec, 4)
    for _ in range(2):
        step(a, amp)
    every, ids = np.ones(4, np.int32), np.arange(4, dtype=np.int32)
    pool, _ = a.state_save(a.state_pool(M), every, ids)
    want = everything(a, amp)
    step(a, amp)
    a.state_restore(np.frombuffer(pool.tobytes(), np.uint8).reshape(pool.shape).copy(), every, ids)
    assert_same(everything(a, amp), want, "a copy of the pool")
    b.state_restore(pool, every, ids)
    assert_same(everything(b, amp), want, "a second context")
    first = step(a, amp)
    assert_same(step(b, amp), first, "a second context, one step on")
    c, _ = make("plain", lib, prec, 4)
    import pytest
    assert c.state_pool(M).shape != pool.shape
    with pytest.raises(ValueError, match="a pool of this scene and precision"):
        c.state_restore(pool, every, ids)
    with pytest.raises(ValueError, match="a pool of this scene and precision"):
        c.state_save(pool, every, ids)
    a.close(); b.close(); c.close()


def new_episode(case, lib, prec):
    """check 5 on one case: slot 2 holds env 0 after two steps; env 1 starts a new episode there"""
    a, amp = make(case, lib, prec, 4)
    b, _ = make(case, lib, prec, 4)
    real = np.float32 if prec == 32 else np.float64
    for env in (a, b):
        for _ in range(2):
            step(env, amp)
    slots = np.full(4, 2, np.int32)
    pool, _ = a.state_save(a.state_pool(M), np.arange(4) == 0, slots)
    for env in (a, b):
        step(env, amp)
        env.set_time_limits(5.0, 10.0)                                         # the limit of the new episode is a draw
    before, xb = a.snapshot(), extras(a)
    draws_before = {seg: own_record(a, 1, seg, np.float64)[col] for seg, col in (("goal", GS_DRAWS), ("pert", PT_DRAWS)) if seg in sp.dims(a)["offsets"]}
    mask = np.array([0, 1, 0, 0], np.int32)
    out = a.state_restore(pool, mask, slots, new_episode=True)
    assert out["bad"] == 0
    after, xa = a.snapshot(), extras(a)
    for key in ("pose", "vel", "tar", "kin"):
        assert same_bits(after[key][1], record(a, pool, 2, key, real)[:after[key].shape[1]].astype(np.float64)), key
    clk = record(a, pool, 2, "clock", np.float64)
    assert same_bits(after["clocks"][1, :3], clk[:3])                          # kin clock, control clock, its offset: the slot's
    assert after["clocks"][1, 3] == 0.0                                        # timer_time
    slot_flags = record(a, pool, 2, "flag", np.int32)
    assert after["flags"][1, 0] == slot_flags[0] and after["flags"][1, 1] == 0 and after["flags"][1, 3] == 1
    assert after["flags"][1, 2] == before["flags"][1, 2] + 1
    b.reset_where(mask)                                                        # the twin: the same env reset at the same episode counter
    assert b.get_state()["flags"][1, 2] == after["flags"][1, 2]
    assert same_bits(after["clocks"][1, 4], b.get_state()["clocks"][1, 4])     # timer_max: the draw of stream 1 at that counter
    assert 5.0 < after["clocks"][1, 4] < 10.0 and after["clocks"][1, 4] != clk[4]
    if "goal" in xa:
        g = record(a, pool, 2, "goal", np.float64)
        assert same_bits(xa["goal"][1, :GS_DRAWS], g[:GS_DRAWS]) and xa["clips"][1] == int(g[GS_CLIP])      # target, timers, clip: the slot's
    if "obj" in after:
        assert same_bits(after["obj"][1], record(a, pool, 2, "obj", real)[:after["obj"].shape[1]].astype(np.float64))
    for seg, col in (("goal", GS_DRAWS), ("pert", PT_DRAWS)):
        if seg in draws_before:
            assert own_record(a, 1, seg, np.float64)[col] == draws_before[seg], seg      # the destination's own draw counters
    for key in before:                                                         # the other envs keep every byte
        assert same_bits(after[key][[0, 2, 3]], before[key][[0, 2, 3]]), key
    if amp:
        # the history is re-initialised: the kinematic character one control period before the restored control clock, not the slot's rows
        P = after["pose"].shape[1]
        hist = own_record(a, 1, "hist", real)
        assert not same_bits(hist, record(a, pool, 2, "hist", real))
        period = 1.0 / a.tables.query_rate
        kq = a.kin_query(np.array([clk[1] - period]), absolute=True)
        assert same_bits(hist[:P].astype(np.float32), kq["pose"][1, 0]) and same_bits(hist[P:2 * P].astype(np.float32), kq["vel"][1, 0])
    a.close(); b.close()


def fresh_draws(lib, prec):
    """check 5, the draws behind the start: the same slot into the same env twice, eight auto-reset steps at a 0.1 s limit after each"""
    runs = {}
    for mode in (True, False):
        a, amp = make("plain", lib, prec, 4, limit=0.1)
        for _ in range(2):
            step(a, amp)                                                       # 0.067 s: the record's episode ends in the next step
        ids = np.arange(4, dtype=np.int32)
        pool, _ = a.state_save(a.state_pool(M), np.ones(4, np.int32), ids)
        mask = np.array([0, 1, 0, 0], np.int32)
        rolls = []
        for _ in range(2):
            a.state_restore(pool, mask, ids, new_episode=mode)
            rolls.append([a.step(None, DT, 20, auto_reset=True, open_loop=True)["state"][1].copy() for _ in range(8)])
        runs[mode] = rolls
        a.close()
    assert not same_bits(np.stack(runs[True][0]), np.stack(runs[True][1]))       # NEW_EPISODE: the episode counter moved on, the resets draw anew
    assert same_bits(np.stack(runs[False][0]), np.stack(runs[False][1]))         # REWIND: the counter is the record's, the same draws again


def masks(case, lib, prec):
    """check 6"""
    a, amp = make(case, lib, prec, 4)
    b, _ = make(case, lib, prec, 4)
    for env in (a, b):
        for _ in range(2):
            step(env, amp)
    ids = np.arange(4, dtype=np.int32)
    pool, _ = a.state_save(a.state_pool(M), np.ones(4, np.int32), ids)
    empty, bad = a.state_save(a.state_pool(M), np.zeros(4, np.int32), ids)
    assert not empty.any() and bad == 0
    for env in (a, b):
        step(env, amp)
    want = everything(a, amp)
    sent = np.full((4, a.S), SENTINEL, np.float32)
    out = a.state_restore(pool, np.zeros(4, np.int32), ids, states=sent)
    assert same_bits(out["state"], sent)
    assert_same(everything(a, amp), want, "zero mask")
    m1 = np.array([1, 0, 1, 0], np.int32)
    oa, ob = a.state_restore(pool, m1, ids, states=sent), b.state_restore(pool, 7 * m1, ids, states=sent)
    assert_same(oa, ob, "mask 7")
    assert_same(everything(a, amp), everything(b, amp), "mask 7")
    p7, _ = b.state_save(b.state_pool(M), 7 * m1, ids)
    p1, _ = a.state_save(a.state_pool(M), m1, ids)
    assert same_bits(p1, p7) and p1[[0, 2]].any() and not p1[[1, 3, 4]].any()
    a.close(); b.close()


def invalid_slots(lib, prec):
    """check 7, CPU emulator only: an env with a slot of -1 or M is untouched, bad is 1, the valid envs of the same call are served"""
    a, amp = make("amp_heading_clips4", lib, prec, 4)
    for _ in range(2):
        step(a, amp)
    good = np.arange(4, dtype=np.int32)
    pool, bad = a.state_save(a.state_pool(M), np.ones(4, np.int32), good)
    assert bad == 0
    for wrong in (-1, M, 2 ** 30, -2 ** 31):
        slots = np.array([wrong, 1, 2, 3], np.int32)
        p2, bad = a.state_save(a.state_pool(M), np.array([1, 1, 0, 1], np.int32), slots)
        assert bad == 1 and p2[1].any() and p2[3].any() and not p2[[0, 2, 4]].any(), wrong
        step(a, amp)
        before = everything(a, amp)
        sent = np.full((4, a.S), SENTINEL, np.float32)
        out = a.state_restore(pool, np.array([1, 1, 0, 1], np.int32), slots, states=sent)
        assert out["bad"] == 1, wrong
        after = everything(a, amp)
        for key in before:
            assert same_bits(after[key][[0, 2]], before[key][[0, 2]]), (wrong, key)
            if key in ("snap.pose", "snap.clocks"):
                assert not same_bits(after[key][1], before[key][1]) and not same_bits(after[key][3], before[key][3]), (wrong, key)
        assert (out["state"][[0, 2]] == SENTINEL).all() and not (out["state"][[1, 3]] == SENTINEL).any(), wrong
    a.close()


def refusals(lib, prec):
    """the host's refusals by name, before any launch"""
    import pytest
    env = BatchEnv(model.load_asset("humanoid3d_walk"), 2, precision=prec, lib_path=lib)
    env.reset()
    buf = np.zeros(sp.pool_bytes(env, 2) // 4 + 64, np.float32)         # never written: every call below is refused before a launch
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    for name, call in (("dm_state_save", lambda p, n, m, s: sp.save_device(env, p, n, m, s)), ("dm_state_restore", lambda p, n, m, s: sp.restore_device(env, p, n, m, s))):
        for what, args in (("null pool_dev", (0, 2, a, a)), ("null mask_dev", (a, 2, 0, a)), ("null slots_dev", (a, 2, a, 0)), ("slots must be positive", (a, 0, a, a)),
                           ("slots must be positive", (a, -3, a, a)), ("the pool must be 16-byte aligned", (a + 4, 2, a, a))):
            with pytest.raises(RuntimeError, match=name + ": " + what):
                call(*args)
    with pytest.raises(RuntimeError, match="dm_state_restore: unknown flag bits"):
        sp.restore_device(env, a, 2, a, a, flags=2)
    with pytest.raises(RuntimeError, match="dm_state_restore: goals_dev on a scene without a goal"):
        sp.restore_device(env, a, 2, a, a, goals_ptr=a)
    with pytest.raises(RuntimeError, match="dm_state_pool_bytes: slots must be positive"):
        sp.pool_bytes(env, 0)
    from deepmimic_amd.core import TAPE_STRIDE
    env.set_draw_tape(np.zeros((env.N, TAPE_STRIDE)))
    with pytest.raises(RuntimeError, match="dm_state_save: a draw tape is bound"):
        sp.save_device(env, a, 2, a, a)
    with pytest.raises(RuntimeError, match="dm_state_restore: a draw tape is bound"):
        sp.restore_device(env, a, 2, a, a)
    env.set_draw_tape(None)
    assert env.lib.dm_state_save(None, a, 2, a, a, None) != 0 and env.lib.dm_state_restore(None, a, 2, a, a, 0, None, None, None) != 0
    assert (buf == 0).all()
    d = sp.dims(env)
    assert d["slot_bytes"] % 16 == 0 and all(o % 16 == 0 for o in d["offsets"].values()) and sp.pool_bytes(env, 3) == 3 * d["slot_bytes"]
    assert sorted(d["offsets"]) == sorted(["pose", "vel", "tar", "tau", "kin", "clock", "flag"])
    env.close()
