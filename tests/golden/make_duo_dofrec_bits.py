"""Records the fixtures of tests/test_duo_dofrec_bits.py from a build of the CURRENT checkout:

    make -C tests/emu && python tests/golden/make_duo_dofrec_bits.py                              ->  tests/golden/duo_dofrec_bits.npz (emulator, fp32 and fp64)
    python tests/golden/make_duo_dofrec_bits.py device <libdm_hip.so> <out.npz>                   ->  the device fixture (fp32, on the GPU)

Run it on the commit whose arithmetic is to be pinned (the parent of a change that must keep results bit for bit), never on
the change itself.  The rollouts aim at every reader and writer of the per-dof records of the LDS record (Lds::dofrec: axis, moment
arm, v*, bias force): the limit rows, the 32-row path of the two-per-wave kernel, its borrowed-lane routine, its 64-lane fallback,
the mass matrix rows built from them (EnvSim::dyn_row) on their way into DuoSim::chol_solve, and the records rebuilt after a character of a pair has been parked.  The recorder watches every control step through a second
env object and refuses to write a fixture whose two-per-wave rollouts miss one of the situations listed in `SITUATIONS`."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["DM_ALLOW_EMULATOR"] = "1"

N, STEPS, SEED, TIME_LIM, SIGMA = 8, 6, 31, 0.1, 0.15
# Start states (the halves of a pair are envs 2k, 2k + 1):
#   pair 0  env 0 lying on its side beside a standing partner    -> more than 32 rows in one half, at most 64 together: borrowed lanes
#   pair 1  both standing, pressed into the ground               -> the 32-row path with contacts on both characters
#   pair 2  both lying                                           -> more than 64 rows together: the 64-lane fallback
#   pair 3  knees and elbows bent past their limits              -> active limit rows on dofs of either slot of a record pair (even and odd dofs)
DEPTHS = (0.0, 0.05, 0.02, 0.03, 0.0, 0.0, 0.01, 0.04)
LYING = {0: (0.16, 3), 4: (0.16, 3), 5: (0.16, 3)}      # env -> height of its root above the ground (m), axis of the quarter turn that lays it down (1: x, 3: z)
PAST_LIMIT = 0.08      # rad beyond the bound; env 6: every limit joint past its upper bound, env 7: past its lower bound
# episode timers of the first episodes (s): the halves of a pair end in different updates of a control step (20 updates of 1 / 600 s), so
# the one that ends first is parked while its partner goes on; later episodes run TIME_LIM
TIMER_MAX = (0.045, 0.1, 0.1, 0.055, 0.1, 0.075, 0.06, 0.1)
# case -> (asset, DM-physics version, wave packing, the kernel family that must have run, environment of the library)
CASES = {
    "walk": ("humanoid3d_walk", 1, 2, 0, {}),             # plain two-per-wave instantiation
    "amp": ("amp_heading_zombie", 1, 2, 1, {}),           # AMP / goal instantiation
    "v2": ("humanoid3d_walk", 2, 2, 22, {}),              # DM-physics v2, two per wave
    "dribble": ("amp_dribble_zombie", 1, 2, 24, {}),      # biped + free body, two per wave
    "tree": ("humanoid3d_walk", 1, 1, 15, {"DM_TREE_BIPED": "1"}),      # one per wave (compiled topology)
}
EMU_CASES, DEVICE_CASES = ("walk", "amp", "v2", "dribble", "tree"), ("walk", "amp")
DUO_V1 = ("walk", "amp")       # the cases whose coverage is demanded (v1 rows: one row per limit joint)
OUT_KEYS = ("state", "reward", "terminate", "valid", "episode_end")
SITUATIONS = ("an active limit row on a dof in slot 0 of its record pair (even dof)", "an active limit row on a dof in slot 1 of its record pair (odd dof)",
              "a pair on the 32-row path with contacts on both characters", "a pair on the borrowed-lane path", "a pair on the 64-lane fallback",
              "a character parked mid-step beside a partner that goes on")


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def limit_joints(t):
    """the limit rows of a character in row order: (pose offset, first dof, lower bound, upper bound) of every revolute joint with lo <= hi"""
    from deepmimic_amd import model as M
    jm, out, dof = t.joint_mat, [], 0
    for j in range(jm.shape[0]):
        jt = int(jm[j, M.JD_TYPE])
        nd = 6 if j == 0 else {M.JT_REVOLUTE: 1, M.JT_PRISMATIC: 1, M.JT_PLANAR: 3, M.JT_FIXED: 0, M.JT_SPHERICAL: 3}[jt]
        if j > 0 and jt == M.JT_REVOLUTE and jm[j, M.JD_LL0] <= jm[j, M.JD_LH0]:
            out.append((int(jm[j, M.JD_PARAM_OFFSET]), dof, float(jm[j, M.JD_LL0]), float(jm[j, M.JD_LH0])))
        dof += nd
    return out


def rollout(case, precision, lib_path, seen=None, rows_out=None):
    """Seeded random actions through auto-resets.  Returns every output of the control steps and the whole snapshot behind each.
    With `seen` (a dict over SITUATIONS) a second env object is set to the snapshot in front of every control step and asked (a) for the
    constraint rows and the row impulses of the update that follows it (tap probe), (b) whether one character of a pair has ended its
    episode 19 updates into the step while its partner has not; the recorded env's own counters say which pairs left the 32-row path.  The
    recorded env is never touched by that."""
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    asset, physics, packing, family, environ = CASES[case]
    old = {k: os.environ.get(k) for k in environ}
    os.environ.update(environ)
    try:
        t = model.load_asset(asset)
        t.cfg.time_lim_min = t.cfg.time_lim_max = TIME_LIM
        t.cfg.enable_fall_end = False          # (a lying character stays in its episode: the heavy pairs last, and episodes end by their timers)
        lims = limit_joints(t)
        mk = lambda: BatchEnv(t, N, precision=precision, lib_path=lib_path, wave_packing=packing, physics=physics, seed=SEED)
        env = mk()
        spy = mk() if seen is not None else None
        env.reset()
        st = env.get_state()
        st["pose"][:, 1] -= np.asarray(DEPTHS)
        for e, (height, axis) in LYING.items():       # a quarter turn, the root just above the ground
            turn = np.zeros(4); turn[0] = turn[axis] = np.sqrt(0.5)
            st["pose"][e, 3:7] = _qmul(turn, st["pose"][e, 3:7])
            st["pose"][e, 1] = height
        for off, _, lo, hi in lims:
            st["pose"][6, off] = hi + PAST_LIMIT
            st["pose"][7, off] = lo - PAST_LIMIT
        st["clocks"][:, 4] = np.asarray(TIMER_MAX)
        env.set_state(pose=st["pose"], vel=st["vel"], tar=st["tar"], kin=st["kin"], clocks=st["clocks"], flags=st["flags"])
        rng = np.random.default_rng(SEED + 100)
        rec = {}
        if spy is not None:
            spy.reset()
        borrowed, fallback = np.zeros(N), np.zeros(N)
        for _ in range(STEPS):
            acts = (SIGMA * rng.normal(size=(N, env.A))).astype(np.float32)
            if spy is not None:
                before = env.snapshot()
                spy.restore(before)
                spy.probe(1, 1.0 / 600)
                rows, lam = spy.debug("rows").astype(np.int64), spy.debug("lambda")
                R, nc = rows[:, 0], rows[:, 1]
                if rows_out is not None:
                    rows_out.append([int(x) for x in R])
                for e in range(N):
                    if physics == 1 and 0 < R[e]:
                        for r, (_, dof, _, _) in enumerate(lims):
                            if lam[e, r] != 0:
                                seen[SITUATIONS[dof & 1]] = True
                for a in range(0, N, 2):
                    if packing == 2 and 0 < R[a] <= 32 and 0 < R[a + 1] <= 32 and nc[a] > 0 and nc[a + 1] > 0:
                        seen[SITUATIONS[2]] = True
                spy.restore(before)
                o19 = spy.step(acts, 1.0 / 600, 19, auto_reset=False, end_early=True)["episode_end"].astype(bool)
                for a in range(0, N, 2):
                    if packing == 2 and o19[a] != o19[a + 1]:
                        seen[SITUATIONS[5]] = True
            out = env.step(acts, 1.0 / 600, 20, auto_reset=True)
            fam = env.debug("family")
            assert (fam == family).all(), (case, fam)
            if seen is not None and packing == 2:
                b, f = env.debug("borrowed"), env.debug("fallback")
                seen[SITUATIONS[3]] |= bool((b > borrowed).any())
                seen[SITUATIONS[4]] |= bool((f > fallback).any())
                borrowed, fallback = np.maximum(b, borrowed), np.maximum(f, fallback)
            snap = env.snapshot()
            for k in OUT_KEYS:
                rec.setdefault(k, []).append(out[k].copy())
            for k, v in snap.items():
                rec.setdefault("snap_" + k, []).append(np.array(v, copy=True))
        env.close()
        if spy is not None:
            spy.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {k: np.stack(v) for k, v in rec.items()}


DIGEST = "__blake2b"


def pack(k, v):
    """the wide arrays (observation, pose, velocity, PD target: more than 16 values per control step and env) are stored as one 16-byte
    BLAKE2b digest of the bytes of each (control step, env) row, which keeps the fixture small and still says where a rollout departs"""
    if v.ndim == 3 and v.shape[2] > 16:
        rows = np.ascontiguousarray(v).reshape(v.shape[0] * v.shape[1], -1)
        d = np.stack([np.frombuffer(hashlib.blake2b(r.tobytes(), digest_size=16).digest(), np.uint8) for r in rows])
        return k + DIGEST, d.reshape(v.shape[0], v.shape[1], 16)
    return k, v


def record(cases, precisions, lib, path):
    data = {}
    for prec in precisions:
        union = dict.fromkeys(SITUATIONS, False)
        for case in cases:
            seen = dict.fromkeys(SITUATIONS, False)
            rows = []
            got = rollout(case, prec, lib, seen=seen, rows_out=rows)
            plain = rollout(case, prec, lib)
            for k in got:
                assert got[k].tobytes() == plain[k].tobytes(), "watching the rollout changed it: %s" % k
            print(case, prec, "episode ends:", int(got["episode_end"].sum()), "seen:", [i for i, s in enumerate(SITUATIONS) if seen[s]], "rows in front of each step:", rows)
            if case in DUO_V1:
                for s in SITUATIONS:
                    union[s] |= seen[s]
            for k, v in got.items():
                k2, v2 = pack(k, v)
                data["%s_f%d_%s" % (case, prec, k2)] = v2
        missing = [s for s in SITUATIONS if not union[s]]
        if missing:
            raise SystemExit("f%d: the recorded steps of %s lack: %s -- change the start states" % (prec, DUO_V1, missing))
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


def compare(gold, case, precision, got):
    """byte comparison of one rollout against its recorded arrays (or their row digests); returns the list of differing (key, step, env)"""
    pre = "%s_f%d_" % (case, precision)
    got = dict(pack(k, v) for k, v in got.items())
    keys = sorted(k[len(pre):] for k in gold.files if k.startswith(pre))
    assert keys and sorted(got) == keys, (keys, sorted(got))
    bad = []
    for k in keys:
        g = gold[pre + k]
        assert got[k].dtype == g.dtype and got[k].shape == g.shape, k
        diff = (np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(g).view(np.uint8)).reshape(g.shape[0], g.shape[1], -1).any(axis=2)
        bad += [(k, int(i), int(e)) for i, e in np.argwhere(diff)]
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "device":
        record(DEVICE_CASES, (32,), os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]))
    else:
        lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "emu", "libdm_emu.so")
        record(EMU_CASES, (32, 64), lib, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(HERE, "duo_dofrec_bits.npz"))
