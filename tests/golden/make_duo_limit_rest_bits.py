"""Records the fixtures of tests/test_duo_limit_rest_bits.py from a build of the CURRENT checkout:

    make -C tests/emu && python tests/golden/make_duo_limit_rest_bits.py                          ->  tests/golden/duo_limit_rest_bits.npz (emulator, fp32 and fp64)
    python tests/golden/make_duo_limit_rest_bits.py device <libdm_hip.so> <out.npz>               ->  the device fixture (fp32, on the GPU)

Run it on the commit whose arithmetic is to be pinned (the parent of a change that must keep results bit for bit), never on
the change itself.  The rollouts aim at the joint-limit rows of the two-per-wave kernel's Gauss-Seidel sweep (DuoSim::substep_post):
rows 0 .. NL - 1 of every character, the first block(s) of four of every iteration, which the sweep may jump over while the limit rows of
both characters of the pair rest.  The recorder watches the row counts of every pair after every control step and refuses to write a fixture
that misses one of the row-count situations listed in `coverage`; whether the limit rows rested, were active in one half or the other, or
changed inside a sweep is counted by the tap kernel (dm_get_debug "limit_rest") -- which the commit being recorded need not have: the test
counts over the rollout it replays (`rollout(..., taps=...)`)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["DM_ALLOW_EMULATOR"] = "1"

N, STEPS, SEED, TIME_LIM, SIGMA = 8, 6, 49, 0.1, 0.15
# Start states (the halves of a pair are envs 2k, 2k + 1):
#   pair 0  env 0: a knee PAST rad beyond its bound, env 1 stands             -> a limit row active from iteration 0 in half 0, the partner's at rest
#   pair 1  env 2 stands, env 3: an elbow PAST rad beyond its bound           -> the same with the halves in the other order
#   pair 2  env 4 dropped into the ground on straight knees, env 5 lying      -> contact impulses drive a knee into its bound during the sweep; Rv >= 25
#   pair 3  both well above the ground                                        -> a pair without any contact, Rv = NL <= 8
# every env but pair 3 starts DEPTHS inside the ground (0 to 6 cm)
DEPTHS = (0.0, 0.06, 0.02, 0.01, 0.03, 0.0, 0.0, 0.0)
LYING = {5: 0.22}            # env -> height of its root (m) after a quarter turn about z
AIRBORNE = {6: 0.6, 7: 0.9}  # env -> how far its root is lifted (m)
PAST = 0.05                  # rad
KNEE_GAP = 1e-3              # rad: how far inside their bound the "straight" knees of env 4 start
# case -> (asset, DM-physics version, the kernel family that must have run)
CASES = {"walk": ("humanoid3d_walk", 1, 0), "amp": ("amp_heading_zombie", 1, 1), "v2": ("humanoid3d_walk", 2, 22)}
EMU_CASES, DEVICE_CASES = ("walk", "amp", "v2"), ("walk", "amp")
TAP_CASES = ("walk", "amp")  # the tap kernel has a two-per-wave family under DM-physics v1 only (dm_probe 5)
ITERS = (10, 1)
TAP_UPDATES = 4              # updates the tap kernel runs from the start state and from the state behind every control step
OUT_KEYS = ("state", "reward", "terminate", "valid", "episode_end")
COUNTERS = ("iterations that skipped the limit blocks", "iterations that visited them for the env's own limit rows",
            "iterations that visited them for the partner's limit rows only", "sweeps in which the decision changed between iterations")


def case_names(cases):
    return ["%s_it%d" % (c, it) for c in cases for it in ITERS]


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def limit_joints(t):
    """the limit rows of a character in row order: (joint name, pose offset, lower bound, upper bound) of every revolute joint with lo <= hi"""
    from deepmimic_amd import model as M
    jm, out = t.joint_mat, []
    for j in range(1, jm.shape[0]):
        if int(jm[j, M.JD_TYPE]) == M.JT_REVOLUTE and jm[j, M.JD_LL0] <= jm[j, M.JD_LH0]:
            out.append((int(jm[j, M.JD_PARAM_OFFSET]), float(jm[j, M.JD_LL0]), float(jm[j, M.JD_LH0])))
    return out


def start_state(t, st):
    """the start poses described above; knees are limit rows 0 and 2, elbows 1 and 3 (humanoid3d.txt joint order: right leg, right arm, left leg, left arm)"""
    lims = limit_joints(t)
    assert len(lims) == 4, lims
    pose = st["pose"]
    pose[:, 1] -= np.asarray(DEPTHS)
    for e, height in LYING.items():
        pose[e, 3:7] = _qmul(np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]), pose[e, 3:7])
        pose[e, 1] = height
    for e, lift in AIRBORNE.items():
        pose[e, 1] += lift
    straight = lambda lo, hi: hi if abs(hi) <= abs(lo) else lo      # the bound next to the straight joint (angle 0)
    inward = lambda lo, hi: -1.0 if abs(hi) <= abs(lo) else 1.0     # from that bound into the range
    off, lo, hi = lims[0]; pose[0, off] = straight(lo, hi) - PAST * inward(lo, hi)       # env 0: right knee past its bound
    off, lo, hi = lims[3]; pose[3, off] = straight(lo, hi) - PAST * inward(lo, hi)       # env 3: left elbow past its bound
    for r in (0, 2):                                                                      # env 4: both knees a hair inside their bound
        off, lo, hi = lims[r]; pose[4, off] = straight(lo, hi) + KNEE_GAP * inward(lo, hi)
    return st


def rollout(name, precision, lib_path, rows_out=None, taps=None):
    """Two characters per wavefront, seeded random actions through auto-resets (the episode timer ends every third control step).
    Returns every output of the control steps and the whole snapshot behind each.  With `rows_out` (a list) a second env object is
    set to the start state and to every snapshot and asked for the constraint rows and contacts of the substep that follows it: N x 2
    per state, appended to the list.  With `taps` (a list) that env runs TAP_UPDATES scene updates on the two-per-wave tap kernel from
    each of those states and its N x 4 "limit_rest" counts (COUNTERS) of every update are appended.  The recorded env is never touched
    by either."""
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    case, iters = name.rsplit("_it", 1)
    asset, physics, family = CASES[case]
    t = model.load_asset(asset)
    t.cfg.time_lim_min = t.cfg.time_lim_max = TIME_LIM
    t.cfg.enable_fall_end = False          # (the lying character stays in its episode; episodes end by their timers)
    mk = lambda: BatchEnv(t, N, precision=precision, lib_path=lib_path, wave_packing=2, physics=physics, seed=SEED, solver_iters=int(iters))
    env = mk()
    spy = mk() if (rows_out is not None or taps is not None) else None
    env.reset()
    st = start_state(t, env.get_state())
    env.set_state(pose=st["pose"], vel=st["vel"], tar=st["tar"], kin=st["kin"], clocks=st["clocks"], flags=st["flags"])
    rng = np.random.default_rng(SEED + 100)
    rec = {}

    def watch(snap):
        if rows_out is not None:
            spy.restore(snap)
            spy.probe(1, 1.0 / 1200)
            rows_out.append(spy.debug("rows").astype(np.int64))
        if taps is not None:
            spy.restore(snap)
            for _ in range(TAP_UPDATES):
                spy.probe(5, 1.0 / 600)
                taps.append(spy.debug("limit_rest").astype(np.int64))

    if spy is not None:
        spy.reset()
        watch(env.snapshot())
    for _ in range(STEPS):
        acts = (SIGMA * rng.normal(size=(N, env.A))).astype(np.float32)
        out = env.step(acts, 1.0 / 600, 20, auto_reset=True)
        fam = env.debug("family")
        assert (fam == family).all(), (name, fam)
        snap = env.snapshot()
        if spy is not None:
            watch(snap)
        for k in OUT_KEYS:
            rec.setdefault(k, []).append(out[k].copy())
        for k, v in snap.items():
            rec.setdefault("snap_" + k, []).append(np.array(v, copy=True))
    env.close()
    if spy is not None:
        spy.close()
    return {k: np.stack(v) for k, v in rec.items()}


def coverage(rows, NL):
    """rows: [state] N x 2 (rows R = NL + 3 nc, contacts nc) -> which row-count situations the pairs (envs 2k, 2k + 1) went through"""
    seen = dict.fromkeys(("a pair without any contact", "a pair with Rv >= 25", "a pair with Rv <= 8", "a pair with contacts on both characters"), False)
    for r in rows:
        R, nc = r[:, 0], r[:, 1]
        for a in range(0, len(R), 2):
            if R[a] == 0 or R[a + 1] == 0 or max(R[a], R[a + 1]) > 32:
                continue
            Rv = max(R[a], R[a + 1])
            seen["a pair without any contact"] |= bool(nc[a] == 0 and nc[a + 1] == 0)
            seen["a pair with Rv >= 25"] |= bool(Rv >= 25)
            seen["a pair with Rv <= 8"] |= bool(Rv <= 8)
            seen["a pair with contacts on both characters"] |= bool(nc[a] > 0 and nc[a + 1] > 0)
    return seen


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
    for name in case_names(cases):
        for prec in precisions:
            rows = []
            got = rollout(name, prec, lib, rows_out=rows)
            plain = rollout(name, prec, lib)
            for k in got:
                assert got[k].tobytes() == plain[k].tobytes(), "watching the rows changed the rollout: %s" % k
            seen = coverage(rows, 8 if name.startswith("v2") else 4)
            print(name, prec, "episode ends:", int(got["episode_end"].sum()), "rows per state:", [list(r[:, 0]) for r in rows])
            missing = [k for k, v in seen.items() if not v]
            if missing:
                raise SystemExit("%s f%d: the recorded steps lack: %s -- change the start poses" % (name, prec, missing))
            for k, v in got.items():
                k2, v2 = pack(k, v)
                data["%s_f%d_%s" % (name, prec, k2)] = v2
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


def compare(gold, name, precision, got):
    """byte comparison of one rollout against its recorded arrays (or their row digests); returns the list of differing (key, step, env)"""
    pre = "%s_f%d_" % (name, precision)
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
        record(EMU_CASES, (32, 64), lib, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(HERE, "duo_limit_rest_bits.npz"))
