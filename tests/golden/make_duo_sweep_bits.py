"""Records the fixtures of tests/test_duo_sweep_bits.py from a build of the CURRENT checkout:

    make -C tests/emu && python tests/golden/make_duo_sweep_bits.py                               ->  tests/golden/duo_sweep_bits.npz (emulator, fp32 and fp64)
    python tests/golden/make_duo_sweep_bits.py device <libdm_hip.so> <out.npz>                    ->  the device fixture (fp32, on the GPU)

Run it on the commit whose arithmetic is to be pinned (the parent of a change that must keep results bit for bit), never on
the change itself.  The rollouts aim at the Gauss-Seidel sweep of the two-per-wave kernel (DuoSim::substep_post): which rows a
pair visits, in which block of four its two friction-refresh rows NL + nc lie, and how many iterations run.  The recorder
watches the row counts of every pair after every control step and refuses to write a fixture that misses one of the
situations listed in `coverage`."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["DM_ALLOW_EMULATOR"] = "1"

N, STEPS, SEED, TIME_LIM, SIGMA = 8, 7, 23, 0.1, 0.15
# how deep each env starts in the ground (m); envs LYING start on their side just above it: the halves of a pair (envs 2k, 2k + 1) differ in contacts
DEPTHS = (0.0, 0.06, 0.01, 0.0, 0.02, 0.05, 0.03, 0.04)
LYING = (3, 4)
LYING_HEIGHT = 0.16
# case -> (asset, the kernel family that must have run)
CASES = {"walk": ("humanoid3d_walk", 0), "amp": ("amp_heading_zombie", 1)}
ITERS = (10, 1)
OUT_KEYS = ("state", "reward", "terminate", "valid", "episode_end")


def case_names():
    return ["%s_it%d" % (c, it) for c in CASES for it in ITERS]


def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def rollout(name, precision, lib_path, rows_out=None):
    """Two characters per wavefront, seeded random actions through auto-resets (the episode timer ends every third control step).
    Returns every output of the control steps and the whole snapshot behind each.  With `rows_out` (a list) a second env object is
    set to every snapshot and asked for the constraint rows and contacts of the substep that follows it (FLG_NROWS, FLG_NCONT): N x 2
    per control step, appended to the list; the recorded env is never touched by that."""
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    case, iters = name.rsplit("_it", 1)
    asset, family = CASES[case]
    t = model.load_asset(asset)
    t.cfg.time_lim_min = t.cfg.time_lim_max = TIME_LIM
    mk = lambda: BatchEnv(t, N, precision=precision, lib_path=lib_path, wave_packing=2, seed=SEED, solver_iters=int(iters))
    env = mk()
    spy = mk() if rows_out is not None else None
    env.reset()
    st = env.get_state()
    st["pose"][:, 1] -= np.asarray(DEPTHS)
    for e in LYING:       # a quarter turn about z, the root just above the ground
        st["pose"][e, 3:7] = _qmul(np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]), st["pose"][e, 3:7])
        st["pose"][e, 1] = LYING_HEIGHT
    env.set_state(pose=st["pose"], vel=st["vel"], tar=st["tar"], kin=st["kin"], clocks=st["clocks"], flags=st["flags"])
    rng = np.random.default_rng(SEED + 100)
    rec = {}

    def spy_rows(snap):
        spy.restore(snap)
        spy.probe(1, 1.0 / 1200)
        rows_out.append(spy.debug("rows").astype(np.int64))

    if spy is not None:
        spy.reset()
        spy_rows(env.snapshot())
    for _ in range(STEPS):
        acts = (SIGMA * rng.normal(size=(N, env.A))).astype(np.float32)
        out = env.step(acts, 1.0 / 600, 20, auto_reset=True)
        fam = env.debug("family")
        assert (fam == family).all(), (name, fam)
        snap = env.snapshot()
        if spy is not None:
            spy_rows(snap)
        for k in OUT_KEYS:
            rec.setdefault(k, []).append(out[k].copy())
        for k, v in snap.items():
            rec.setdefault("snap_" + k, []).append(np.array(v, copy=True))
    env.close()
    if spy is not None:
        spy.close()
    return {k: np.stack(v) for k, v in rec.items()}


def coverage(rows, NL=4):
    """rows: [control step] N x 2 (rows R = NL + 3 nc, contacts nc) -> which sweep situations the pairs (envs 2k, 2k + 1) went through"""
    seen = dict.fromkeys(("refresh rows in one block of four", "refresh rows in different blocks", "a refresh row = 0 mod 4", "a refresh row = 3 mod 4",
                          "a character without contact", "a pair with Rv >= 25", "a pair with Rv <= 8"), False)
    for r in rows:
        R, nc = r[:, 0], r[:, 1]
        assert ((R == NL + 3 * nc) | (R == 0)).all(), r
        for a in range(0, len(R), 2):
            if R[a] == 0 or R[a + 1] == 0 or max(R[a], R[a + 1]) > 32:
                continue
            rn = (NL + nc[a], NL + nc[a + 1])
            Rv = max(R[a], R[a + 1])
            seen["refresh rows in one block of four"] |= bool(rn[0] // 4 == rn[1] // 4)
            seen["refresh rows in different blocks"] |= bool(rn[0] // 4 != rn[1] // 4)
            seen["a refresh row = 0 mod 4"] |= bool(rn[0] % 4 == 0 or rn[1] % 4 == 0)
            seen["a refresh row = 3 mod 4"] |= bool(rn[0] % 4 == 3 or rn[1] % 4 == 3)
            seen["a character without contact"] |= bool(nc[a] == 0 or nc[a + 1] == 0)
            seen["a pair with Rv >= 25"] |= bool(Rv >= 25)
            seen["a pair with Rv <= 8"] |= bool(Rv <= 8)
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


def record(precisions, lib, path):
    data = {}
    for name in case_names():
        for prec in precisions:
            rows = []
            got = rollout(name, prec, lib, rows_out=rows)
            plain = rollout(name, prec, lib)
            for k in got:
                assert got[k].tobytes() == plain[k].tobytes(), "watching the rows changed the rollout: %s" % k
            seen = coverage(rows)
            print(name, prec, "episode ends:", int(got["episode_end"].sum()), "rows per step:", [list(r[:, 0]) for r in rows])
            missing = [k for k, v in seen.items() if not v]
            if name.startswith("walk") and missing:
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
        record((32,), os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]))
    else:
        record((32, 64), os.path.join(ROOT, "tests", "emu", "libdm_emu.so"), os.path.join(HERE, "duo_sweep_bits.npz"))
