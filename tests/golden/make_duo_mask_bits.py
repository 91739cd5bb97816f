"""Records the fixtures of tests/test_duo_mask_bits.py (emulator) and tests/test_duo_device_bits.py (MI355X) from a build of the CURRENT checkout:

    make -C oracle && make -C tests/emu && python tests/golden/make_duo_mask_bits.py              ->  tests/golden/duo_mask_bits.npz
    python tests/golden/make_duo_mask_bits.py device <libdm_hip.so> <out.npz>                     ->  the device fixture (fp32, on the GPU)

Run it on the commit whose arithmetic is to be pinned (the parent of a change that must keep results bit for bit), never on
the change itself.  The rollouts are those of make_duo_solve_bits.py on the instantiations of the two-per-wave kernel that
fixture does not reach; the family that ran is asked of the library and asserted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["DM_ALLOW_EMULATOR"] = "1"

N, STEPS, SEED, TIME_LIM, LIFTS, SIGMA = 4, 7, 11, 0.1, (0.0, -0.03, 0.0, -0.05), 0.15
# case -> (asset, DM-physics version, the kernel family that must have run)
CASES = {
    "walk": ("humanoid3d_walk", 1, 0),           # plain instantiation (device fixture only: duo_solve_bits.npz holds it on the emulator)
    "amp": ("amp_heading_zombie", 1, 1),         # AMP / goal instantiation
    "v2": ("humanoid3d_walk", 2, 22),            # DM-physics v2
    "dribble": ("amp_dribble_zombie", 1, 24),    # biped + free body
}
EMU_CASES, DEVICE_CASES = ("amp", "v2", "dribble"), ("walk", "amp", "v2", "dribble")
OUT_KEYS = ("state", "reward", "terminate", "valid", "episode_end")


def rollout(case, precision, lib_path):
    """Two characters per wavefront, seeded random actions through auto-resets: the episode timer ends every third control step;
    envs 1 and 3 start pressed 3 / 5 cm into the ground (the partners of a pair carry different row counts and refresh their
    friction bounds at different rows).  Returns every output of the control steps and the whole snapshot behind each."""
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    asset, physics, family = CASES[case]
    t = model.load_asset(asset)
    t.cfg.time_lim_min = t.cfg.time_lim_max = TIME_LIM
    env = BatchEnv(t, N, precision=precision, lib_path=lib_path, wave_packing=2, physics=physics, seed=SEED)
    env.reset()
    st = env.get_state()
    st["pose"][:, 1] += np.asarray(LIFTS)
    env.set_state(pose=st["pose"], vel=st["vel"], tar=st["tar"], kin=st["kin"], clocks=st["clocks"], flags=st["flags"])
    rng = np.random.default_rng(SEED + 100)
    rec = {}
    for _ in range(STEPS):
        acts = (SIGMA * rng.normal(size=(N, env.A))).astype(np.float32)
        out = env.step(acts, 1.0 / 600, 20, auto_reset=True)
        fam = env.debug("family")
        assert (fam == family).all(), (case, fam)
        snap = env.snapshot()
        for k in OUT_KEYS:
            rec.setdefault(k, []).append(out[k].copy())
        for k, v in snap.items():
            rec.setdefault("snap_" + k, []).append(np.array(v, copy=True))
    env.close()
    return {k: np.stack(v) for k, v in rec.items()}


def record(cases, precisions, lib, path):
    data = {}
    for case in cases:
        for prec in precisions:
            for k, v in rollout(case, prec, lib).items():
                data["%s_f%d_%s" % (case, prec, k)] = v
            pre = "%s_f%d_" % (case, prec)
            print(case, prec, "episode ends:", int(data[pre + "episode_end"].sum()), "rewards:", data[pre + "reward"][:, 1])
    np.savez_compressed(path, **data)


def compare(gold, case, precision, got):
    """byte comparison of one rollout against its recorded arrays; returns the list of differing (key, step, env)"""
    pre = "%s_f%d_" % (case, precision)
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
        record(EMU_CASES, (32, 64), os.path.join(ROOT, "tests", "emu", "libdm_emu.so"), os.path.join(HERE, "duo_mask_bits.npz"))
