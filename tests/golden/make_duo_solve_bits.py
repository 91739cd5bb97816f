"""Records tests/golden/duo_solve_bits.npz for tests/test_duo_solve_bits.py from the emulator build of the CURRENT checkout:

    make -C oracle && make -C tests/emu && python tests/golden/make_duo_solve_bits.py

Run it on the commit whose arithmetic is to be pinned (the parent of a change that must keep results bit for bit), never on
the change itself."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["DM_ALLOW_EMULATOR"] = "1"

N, STEPS, SEED, TIME_LIM, LIFTS = 4, 7, 11, 0.1, (0.0, -0.03, 0.0, -0.05)


def rollout(precision, lib_path):
    """humanoid3d_walk, two characters per wavefront, open loop through auto-resets: the episode timer ends every third control
    step; envs 1 and 3 start pressed 3 / 5 cm into the ground (more contact rows, the partners of a pair differ)."""
    from deepmimic_amd import model
    from deepmimic_amd.core import BatchEnv
    t = model.load_asset("humanoid3d_walk")
    t.cfg.time_lim_min = t.cfg.time_lim_max = TIME_LIM
    env = BatchEnv(t, N, precision=precision, lib_path=lib_path, wave_packing=2, seed=SEED)
    env.reset()
    st = env.get_state()
    st["pose"][:, 1] += np.asarray(LIFTS)
    env.set_state(pose=st["pose"], vel=st["vel"], tar=st["tar"], kin=st["kin"], clocks=st["clocks"], flags=st["flags"])
    rec = {k: [] for k in ("state", "reward", "terminate", "valid", "episode_end", "pose", "vel", "flags")}
    for _ in range(STEPS):
        out = env.step(None, 1.0 / 600, 20, open_loop=True, auto_reset=True)
        snap = env.get_state()
        for k in ("state", "reward", "terminate", "valid", "episode_end"):
            rec[k].append(out[k].copy())
        for k in ("pose", "vel", "flags"):
            rec[k].append(snap[k].copy())
    env.close()
    return {k: np.stack(v) for k, v in rec.items()}


if __name__ == "__main__":
    lib = os.path.join(ROOT, "tests", "emu", "libdm_emu.so")
    data = {}
    for prec in (32, 64):
        for k, v in rollout(prec, lib).items():
            data["f%d_%s" % (prec, k)] = v
        print(prec, "episode ends:", int(data["f%d_episode_end" % prec].sum()), "rewards:", data["f%d_reward" % prec][:, 0])
    np.savez_compressed(os.path.join(HERE, "duo_solve_bits.npz"), **data)
