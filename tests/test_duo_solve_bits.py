"""The two-per-wave kernel's factor / solve chains keep their arithmetic: bitwise comparison against a recorded rollout.

tests/golden/duo_solve_bits.npz was recorded with tests/golden/make_duo_solve_bits.py from the emulator build (tests/emu) of commit
c40d3e3, the parent of the change that made the column reads of DuoSim::back_substitute branch-free: humanoid3d_walk, wave
packing 2, 4 envs (two of them started 3 / 5 cm inside the ground, so the partners of a pair carry different contact sets), 7
open-loop control steps with the episode timer at 0.1 s (every env passes an auto-reset), fp32 and fp64.  Every output of a
control step (observation, reward, the three flags) and the simulation state behind it (pose, velocity, flag words) must
reproduce bit for bit.  This pins "same operations in the same order" for the sources as the CPU compiles them; what the GPU
compiler makes of them (FMA contraction) is pinned by tests/test_replay.py on the device.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_solve_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_solve_bits.npz")
KEYS = ("state", "reward", "terminate", "valid", "episode_end", "pose", "vel", "flags")


@pytest.mark.parametrize("precision", [32, 64])
def test_duo_rollout_bits(emu_lib, precision):
    gold = np.load(GOLDEN)
    got = rec.rollout(precision, emu_lib)
    assert gold["f%d_episode_end" % precision].sum() >= rec.N, "the fixture must pass through auto-resets"
    for k in KEYS:
        g = gold["f%d_%s" % (precision, k)]
        assert got[k].dtype == g.dtype and got[k].shape == g.shape, k
        same = got[k].view(np.uint8) == g.view(np.uint8)
        assert same.all(), "%s differs from the recorded rollout at (step, env) %s" % (
            k, sorted({(int(i[0]), int(i[1])) for i in np.argwhere(got[k] != g)})[:8])
