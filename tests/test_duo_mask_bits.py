"""The two-per-wave kernel's mask and select arithmetic (dyn_row, the sweep set-up, chol_solve) changes no result: bitwise comparison
against recorded rollouts of the instantiations tests/test_duo_solve_bits.py does not reach.

tests/golden/duo_mask_bits.npz was recorded with tests/golden/make_duo_mask_bits.py from the emulator build (tests/emu) of commit
2e4d120, the parent of the change that took the per-entry mask arithmetic out of those loops: wave packing 2, 4 envs (two of them
started 3 / 5 cm inside the ground, so the halves of a pair have different row counts and refresh friction at different rows), 7
control steps of seeded random actions with the episode timer at 0.1 s (every env passes an auto-reset), fp32 and fp64, on
* amp_heading_zombie          the AMP / goal instantiation (family 1),
* humanoid3d_walk, physics=2  DM-physics v2 (family 22),
* amp_dribble_zombie          biped + free body (family 24).
Every output of a control step (observation, reward, the three flags) and the whole snapshot behind it (pose, velocity, clocks, flag
words, goal rows, free body, manifolds) must reproduce bit for bit.  The sources as the CPU compiles them; what the GPU compiler makes
of them is pinned by tests/test_duo_device_bits.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_mask_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_mask_bits.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("case", rec.EMU_CASES)
def test_duo_mask_rollout_bits(emu_lib, gold, case, precision):
    assert gold["%s_f%d_episode_end" % (case, precision)].sum() >= rec.N, "the fixture must pass through auto-resets"
    bad = rec.compare(gold, case, precision, rec.rollout(case, precision, emu_lib))
    assert not bad, "%s f%d differs from the recorded rollout at (array, step, env) %s" % (case, precision, bad[:8])
