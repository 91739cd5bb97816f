"""The Gauss-Seidel sweep of the two-per-wave kernel (DuoSim::substep_post: DM_DUO_PGS_ROW / DM_DUO_PGS_BLK) keeps its results bit for bit:
which visits carry the friction-refresh test is a matter of issue slots, never of arithmetic.

tests/golden/duo_sweep_bits.npz (emulator, fp32 and fp64) and tests/golden/duo_sweep_device_bits.npz (MI355X, fp32) were recorded with
tests/golden/make_duo_sweep_bits.py from commit ceabe35, the parent of the change that tests the refresh predicate once per block of
four visits: wave packing 2, 8 envs started 0 to 6 cm inside the ground, two of them lying on their side (the halves of a pair differ
in contact count), 7 control steps of seeded random actions with the episode timer at 0.1 s (every env passes an auto-reset), on
* humanoid3d_walk      the plain instantiation (family 0),
* amp_heading_zombie   the AMP / goal instantiation (family 1; its first steps also run pairs with more than 32 rows),
with 10 solver iterations and with 1.  The recorder watched the row counts after every control step and wrote the fixture only because
the humanoid3d_walk rollouts hold: a pair whose two refresh rows NL + nc lie in one block of four and a pair with them in different
blocks, refresh rows = 0 and = 3 mod 4, a character without contact, a pair with Rv >= 25 and one with Rv <= 8.
Every output of a control step (observation, reward, the three flags) and the whole snapshot behind it (pose, velocity, PD target,
clocks, flag words, goal rows) must reproduce bit for bit; the wide arrays are held as a digest per (control step, env) row.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_sweep_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "duo_sweep_bits.npz"))


@pytest.fixture(scope="module")
def gold_device():
    return np.load(os.path.join(GOLDEN, "duo_sweep_device_bits.npz"))


def check(gold, name, precision, lib):
    assert gold["%s_f%d_episode_end" % (name, precision)].sum() >= rec.N, "the fixture must pass through auto-resets"
    bad = rec.compare(gold, name, precision, rec.rollout(name, precision, lib))
    assert not bad, "%s f%d differs from the recorded rollout at (array, step, env) %s" % (name, precision, bad[:8])


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("name", rec.case_names())
def test_duo_sweep_rollout_bits(emu_lib, gold, name, precision):
    check(gold, name, precision, emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", rec.case_names())
def test_duo_sweep_device_rollout_bits(hip_lib, gold_device, name):
    check(gold_device, name, 32, hip_lib)
