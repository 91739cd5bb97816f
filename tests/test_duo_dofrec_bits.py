"""The readers and writers of the per-dof records of the LDS record (Lds::dofrec: axis, moment arm, v*, bias force) and of the mass matrix rows built from
them keep their results bit for bit: where a word lies, and whether a lane's row of H reaches DuoSim::chol_solve through Lt or in registers (EnvSim::dyn_row<MODE>,
the substep phases of the fp32 two-per-wave kernels), is never a matter of arithmetic.

tests/golden/duo_dofrec_bits.npz (emulator, fp32 and fp64) and tests/golden/duo_dofrec_device_bits.npz (MI355X, fp32) were recorded
with tests/golden/make_duo_dofrec_bits.py from commit c1a02fe, the parent of the change that hands the row over in registers (and that tried,
measured and dropped a pair-interleaved record layout: docs/HISTORY.md 28): 8 envs, 6 control steps of seeded random actions through
auto-resets, fall end off and the first episode timers staggered, on
* walk      humanoid3d_walk, plain two-per-wave instantiation (family 0)            emulator + device
* amp       amp_heading_zombie, AMP / goal instantiation (family 1)                 emulator + device
* v2        humanoid3d_walk under DM-physics v2, two per wave (family 22)           emulator
* dribble   amp_dribble_zombie, biped + free body, two per wave (family 24)         emulator
* tree      humanoid3d_walk, one per wave on the compiled topology (family 15)      emulator: the one-per-wave record stands as it was
Pair 0 starts with one character lying beside a standing one, pair 1 with both pressed into the ground, pair 2 with both lying, pair 3
with knees and elbows bent past their limits.  The recorder watched every control step and wrote the fixtures only because the family-0
and family-1 rollouts of each leg hold: an active limit row on a dof of even index (left knee 26, right elbow 22) and one of odd index
(right knee 15, left elbow 33) -- the two slots of a record pair --, a pair on the 32-row path with contacts on both characters, a pair on
the borrowed-lane path, a pair on the 64-lane fallback, and a character parked mid-step beside a partner that goes on (its next dynamics
pass rebuilds the records).  Every output of a control step (observation, reward, the three flags) and the whole snapshot behind it must
reproduce bit for bit; the wide arrays are held as a digest per (control step, env) row.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_dofrec_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "duo_dofrec_bits.npz"))


@pytest.fixture(scope="module")
def gold_device():
    return np.load(os.path.join(GOLDEN, "duo_dofrec_device_bits.npz"))


def check(gold, case, precision, lib):
    assert gold["%s_f%d_episode_end" % (case, precision)].sum() >= rec.N, "the fixture must pass through auto-resets"
    bad = rec.compare(gold, case, precision, rec.rollout(case, precision, lib))
    assert not bad, "%s f%d differs from the recorded rollout at (array, step, env) %s" % (case, precision, bad[:8])


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("case", rec.EMU_CASES)
def test_duo_dofrec_rollout_bits(emu_lib, gold, case, precision):
    check(gold, case, precision, emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.DEVICE_CASES)
def test_duo_dofrec_device_rollout_bits(hip_lib, gold_device, case):
    check(gold_device, case, 32, hip_lib)
