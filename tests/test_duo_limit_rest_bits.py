"""The Gauss-Seidel sweep of the two-per-wave kernel (DuoSim::substep_post) jumps over the joint-limit blocks of an iteration while the limit rows of
both characters of the pair rest (lambda = +0, t < 0): the skipped visits are the identity, so every result stays what it was, bit for bit.

tests/golden/duo_limit_rest_bits.npz (emulator, fp32 and fp64) and tests/golden/duo_limit_rest_device_bits.npz (MI355X, fp32) were recorded with
tests/golden/make_duo_limit_rest_bits.py from commit f3a38ea, the parent of that change, which visits every limit row in every iteration: wave
packing 2, 8 envs, 6 control steps of seeded random actions with the episode timer at 0.1 s (every env passes an auto-reset), on
* humanoid3d_walk                       the plain instantiation (family 0),
* amp_heading_zombie                    the AMP / goal instantiation (family 1),
* humanoid3d_walk under DM-physics v2   NL = 8, two limit blocks (family 22; emulator only),
with 10 solver iterations and with 1.  Start states: a knee (env 0) and an elbow (env 3) 0.05 rad past their bound beside a standing partner, in either
order of the halves, the envs 0 to 6 cm inside the ground; env 4 dropped 3 cm into the ground on knees 1e-3 rad inside their bound, beside a lying
partner (Rv >= 25); a pair well above the ground (no contact, Rv = NL).  The recorder wrote the fixture only because the row counts hold a pair without any contact, a pair with Rv >= 25, one
with Rv <= 8 and one with contacts on both characters.
Every output of a control step (observation, reward, the three flags) and the whole snapshot behind it (pose, velocity, PD target, clocks, flag
words, goal rows) must reproduce bit for bit; the wide arrays are held as a digest per (control step, env) row.

Coverage is counted, not assumed: the tap instantiation of the kernel shares the sweep and counts its decisions per env (dm_get_debug "limit_rest").
The test runs it from the start state and from the state behind every replayed control step and fails unless iterations were skipped, visited for the
env's own limit rows and visited for the partner's alone; with 10 iterations also unless a sweep changed its decision between iterations (with 1
iteration a sweep takes one decision, so there is none to change).  The tap kernel has a two-per-wave family under DM-physics v1 only: the v2 cases
replay without counts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_limit_rest_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "duo_limit_rest_bits.npz"))


@pytest.fixture(scope="module")
def gold_device():
    return np.load(os.path.join(GOLDEN, "duo_limit_rest_device_bits.npz"))


def check(gold, name, precision, lib):
    assert gold["%s_f%d_episode_end" % (name, precision)].sum() >= rec.N, "the fixture must pass through auto-resets"
    counted = name.rsplit("_it", 1)[0] in rec.TAP_CASES
    taps = [] if counted else None
    bad = rec.compare(gold, name, precision, rec.rollout(name, precision, lib, taps=taps))
    assert not bad, "%s f%d differs from the recorded rollout at (array, step, env) %s" % (name, precision, bad[:8])
    if counted:
        total = np.sum(taps, axis=0)        # N x 4
        print(name, "f%d" % precision, "limit_rest counts per env (skipped | own | partner only | changed):", total.tolist())
        need = 4 if name.endswith("_it10") else 3
        missing = [rec.COUNTERS[k] for k in range(need) if total[:, k].sum() == 0]
        assert not missing, "%s f%d: the fixture's states never ran: %s" % (name, precision, missing)
        # the two characters of a pair share every decision: what one counts as its own the other counts as its partner's, or as its own too
        pairs = total.reshape(-1, 2, 4)
        assert (pairs[:, 0, 0] == pairs[:, 1, 0]).all() and (pairs[:, 0, 3] == pairs[:, 1, 3]).all(), total.tolist()
        assert (pairs[:, :, :3].sum(axis=2)[:, 0] == pairs[:, :, :3].sum(axis=2)[:, 1]).all(), total.tolist()


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("name", rec.case_names(rec.EMU_CASES))
def test_duo_limit_rest_rollout_bits(emu_lib, gold, name, precision):
    check(gold, name, precision, emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", rec.case_names(rec.DEVICE_CASES))
def test_duo_limit_rest_device_rollout_bits(hip_lib, gold_device, name):
    check(gold_device, name, 32, hip_lib)
