"""What the GPU compiler makes of the two-per-wave step kernel (FMA contraction, operation order), pinned against a fixed commit.

tests/golden/duo_device_bits.npz was recorded on an MI355X with tests/golden/make_duo_mask_bits.py (`device` mode) from the libdm_hip.so
of commit 2e4d120, the parent of the change that took the per-entry mask arithmetic out of dyn_row, the sweep set-up and chol_solve:
the rollouts of tests/test_duo_mask_bits.py in fp32, on the plain instantiation (family 0) as well as families 1, 22 and 24.  Outputs
and snapshots must reproduce byte for byte: an edit of the kernel that moves one rounding fails here, on the device, where the emulator
tests cannot see it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_duo_mask_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_device_bits.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.DEVICE_CASES)
def test_duo_device_rollout_bits(hip_lib, gold, case):
    assert gold["%s_f32_episode_end" % case].sum() >= rec.N, "the fixture must pass through auto-resets"
    bad = rec.compare(gold, case, 32, rec.rollout(case, 32, hip_lib))
    assert not bad, "%s differs from the recorded rollout at (array, step, env) %s" % (case, bad[:8])
