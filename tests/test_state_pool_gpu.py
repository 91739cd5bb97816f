"""tests/test_state_pool.py on the device (tests/state_pool_common.py): libdm_hip.so, fp32 contexts, the plain scene in fp64 as well.  Checks 1 and 2 run each of
the seven cases once, every later check one case.  Invalid slots are an emulator check; here the host's refusals by name."""
import pytest

import state_pool_common as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,physics", pc.SCENES)
def test_rewind_gpu(hip_lib, case, physics):
    pc.rewind(case, hip_lib, 32, 4, physics)


@pytest.mark.parametrize("n,packing,prec", [(3, 0, 32), (4, 1, 32), (4, 0, 64)])
def test_rewind_plain_odd_packing_f64_gpu(hip_lib, n, packing, prec):
    pc.rewind("plain", hip_lib, prec, n, packing=packing)


@pytest.mark.parametrize("case,physics", pc.SCENES)
def test_emitted_rows_gpu(hip_lib, case, physics):
    pc.emitted_rows(case, hip_lib, 32, 4, physics)


@pytest.mark.parametrize("n,packing", [(4, 0), (3, 0), (4, 1)])
def test_across_envs_and_inside_a_pair_gpu(hip_lib, n, packing):
    pc.across_envs(hip_lib, 32, n, packing)


def test_draw_keys_stay_the_envs_own_gpu(hip_lib):
    pc.own_keys(hip_lib, 32)


def test_the_pool_is_data_gpu(hip_lib):
    pc.pool_is_data(hip_lib, 32)


@pytest.mark.parametrize("prec", [32, 64])
def test_new_episode_gpu(hip_lib, prec):
    pc.new_episode("amp_dribble_zombie", hip_lib, prec)


def test_new_episode_draws_anew_rewind_repeats_gpu(hip_lib):
    pc.fresh_draws(hip_lib, 32)


def test_masks_gpu(hip_lib):
    pc.masks("amp_heading_clips4", hip_lib, 32)


def test_refusals_gpu(hip_lib):
    pc.refusals(hip_lib, 32)


def test_determinism_gpu(hip_lib):
    assert pc.rewind("amp_perturbed", hip_lib, 32, 4) == pc.rewind("amp_perturbed", hip_lib, 32, 4)
