"""The device state pool (`dm_state_save` / `dm_state_restore`, k_state_save and k_state_restore of dm_device.h) on the CPU emulator, both precisions.  The method and
the checks are in tests/state_pool_common.py; tests/test_state_pool_gpu.py runs them on the device."""
import pytest

import state_pool_common as pc


@pytest.mark.parametrize("n", [4, 3])
@pytest.mark.parametrize("case,physics", pc.SCENES)
def test_rewind(emu_lib, case, physics, n):
    pc.rewind(case, emu_lib, 64, n, physics)


@pytest.mark.parametrize("packing", [1, 2])
@pytest.mark.parametrize("case", ["plain", "amp_heading_clips4"])
def test_rewind_f32_both_packings(emu_lib, case, packing):
    pc.rewind(case, emu_lib, 32, 4, packing=packing)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case,physics", pc.SCENES)
def test_emitted_rows(emu_lib, case, physics, prec):
    pc.emitted_rows(case, emu_lib, prec, 4 if prec == 64 else 3, physics)


@pytest.mark.parametrize("n,packing,prec", [(4, 0, 64), (3, 0, 64), (4, 1, 64), (4, 2, 32), (3, 1, 32)])
def test_across_envs_and_inside_a_pair(emu_lib, n, packing, prec):
    pc.across_envs(emu_lib, prec, n, packing)


@pytest.mark.parametrize("prec", [64, 32])
def test_draw_keys_stay_the_envs_own(emu_lib, prec):
    pc.own_keys(emu_lib, prec)


@pytest.mark.parametrize("prec", [64, 32])
def test_the_pool_is_data(emu_lib, prec):
    pc.pool_is_data(emu_lib, prec)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", ["amp_dribble_zombie", "amp_perturbed", "amp_heading_clips4", "plain"])
def test_new_episode(emu_lib, case, prec):
    pc.new_episode(case, emu_lib, prec)


def test_new_episode_draws_anew_rewind_repeats(emu_lib):
    pc.fresh_draws(emu_lib, 64)


@pytest.mark.parametrize("prec", [64, 32])
def test_masks(emu_lib, prec):
    pc.masks("amp_heading_clips4", emu_lib, prec)


@pytest.mark.parametrize("prec", [64, 32])
def test_invalid_slots(emu_lib, prec):
    pc.invalid_slots(emu_lib, prec)


@pytest.mark.parametrize("prec", [64, 32])
def test_refusals(emu_lib, prec):
    pc.refusals(emu_lib, prec)


def test_determinism(emu_lib):
    assert pc.rewind("amp_perturbed", emu_lib, 64, 4) == pc.rewind("amp_perturbed", emu_lib, 64, 4)
