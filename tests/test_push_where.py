"""Task-chosen pushes (include/dm_hip.h dm_push_where / dm_push_state; tests/push_common.py has the checks): every check on the CPU emulator, and marked `gpu` on the
device in both precisions.  The closed form keeps the bounds of tests/test_perturbs.py for the same scenario (1e-11 in fp64, 2e-5 in fp32), the rollout against the
oracle that file's bounds for its free-running rollouts; everything else is an equality of bytes, except the heading frame (64 eps |f|, push_common.heading_frame)."""
import numpy as np
import pytest

import push_common as pc

PRECS = [32, 64]


# ---------------------------------------------------------------------------------------------------------------- CPU emulator
def test_closed_form_emulator(emu_lib):
    pc.closed_form(emu_lib, 64, 1e-11)


@pytest.mark.parametrize("asset,n,packing,physics,prec", [s + (64,) for s in pc.SHAPES] + [pc.SHAPES[0] + (32,), pc.SHAPES[1] + (32,)])
def test_equals_host_route_emulator(emu_lib, asset, n, packing, physics, prec):
    pc.equals_host_route(emu_lib, prec, asset, n, packing, physics)


@pytest.mark.parametrize("prec", PRECS)
def test_slot_rule_and_clearing_emulator(emu_lib, prec):
    pc.slot_rule(emu_lib, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_heading_frame_emulator(emu_lib, prec):
    pc.heading_frame(emu_lib, prec)


def test_lifetime_in_updates_emulator(emu_lib):
    pc.lifetime_in_updates(emu_lib, 64)


def test_resets_and_pool_emulator(emu_lib):
    pc.resets_and_pool(emu_lib, 64)


@pytest.mark.parametrize("packing", [1, 2])
def test_nothing_fires_by_itself_emulator(emu_lib, packing):
    pc.nothing_fires(emu_lib, 64, packing)


@pytest.mark.parametrize("packing", [1, 2])
def test_with_the_random_schedule_emulator(emu_lib, packing):
    dr, ds, rows_ok, hits, both, resets, pushed = pc.with_the_random_schedule(emu_lib, 64, packing)
    assert rows_ok and hits > 30 and pushed == 32, (hits, both, resets)
    assert np.median(ds) < 1e-6 and (ds < 1e-5).mean() > 0.8, (np.median(ds), (ds < 1e-5).mean())


def test_invalid_input_emulator(emu_lib):
    pc.invalid_input(emu_lib, 64)


def test_refusals_emulator(emu_lib):
    pc.refusals(emu_lib, 64)


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", [(64, 1e-11), (32, 2e-5)])
def test_closed_form_gpu(hip_lib, prec, tol):
    pc.closed_form(hip_lib, prec, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("asset,n,packing,physics", pc.SHAPES)
def test_equals_host_route_gpu(hip_lib, asset, n, packing, physics, prec):
    pc.equals_host_route(hip_lib, prec, asset, n, packing, physics)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_slot_rule_and_clearing_gpu(hip_lib, prec):
    pc.slot_rule(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_heading_frame_gpu(hip_lib, prec):
    pc.heading_frame(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_lifetime_in_updates_gpu(hip_lib, prec):
    pc.lifetime_in_updates(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_resets_and_pool_gpu(hip_lib, prec):
    pc.resets_and_pool(hip_lib, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", [1, 2])
def test_nothing_fires_by_itself_gpu(hip_lib, packing):
    pc.nothing_fires(hip_lib, 32, packing)


@pytest.mark.gpu
def test_with_the_random_schedule_gpu_fp64(hip_lib):
    dr, ds, rows_ok, hits, both, resets, pushed = pc.with_the_random_schedule(hip_lib, 64, 2)
    assert rows_ok and hits > 30 and pushed == 32, (hits, both, resets)
    assert np.median(ds) < 1e-6 and (ds < 1e-5).mean() > 0.8, (np.median(ds), (ds < 1e-5).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_invalid_input_gpu(hip_lib, prec):
    pc.invalid_input(hip_lib, prec)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    pc.refusals(hip_lib, 32)
