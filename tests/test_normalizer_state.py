"""`DeviceNormalizer.state_host` / `set_state` (`dm_norm_set_state`): a learner's checkpoint puts the statistics back word for word -- mean_sq as stored, not rebuilt
from std as `set_mean_std` does -- so that a resumed normaliser continues with the bits of the run that never stopped.  On the CPU emulator build through host rows."""
import numpy as np
import pytest

from deepmimic_amd.normalizer import DeviceNormalizer


def _rows(rng, n, size):
    return (rng.normal(size=(n, size)) * np.linspace(0.01, 30.0, size) + np.linspace(-5.0, 5.0, size)).astype(np.float32)


def _bytes(st):
    return b"".join(np.asarray(st[k]).tobytes() for k in ("mean", "std", "mean_sq")) + np.int64(st["count"]).tobytes()


@pytest.mark.parametrize("groups", [None, "mixed"])
def test_set_state_resumes_bit_for_bit(emu_lib, groups):
    size = 37
    gids = None if groups is None else np.array([0] * 10 + [1] * 9 + [-1] * 3 + [2] * 15, np.int32)
    rng = np.random.default_rng(5)
    first, second = [_rows(rng, 100 + 7 * k, size) for k in range(3)], [_rows(rng, 64, size) for _ in range(2)]
    straight = DeviceNormalizer(size, groups_ids=gids, lib_path=emu_lib)
    for x in first:
        straight.record(x); straight.update()
    saved = straight.state_host()
    assert saved["count"] == sum(x.shape[0] for x in first) and saved["mean"].dtype == np.float64 and saved["mean_sq"].shape == (size,)
    resumed = DeviceNormalizer(size, groups_ids=gids, lib_path=emu_lib)
    resumed.set_state(saved["mean"], saved["std"], saved["mean_sq"], saved["count"])
    assert _bytes(resumed.state_host()) == _bytes(saved)
    # what a normalised row looks like is restored too (mean and 1 / std as the kernels read them)
    x = _rows(rng, 5, size)
    out = [np.zeros_like(x), np.zeros_like(x)]
    for n, o in zip((straight, resumed), out):
        n.normalize_device(x.ctypes.data, 5, o.ctypes.data)
    assert out[0].tobytes() == out[1].tobytes() and np.isfinite(out[0]).all()
    for y in second:
        for n in (straight, resumed):
            n.record(y); n.update()
    assert _bytes(resumed.state_host()) == _bytes(straight.state_host())
    # the reason for the entry point: set_mean_std rebuilds mean_sq = std^2 + mean^2, which is not the stored word in every column
    rebuilt = DeviceNormalizer(size, groups_ids=gids, lib_path=emu_lib)
    rebuilt.set_mean_std(saved["mean"], saved["std"], count=saved["count"])
    assert rebuilt.state_host()["mean_sq"].tobytes() != saved["mean_sq"].tobytes()


def test_set_state_refusals(emu_lib):
    n = DeviceNormalizer(4, lib_path=emu_lib)
    ok = np.ones(4)
    with pytest.raises(ValueError, match="expecting size 4"):
        n.set_state(np.ones(3), ok, ok, 1)
    with pytest.raises(RuntimeError, match="std must be positive"):
        n.set_state(ok, np.array([1.0, 0.0, 1.0, 1.0]), ok, 1)
    with pytest.raises(RuntimeError, match="count must be >= 0"):
        n.set_state(ok, ok, ok, -1)
