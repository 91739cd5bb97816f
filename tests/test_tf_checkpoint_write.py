"""deepmimic_amd/tf_checkpoint.py write_checkpoint and agent_variables: the writer against the reader (bits and checksums), the variable set of a saved agent
against the shipped checkpoints' (tests/golden/ckpt_names_*.json: names, shapes and dtypes read once with read_index from three shipped .index files)."""
import json
import os

import numpy as np
import pytest

from deepmimic_amd import tf_checkpoint as tfc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tensors(seed=0):
    rng = np.random.default_rng(seed)
    t = {"agent/main/actor/0/dense/kernel": rng.normal(size=(37, 64)).astype(np.float32), "agent/main/actor/0/dense/bias": rng.normal(size=64).astype(np.float32),
         "agent/resource/s_norm/count": np.array([12345], np.int32), "agent/resource/g_norm/mean": np.zeros(0, np.float32),
         "agent/resource/big": rng.normal(size=(300, 100)).astype(np.float32),             # 120 000 bytes: past read_tensors' default verify_below
         "agent/wide/int64": np.arange(-3, 4, dtype=np.int64), "agent/wide/float64": rng.normal(size=(2, 3, 5)),
         "agent/reward_scale": np.array([2.0], np.float32)}
    t["agent/main/actor/0/dense/bias"][:3] = [np.nan, -0.0, np.inf]                            # bit patterns, not values
    for i in range(40):                                                                       # more entries than one restart interval of the table block
        t["agent/many/v%02d" % i] = np.full(i % 5, i, np.float32)
    return t


def test_round_trip_bits_and_checksums(tmp_path):
    prefix = str(tmp_path / "sub" / "model.ckpt")
    t = _tensors()
    tfc.write_checkpoint(prefix, t)
    assert sorted(os.listdir(tmp_path / "sub")) == ["model.ckpt.data-00000-of-00001", "model.ckpt.index"]
    idx = tfc.read_index(prefix + ".index")                     # (verifies the CRC of every table block)
    assert idx[""]["num_shards"] == 1 and sorted(n for n in idx if n) == sorted(t)
    pos = 0
    for n in sorted(t):                                         # back to back in name order, as the Saver lays them out
        e = idx[n]
        assert e["offset"] == pos and e["size"] == t[n].nbytes and e["shape"] == list(t[n].shape) and tfc.DTYPES[e["dtype"]] == t[n].dtype.type
        assert e["crc32c"] == tfc.masked_crc32c(t[n].tobytes())
        pos += e["size"]
    assert os.path.getsize(prefix + ".data-00000-of-00001") == pos
    back = tfc.read_tensors(prefix, verify_below=None)         # every tensor's CRC verified
    for n, a in t.items():
        assert back[n].dtype == a.dtype and back[n].shape == a.shape and back[n].tobytes() == a.tobytes(), n


def test_corruption_is_refused(tmp_path):
    prefix = str(tmp_path / "model.ckpt")
    t = _tensors(1)
    tfc.write_checkpoint(prefix, t)
    data = prefix + ".data-00000-of-00001"
    raw = open(data, "rb").read()
    # a truncated data shard: the last tensor in name order loses bytes
    open(data, "wb").write(raw[:-5])
    with pytest.raises(ValueError, match="bytes for shape"):
        tfc.read_tensors(prefix)
    # a flipped bit in a small tensor: its checksum
    flipped = bytearray(raw); flipped[tfc.read_index(prefix + ".index")["agent/reward_scale"]["offset"]] ^= 1
    open(data, "wb").write(bytes(flipped))
    with pytest.raises(ValueError, match="agent/reward_scale: checksum mismatch"):
        tfc.read_tensors(prefix)
    open(data, "wb").write(raw)
    tfc.read_tensors(prefix)
    # a flipped bit in the index: the table block's checksum
    ib = bytearray(open(prefix + ".index", "rb").read()); ib[10] ^= 1
    open(prefix + ".index", "wb").write(bytes(ib))
    with pytest.raises(ValueError, match="checksum mismatch"):
        tfc.read_index(prefix + ".index")


def test_writer_refuses_what_the_format_cannot_hold(tmp_path):
    with pytest.raises(ValueError, match="unsupported dtype float16"):
        tfc.write_checkpoint(str(tmp_path / "a"), {"x": np.zeros(2, np.float16)})
    with pytest.raises(ValueError, match="no tensors"):
        tfc.write_checkpoint(str(tmp_path / "a"), {})


@pytest.mark.parametrize("kind", ["ppo", "amp", "amp_task"])
def test_variable_set_is_the_shipped_checkpoints(kind, tmp_path):
    """the names, shapes and dtypes save_model emits (agent_variables, for the sizes the fixture itself states) are the shipped checkpoint's, and a checkpoint
    written with them indexes like it: same offsets and sizes"""
    fix = json.load(open(os.path.join(GOLDEN, "ckpt_names_%s.json" % kind)))
    want = {name: (np.dtype(dtype), tuple(shape)) for name, dtype, shape in fix["variables"]}
    size = lambda res: want["agent/resource/%s/mean" % res][1][0] if "agent/resource/%s/mean" % res in want else 0
    S, G, A, AMP = size("s_norm"), size("g_norm"), size("a_norm"), size("amp_obs_norm")
    assert (kind == "ppo") == (AMP == 0) and (kind == "amp_task") == (G > 0)
    got = tfc.agent_variables(S, G, A, AMP, gated=kind == "amp_task", reward_scale=kind != "ppo")
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    assert got == want, [n for n in want if got[n] != want[n]]
    prefix = str(tmp_path / "m.ckpt")
    tfc.write_checkpoint(prefix, {n: np.zeros(shape, dt) for n, (dt, shape) in got.items()})
    idx = tfc.read_index(prefix + ".index")
    pos = 0
    for name, dtype, shape in sorted(fix["variables"]):
        e = idx[name]
        assert e["shape"] == shape and np.dtype(tfc.DTYPES[e["dtype"]]).name == dtype and e["offset"] == pos
        pos += e["size"]
