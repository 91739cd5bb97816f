"""deepmimic_amd/tf_checkpoint.py gated_actor_weights: the gated actor of the AMP task checkpoints ("ActorNet": "fc_2layers_gated_1024units") for the device
actor, with the variable names the shipped gated .index files carry."""
import glob
import os

import numpy as np
import pytest

from deepmimic_amd import tf_checkpoint as tfc
from deepmimic_amd.policy import GATE_KEYS, Policy, random_weights, reference_forward
from test_tf_checkpoint import REF_POLICIES, _agent_tensors, write_checkpoint

# <scope>/main/actor/... of every gate variable, read once from data/policies/humanoid3d_amp/humanoid3d_amp_heading_zombie.ckpt.index with
# tf_checkpoint.read_index (test_every_shipped_gated_index holds GATE_VARIABLES to all shipped files); shapes there: G = 3, 128, 64, 1024 / 512
SHIPPED_GATE_NAMES = ["gate0/0/dense/bias", "gate0/0/dense/kernel", "gate0/dense/bias", "gate0/dense/kernel", "gate0/dense_1/bias", "gate0/dense_1/kernel",
                      "gate1/0/dense/bias", "gate1/0/dense/kernel", "gate1/dense/bias", "gate1/dense/kernel", "gate1/dense_1/bias", "gate1/dense_1/kernel",
                      "gate_common/0/dense/bias", "gate_common/0/dense/kernel"]


def test_mapper_uses_the_shipped_names():
    mine = sorted("%s/%s" % (v, k) for v in tfc.GATE_VARIABLES.values() for k in ("bias", "kernel"))
    assert mine == sorted(SHIPPED_GATE_NAMES)
    assert sorted(k + s for k in tfc.GATE_VARIABLES for s in ("_w", "_b")) == sorted(GATE_KEYS)


def _gated_tensors(S, A, G, seed):
    t = _agent_tensors(S, A, G, seed=seed)
    g = random_weights(S + G, A, seed=seed + 7, gated_goal_dim=G)
    rng = np.random.default_rng(seed + 9)
    for key, var in tfc.GATE_VARIABLES.items():
        t["agent/main/actor/%s/kernel" % var] = g[key + "_w"]
        t["agent/main/actor/%s/bias" % var] = (0.1 * rng.normal(size=g[key + "_b"].shape)).astype(np.float32)
    return t


def test_gated_checkpoint_drives_the_device_actor(emu_lib, tmp_path, monkeypatch):
    """checkpoint -> Policy.from_checkpoint -> gated kernels: the mode action equals the numpy statement on the tensors written"""
    monkeypatch.setenv("DM_ALLOW_EMULATOR", "1")
    S, G, A = 226, 3, 28
    t = _gated_tensors(S, A, G, seed=3)
    prefix = str(tmp_path / "task.ckpt")
    write_checkpoint(prefix, t)
    assert tfc.is_gated_checkpoint(prefix)
    with pytest.raises(NotImplementedError, match="gated_actor_weights"):
        tfc.actor_weights(prefix)
    w = tfc.gated_actor_weights(prefix, state_dim=S)
    assert w["goal_dim"] == G and np.array_equal(w["g0_scale_w"], t["agent/main/actor/gate0/dense_1/kernel"]) and np.array_equal(w["g1_bias_b"], t["agent/main/actor/gate1/dense/bias"])
    assert np.array_equal(w["gc_w"], t["agent/main/actor/gate_common/0/dense/kernel"]) and np.array_equal(w["g1_w"], t["agent/main/actor/gate1/0/dense/kernel"])
    pol = Policy.from_checkpoint(prefix, state_dim=S, lib_path=emu_lib)
    info = pol.info()
    assert info["gated"] and info["goal_dim"] == G
    rng = np.random.default_rng(5)
    s = rng.normal(size=(33, S)).astype(np.float32); g = rng.normal(size=(33, G)).astype(np.float32)
    a, _, _ = pol.forward_host_ex(s, g)
    w_cat = dict(w); w_cat["s_mean"] = np.concatenate([w["s_mean"], w["g_mean"]]); w_cat["s_std"] = np.concatenate([w["s_std"], w["g_std"]])
    ref, _ = reference_forward(w_cat, np.concatenate([s, g], axis=1), bf16=True)
    assert np.abs(a - ref).max() < 2e-3 * max(1.0, np.abs(ref).max())
    # the gate is in it: the plain statement on the same main weights is something else
    plain, _ = reference_forward({k: v for k, v in w_cat.items() if k not in GATE_KEYS}, np.concatenate([s, g], axis=1), bf16=True)
    assert np.abs(plain - ref).max() > 1e-2
    with pytest.raises(ValueError, match="state features"):
        tfc.gated_actor_weights(prefix, state_dim=S + 1)
    # a plain checkpoint still takes the plain mapper, and the gated one says what is missing
    plain_prefix = str(tmp_path / "plain.ckpt")
    write_checkpoint(plain_prefix, _agent_tensors(197, 36, seed=4))
    assert not tfc.is_gated_checkpoint(plain_prefix) and not Policy.from_checkpoint(plain_prefix, lib_path=emu_lib).info()["gated"]
    with pytest.raises(ValueError, match="not a gated actor"):
        tfc.gated_actor_weights(plain_prefix)


@pytest.mark.skipif(not os.path.isdir(REF_POLICIES), reason="needs the reference checkout (data/policies/*.ckpt.index)")
def test_every_shipped_gated_index():
    """every tensor gated_actor_weights needs is there with consistent shapes, and the call ends in FileNotFoundError for the absent .data blob"""
    gated = 0
    for f in sorted(glob.glob(os.path.join(REF_POLICIES, "*", "*.ckpt.index"))):
        prefix = f[:-len(".index")]
        if not tfc.is_gated_checkpoint(prefix):
            continue
        gated += 1
        idx = tfc.read_index(f)
        a = "agent/main/actor/"
        assert sorted(n[len(a):] for n in idx if n.startswith(a + "gate")) == sorted(SHIPPED_GATE_NAMES), f
        sh = lambda n: idx[a + n]["shape"]
        G = idx["agent/resource/g_norm/mean"]["shape"][0]
        GC, GH = sh("gate_common/0/dense/kernel")[1], sh("gate0/0/dense/kernel")[1]
        assert sh("gate_common/0/dense/kernel") == [G, GC] and sh("gate_common/0/dense/bias") == [GC] and (GC, GH) == (128, 64) and 1 <= G <= 128
        for i, H in ((0, sh("0/dense/kernel")[1]), (1, sh("1/dense/kernel")[1])):
            assert sh("gate%d/0/dense/kernel" % i) == [GC, GH] and sh("gate%d/0/dense/bias" % i) == [GH]
            for v in ("dense", "dense_1"):
                assert sh("gate%d/%s/kernel" % (i, v)) == [GH, H] and sh("gate%d/%s/bias" % (i, v)) == [H], (f, i, v)
        with pytest.raises(FileNotFoundError):
            tfc.gated_actor_weights(prefix)
    assert gated >= 5
