"""deepmimic_amd/tf_checkpoint.py critic_weights / disc_weights: the critic (plain and gated) and the AMP discriminator of a reference checkpoint for the
device heads (deepmimic_amd/heads.py), with the variable names the shipped .index files carry."""
import glob
import os

import numpy as np
import pytest

from deepmimic_amd import heads
from deepmimic_amd import tf_checkpoint as tfc
from deepmimic_amd.policy import GATE_KEYS, random_weights
from test_tf_checkpoint import REF_POLICIES, _agent_tensors, write_checkpoint


def _head_tensors(S, G, amp, gated, seed):
    """an agent's tensors in the reference's names: actor (test_tf_checkpoint), critic under agent/main/critic, discriminator under agent/main/disc"""
    t = _agent_tensors(S, 12, G, seed=seed)
    rng = np.random.default_rng(seed + 3)
    c = random_weights(S + G, 1, seed=seed + 4, init_output_scale=1.0, gated_goal_dim=G if gated else 0)
    for i, (wk, bk) in enumerate((("w1", "b1"), ("w2", "b2"))):
        t["agent/main/critic/%d/dense/kernel" % i] = c[wk]; t["agent/main/critic/%d/dense/bias" % i] = (0.1 * rng.normal(size=c[bk].shape)).astype(np.float32)
    t["agent/main/critic/dense/kernel"] = c["w3"]; t["agent/main/critic/dense/bias"] = np.array([0.25], np.float32)
    if gated:
        for key, var in tfc.GATE_VARIABLES.items():
            t["agent/main/critic/%s/kernel" % var] = c[key + "_w"]
            t["agent/main/critic/%s/bias" % var] = (0.1 * rng.normal(size=c[key + "_b"].shape)).astype(np.float32)
    if amp:
        d = random_weights(amp, 1, seed=seed + 5, init_output_scale=1.0)
        for i, (wk, bk) in enumerate((("w1", "b1"), ("w2", "b2"))):
            t["agent/main/disc/%d/dense/kernel" % i] = d[wk]; t["agent/main/disc/%d/dense/bias" % i] = (0.1 * rng.normal(size=d[bk].shape)).astype(np.float32)
        t["agent/main/disc/disc_logits/kernel"] = d["w3"]; t["agent/main/disc/disc_logits/bias"] = np.array([-0.5], np.float32)
        t["agent/resource/amp_obs_norm/mean"] = rng.normal(size=amp).astype(np.float32); t["agent/resource/amp_obs_norm/std"] = (0.5 + rng.random(amp)).astype(np.float32)
    return t


def test_plain_critic_round_trip_drives_the_device_head(emu_lib, tmp_path):
    S = 197
    t = _head_tensors(S, 0, 0, False, seed=3)
    prefix = str(tmp_path / "plain.ckpt")
    write_checkpoint(prefix, t)
    w = tfc.critic_weights(prefix, state_dim=S)
    assert not tfc.is_gated_critic(prefix) and "goal_dim" not in w and "g_mean" not in w
    for k, n in dict(w1="critic/0/dense/kernel", b1="critic/0/dense/bias", w2="critic/1/dense/kernel", b2="critic/1/dense/bias", w3="critic/dense/kernel",
                     b3="critic/dense/bias").items():
        assert np.array_equal(w[k], t["agent/main/" + n]), k
    assert np.array_equal(w["s_mean"], t["agent/resource/s_norm/mean"]) and np.array_equal(w["s_std"], t["agent/resource/s_norm/std"]) and w["w3"].shape == (512, 1)
    crit = heads.Critic.from_checkpoint(prefix, state_dim=S, lib_path=emu_lib)
    x = np.random.default_rng(5).normal(size=(33, S)).astype(np.float32)
    v, y = crit.eval_host(x)
    ref = heads.reference_forward(w, x, bf16=True)
    assert np.abs(y - ref).max() < 2e-3 * max(1.0, np.abs(ref).max()) and np.array_equal(v, y)
    crit.close()
    with pytest.raises(ValueError, match="state features"):
        tfc.critic_weights(prefix, state_dim=S + 1)
    with pytest.raises(ValueError, match="disc"):
        tfc.disc_weights(prefix)


def test_gated_critic_with_a_goal(emu_lib, tmp_path):
    S, G = 226, 3
    t = _head_tensors(S, G, 0, True, seed=4)
    prefix = str(tmp_path / "task.ckpt")
    write_checkpoint(prefix, t)
    assert tfc.is_gated_critic(prefix)
    w = tfc.critic_weights(prefix, state_dim=S)
    assert w["goal_dim"] == G and np.array_equal(w["g_mean"], t["agent/resource/g_norm/mean"]) and np.array_equal(w["g_std"], t["agent/resource/g_norm/std"])
    for key, var in tfc.GATE_VARIABLES.items():
        assert np.array_equal(w[key + "_w"], t["agent/main/critic/%s/kernel" % var]) and np.array_equal(w[key + "_b"], t["agent/main/critic/%s/bias" % var]), key
    assert set(GATE_KEYS) <= set(w) and w["w1"].shape[0] == S + G
    crit = heads.Critic.from_checkpoint(prefix, state_dim=S, lib_path=emu_lib)
    assert crit.gated and crit.info()["net"]["goal_dim"] == G
    rng = np.random.default_rng(5)
    s = rng.normal(size=(33, S)).astype(np.float32); g = rng.normal(size=(33, G)).astype(np.float32)
    _, y = crit.eval_host(s, g)
    w_cat = dict(w); w_cat["s_mean"] = np.concatenate([w["s_mean"], w["g_mean"]]); w_cat["s_std"] = np.concatenate([w["s_std"], w["g_std"]])
    ref = heads.reference_forward(w_cat, np.concatenate([s, g], axis=1), bf16=True)
    assert np.abs(y - ref).max() < 2e-3 * max(1.0, np.abs(ref).max())
    plain = heads.reference_forward({k: v for k, v in w_cat.items() if k not in GATE_KEYS}, np.concatenate([s, g], axis=1), bf16=True)
    assert np.abs(plain - ref).max() > 1e-2          # the gate is in it
    crit.close()


def test_discriminator_with_amp_obs_norm(emu_lib, tmp_path):
    S, AMP = 197, 226
    t = _head_tensors(S, 0, AMP, False, seed=6)
    prefix = str(tmp_path / "amp.ckpt")
    write_checkpoint(prefix, t)
    w = tfc.disc_weights(prefix)
    for k, n in dict(w1="disc/0/dense/kernel", b1="disc/0/dense/bias", w2="disc/1/dense/kernel", b2="disc/1/dense/bias", w3="disc/disc_logits/kernel",
                     b3="disc/disc_logits/bias").items():
        assert np.array_equal(w[k], t["agent/main/" + n]), k
    assert np.array_equal(w["s_mean"], t["agent/resource/amp_obs_norm/mean"]) and np.array_equal(w["s_std"], t["agent/resource/amp_obs_norm/std"])
    assert w["w1"].shape[0] == AMP and "g_mean" not in w
    disc = heads.Discriminator.from_checkpoint(prefix, reward_scale=2.0, lib_path=emu_lib)
    x = np.random.default_rng(7).normal(size=(33, AMP)).astype(np.float32)
    r, y = disc.eval_host(x)
    ref = heads.reference_forward(w, x, bf16=True)
    assert np.abs(y - ref).max() < 2e-3 * max(1.0, np.abs(ref).max())
    assert np.abs(r - heads.reference_style_reward(y.astype(np.float64), 2.0)).max() < 1e-6 and (r > 0).any()
    disc.close()


@pytest.mark.skipif(not os.path.isdir(REF_POLICIES), reason="needs the reference checkout (data/policies/*.ckpt.index)")
def test_every_shipped_index_maps_its_critic_and_discriminator():
    """no variable critic_weights / disc_weights need is missing from a shipped index (the calls end in FileNotFoundError: the .data blobs are not shipped);
    critic input width = state + goal size, discriminator input width = amp_obs_norm width"""
    files = sorted(glob.glob(os.path.join(REF_POLICIES, "*", "*.ckpt.index")))
    assert len(files) >= 40
    gated = discs = 0
    for f in files:
        prefix = f[:-len(".index")]
        idx = tfc.read_index(f)
        sh = lambda n: idx[n]["shape"]
        with pytest.raises(FileNotFoundError):
            tfc.critic_weights(prefix)
        S, G = sh("agent/resource/s_norm/mean")[0], sh("agent/resource/g_norm/mean")[0]
        assert sh("agent/main/critic/0/dense/kernel")[0] == S + G and sh("agent/main/critic/dense/kernel") == [sh("agent/main/critic/1/dense/kernel")[1], 1], f
        if tfc.is_gated_critic(prefix):
            gated += 1
            assert G >= 1 and sh("agent/main/critic/gate_common/0/dense/kernel")[0] == G, f
            assert sorted(n for n in idx if n.startswith("agent/main/critic/gate")) == sorted(
                "agent/main/critic/%s/%s" % (v, k) for v in tfc.GATE_VARIABLES.values() for k in ("bias", "kernel")), f
        if any(n.startswith("agent/main/disc/") for n in idx):
            discs += 1
            with pytest.raises(FileNotFoundError):
                tfc.disc_weights(prefix)
            assert sh("agent/main/disc/0/dense/kernel")[0] == sh("agent/resource/amp_obs_norm/mean")[0] and sh("agent/main/disc/disc_logits/kernel")[1] == 1, f
        else:
            with pytest.raises(ValueError):
                tfc.disc_weights(prefix)
    assert gated >= 5 and discs >= 5
