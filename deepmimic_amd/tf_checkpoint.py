"""Reader for the reference's policy checkpoints (`--model_files data/policies/...ckpt`: learning/rl_world.py:67-85 -> learning/tf_agent.py:36-48, a
`tf.train.Saver` V2 checkpoint) into the on-device actor of `deepmimic_amd.policy` -- without TensorFlow.

A V2 checkpoint is two files.  `<prefix>.index` is an uncompressed leveldb-format sorted table (blocks of prefix-compressed keys with restart arrays, a 5-byte
block trailer, a 48-byte footer ending in the magic 0xdb4775248b80fb57) whose keys are variable names and whose values are `BundleEntryProto` messages
(dtype, shape, shard, offset, size, masked crc32c); the empty key holds the `BundleHeaderProto`.  `<prefix>.data-0000k-of-0000n` holds the tensors raw,
little-endian, at those offsets.  The reference checkout ships the 52 `.index` files of its pretrained policies (the `.data` blobs are not in the repository):
`read_index` is tested on all of them, `read_tensors` / `actor_weights` on checkpoints written by the test suite's own writer in the same format.

Variables of an agent (learning/pg_agent.py:141-188, learning/nets/fc_2layers_1024units.py, learning/rl_agent.py normalizers), scope `agent`:
    agent/main/actor/0/dense/{kernel,bias}  [S + G, 1024]      agent/main/actor/1/dense/{kernel,bias}  [1024, 512]
    agent/main/actor/dist_gauss_diag/mean/{kernel,bias}  [512, A]      agent/main/actor/dist_gauss_diag/logstd/bias  [A]
    agent/resource/{s_norm,g_norm,a_norm}/{mean,std}
The AMP task policies use the gated net (learning/nets/fc_2layers_gated_1024units.py: `gate0`, `gate1`, `gate_common` variables): `gated_actor_weights`
reads those for the gated device actor; `actor_weights`, which returns the plain net's dict, refuses them and says so."""
import os
import struct
from typing import Dict, Optional

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 9: np.int64}       # tensorflow/core/framework/types.proto: DT_FLOAT, DT_DOUBLE, DT_INT32, DT_INT64


def _varint(b: bytes, i: int):
    r = s = 0
    while True:
        c = b[i]; i += 1
        r |= (c & 0x7f) << s; s += 7
        if c < 0x80:
            return r, i


def _block(b: bytes, off: int, size: int):
    """entries of one table block: shared-prefix length, unshared length, value length (varints), key suffix, value; restart array + count at the end"""
    if b[off + size] != 0:
        raise ValueError("compressed table block (type %d): tf.train.Saver writes the index uncompressed" % b[off + size])
    if masked_crc32c(b[off:off + size + 1]) != struct.unpack("<I", b[off + size + 1:off + size + 5])[0]:
        raise ValueError("table block at %d: checksum mismatch" % off)
    blk = b[off:off + size]
    n_restarts = struct.unpack("<I", blk[-4:])[0]
    end = len(blk) - 4 - 4 * n_restarts
    i, key, out = 0, b"", []
    while i < end:
        shared, i = _varint(blk, i); unshared, i = _varint(blk, i); vlen, i = _varint(blk, i)
        key = key[:shared] + blk[i:i + unshared]; i += unshared
        out.append((key, blk[i:i + vlen])); i += vlen
    return out


def _handle(b: bytes, i: int):
    off, i = _varint(b, i); size, i = _varint(b, i)
    return (off, size), i


def _entry(v: bytes) -> dict:
    """BundleEntryProto (tensorflow/core/protobuf/tensor_bundle.proto): 1 dtype, 2 shape {2 dim {1 size}}, 3 shard_id, 4 offset, 5 size, 6 crc32c (fixed32)"""
    e = {"dtype": 0, "shape": [], "shard": 0, "offset": 0, "size": 0, "crc32c": None}
    i = 0
    while i < len(v):
        tag, i = _varint(v, i)
        field, wire = tag >> 3, tag & 7
        if wire == 0:
            x, i = _varint(v, i)
        elif wire == 5:
            x = struct.unpack("<I", v[i:i + 4])[0]; i += 4
        elif wire == 2:
            n, i = _varint(v, i); x = v[i:i + n]; i += n
        elif wire == 1:
            x = v[i:i + 8]; i += 8
        else:
            raise ValueError("unsupported protobuf wire type %d in a bundle entry" % wire)
        if field == 1:
            e["dtype"] = x
        elif field == 2:
            j = 0
            while j < len(x):
                t2, j = _varint(x, j)
                if t2 & 7 != 2:
                    _, j = _varint(x, j); continue          # unknown_rank and the like
                n2, j = _varint(x, j); dim = x[j:j + n2]; j += n2
                if t2 >> 3 == 2:
                    k, dsize = 0, 0                             # (proto3 omits a zero: an empty dim message is a dimension of size 0 -- g_norm of an agent without a goal)
                    while k < len(dim):
                        t3, k = _varint(dim, k)
                        if t3 & 7 == 0:
                            val, k = _varint(dim, k)
                            if t3 >> 3 == 1:
                                dsize = val
                        else:
                            n3, k = _varint(dim, k); k += n3    # dim name
                    e["shape"].append(dsize)
        elif field == 3:
            e["shard"] = x
        elif field == 4:
            e["offset"] = x
        elif field == 5:
            e["size"] = x
        elif field == 6:
            e["crc32c"] = x
    return e


def read_index(path: str) -> Dict[str, dict]:
    """`<prefix>.index` -> {variable name: {dtype, shape, shard, offset, size, crc32c}}; key "" holds {"num_shards": n}"""
    b = open(path, "rb").read()
    if len(b) < 48 or struct.unpack("<Q", b[-8:])[0] != TABLE_MAGIC:
        raise ValueError("%s is not a tensor-bundle index (table magic missing)" % path)
    foot = b[-48:]
    _, i = _handle(foot, 0)                    # metaindex block (empty)
    (ioff, isize), _ = _handle(foot, i)
    out = {}
    for _, hv in _block(b, ioff, isize):       # index block: one handle per data block
        (doff, dsize), _ = _handle(hv, 0)
        for key, val in _block(b, doff, dsize):
            if key == b"":                      # BundleHeaderProto: 1 num_shards, 2 endianness (0 little), 3 version
                hdr, i2 = {"num_shards": 1, "endianness": 0}, 0
                while i2 < len(val):
                    tag, i2 = _varint(val, i2)
                    if tag & 7 == 0:
                        x, i2 = _varint(val, i2)
                        if tag >> 3 == 1:
                            hdr["num_shards"] = x
                        elif tag >> 3 == 2:
                            hdr["endianness"] = x
                    else:
                        n, i2 = _varint(val, i2); i2 += n
                if hdr["endianness"] != 0:
                    raise ValueError("big-endian tensor bundle")
                out[""] = hdr
            else:
                out[key.decode()] = _entry(val)
    return out


_CRC_TABLE = None


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli), the checksum of the table blocks and of every tensor"""
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = []
        for n in range(256):
            c = n
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            t.append(c)
        _CRC_TABLE = t
    t, c = _CRC_TABLE, 0xFFFFFFFF
    for byte in data:
        c = t[(c ^ byte) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    """how the bundle stores it (tensorflow/core/lib/hash/crc32c.h Mask): rotate right by 15, add a constant"""
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def read_tensors(prefix: str, names=None, verify_below: int = 1 << 16) -> Dict[str, np.ndarray]:
    """tensors of `<prefix>.index` + `<prefix>.data-*`; checksums are verified for tensors up to `verify_below` bytes (all of them with verify_below=None:
    a pure-Python CRC, seconds per megabyte)"""
    idx = read_index(prefix + ".index")
    shards = idx[""]["num_shards"]
    files = {}
    out = {}
    for name, e in idx.items():
        if name == "" or (names is not None and name not in names):
            continue
        if e["dtype"] not in DTYPES:
            raise ValueError("%s: unsupported dtype %d" % (name, e["dtype"]))
        if e["shard"] not in files:
            p = "%s.data-%05d-of-%05d" % (prefix, e["shard"], shards)
            if not os.path.exists(p):
                raise FileNotFoundError("%s (the tensor data of the checkpoint; the reference repository ships the .index files only)" % p)
            files[e["shard"]] = open(p, "rb")
        f = files[e["shard"]]
        f.seek(e["offset"]); raw = f.read(e["size"])
        dt = np.dtype(DTYPES[e["dtype"]])
        if len(raw) != e["size"] or e["size"] != int(np.prod(e["shape"], dtype=np.int64)) * dt.itemsize:
            raise ValueError("%s: %d bytes for shape %s" % (name, len(raw), e["shape"]))
        if e["crc32c"] is not None and (verify_below is None or e["size"] <= verify_below) and masked_crc32c(raw) != e["crc32c"]:
            raise ValueError("%s: checksum mismatch" % name)
        out[name] = np.frombuffer(raw, dtype=dt.newbyteorder("<")).reshape(e["shape"]).astype(dt)
    for f in files.values():
        f.close()
    return out


def actor_weights(prefix: str, scope: str = "agent", state_dim: Optional[int] = None, verify_below: int = 1 << 16) -> dict:
    """The actor of a reference checkpoint as the weights dict of `deepmimic_amd.policy.Policy`: w1 b1 w2 b2 w3 b3 logstd s_mean s_std a_mean a_std (+ g_mean,
    g_std when the agent has a goal: the first layer then takes [state, goal], learning/pg_agent.py:141-146).  `state_dim`: checked against s_norm when given."""
    idx = read_index(prefix + ".index")
    a = scope + "/main/actor/"
    gated = sorted(n for n in idx if n.startswith(a + "gate"))
    if gated:
        raise NotImplementedError("%s holds a gated actor (learning/nets/fc_2layers_gated_1024units.py: %s, ...); actor_weights returns the plain fc_2layers_1024units "
                                  "net's dict: read it with gated_actor_weights (Policy.from_checkpoint picks the mapper by itself)" % (prefix, gated[0]))
    return _actor_weights(idx, prefix, scope, state_dim, verify_below, {})


# key of the weights dict of deepmimic_amd.policy (GATE_KEYS) -> variable under <scope>/main/actor/, as tf.layers.dense names them in the shipped gated
# checkpoints (data/policies/humanoid3d_amp/*.ckpt.index: the first dense of a scope is `dense`, the second `dense_1`; tests/test_tf_checkpoint_gated.py
# holds this table to every shipped index)
GATE_VARIABLES = {"gc": "gate_common/0/dense", "g0": "gate0/0/dense", "g0_bias": "gate0/dense", "g0_scale": "gate0/dense_1",
                  "g1": "gate1/0/dense", "g1_bias": "gate1/dense", "g1_scale": "gate1/dense_1"}


def is_gated_checkpoint(prefix: str, scope: str = "agent") -> bool:
    return any(n.startswith(scope + "/main/actor/gate") for n in read_index(prefix + ".index"))


def gated_actor_weights(prefix: str, scope: str = "agent", state_dim: Optional[int] = None, verify_below: int = 1 << 16) -> dict:
    """The gated actor of an AMP task checkpoint ("ActorNet": "fc_2layers_gated_1024units") as the weights dict of `deepmimic_amd.policy.Policy`: what
    actor_weights returns plus the gate arrays (policy.GATE_KEYS) and goal_dim, the width of g_norm -- the gate's input is the normalised goal."""
    idx = read_index(prefix + ".index")
    a = scope + "/main/actor/"
    extra = {}
    for key, var in GATE_VARIABLES.items():
        extra[key + "_w"] = a + var + "/kernel"; extra[key + "_b"] = a + var + "/bias"
    missing = [n for n in extra.values() if n not in idx]
    if missing:
        raise ValueError("%s: no %s (not a gated actor; plain ones are read by actor_weights)" % (prefix, missing[0]))
    w = _actor_weights(idx, prefix, scope, state_dim, verify_below, extra)
    G = w["g_mean"].size if "g_mean" in w else 0
    if G < 1 or w["gc_w"].shape[0] != G:
        raise ValueError("%s: the gate takes %d inputs, g_norm has %d" % (prefix, w["gc_w"].shape[0], G))
    GC, GH = w["gc_w"].shape[1], w["g0_w"].shape[1]
    for i, H in ((0, w["w1"].shape[1]), (1, w["w2"].shape[1])):
        if w["g%d_w" % i].shape != (GC, GH) or w["g%d_bias_w" % i].shape != (GH, H) or w["g%d_scale_w" % i].shape != (GH, H):
            raise ValueError("%s: gate %d shapes %s %s %s do not chain from %d to %d" % (prefix, i, w["g%d_w" % i].shape, w["g%d_bias_w" % i].shape, w["g%d_scale_w" % i].shape, GC, H))
    w["goal_dim"] = G
    return w


def _actor_weights(idx, prefix, scope, state_dim, verify_below, extra) -> dict:
    a = scope + "/main/actor/"
    need = [a + "0/dense/kernel", a + "0/dense/bias", a + "1/dense/kernel", a + "1/dense/bias", a + "dist_gauss_diag/mean/kernel", a + "dist_gauss_diag/mean/bias",
            a + "dist_gauss_diag/logstd/bias"]
    missing = [n for n in need if n not in idx]
    if missing:
        raise ValueError("%s: no %s (not a pg / ppo agent checkpoint of scope %r)" % (prefix, missing[0], scope))
    norms = [scope + "/resource/%s/%s" % (g, k) for g in ("s_norm", "g_norm", "a_norm") for k in ("mean", "std")]
    t = read_tensors(prefix, names=set(need + list(extra.values()) + [n for n in norms if n in idx]), verify_below=verify_below)
    w = dict(w1=t[need[0]], b1=t[need[1]], w2=t[need[2]], b2=t[need[3]], w3=t[need[4]], b3=t[need[5]], logstd=t[need[6]])
    for k, n in extra.items():
        w[k] = t[n]
    for g, key in (("s_norm", "s"), ("g_norm", "g"), ("a_norm", "a")):
        for k in ("mean", "std"):
            n = scope + "/resource/%s/%s" % (g, k)
            if n in t and t[n].size:
                w["%s_%s" % (key, k)] = t[n].reshape(-1)
    S = w["s_mean"].size if "s_mean" in w else w["w1"].shape[0]
    G = w["g_mean"].size if "g_mean" in w else 0
    if state_dim is not None and S != state_dim:
        raise ValueError("%s was trained on %d state features, the scene records %d" % (prefix, S, state_dim))
    if w["w1"].shape[0] != S + G or w["w2"].shape[0] != w["w1"].shape[1] or w["w3"].shape[0] != w["w2"].shape[1] or w["logstd"].size != w["w3"].shape[1]:
        raise ValueError("%s: layer shapes %s %s %s do not chain from %d + %d inputs" % (prefix, w["w1"].shape, w["w2"].shape, w["w3"].shape, S, G))
    return w


def _mlp_weights(idx, prefix, base, out_layer, norms, verify_below, extra) -> dict:
    """a two-layer net with a linear output under `base` (0/dense, 1/dense, <out_layer>) plus the normalisers `norms` ((resource group, key prefix), ...)"""
    need = [base + "0/dense/kernel", base + "0/dense/bias", base + "1/dense/kernel", base + "1/dense/bias", base + out_layer + "/kernel", base + out_layer + "/bias"]
    missing = [n for n in need + list(extra.values()) if n not in idx]
    if missing:
        raise ValueError("%s: no %s" % (prefix, missing[0]))
    scope = base.split("/main/")[0]
    nn = [scope + "/resource/%s/%s" % (g, k) for g, _ in norms for k in ("mean", "std")]
    t = read_tensors(prefix, names=set(need + list(extra.values()) + [n for n in nn if n in idx]), verify_below=verify_below)
    w = dict(w1=t[need[0]], b1=t[need[1]], w2=t[need[2]], b2=t[need[3]], w3=t[need[4]], b3=t[need[5]])
    for k, n in extra.items():
        w[k] = t[n]
    for g, key in norms:
        for k in ("mean", "std"):
            n = scope + "/resource/%s/%s" % (g, k)
            if n in t and t[n].size:
                w["%s_%s" % (key, k)] = t[n].reshape(-1)
    if w["w2"].shape[0] != w["w1"].shape[1] or w["w3"].shape != (w["w2"].shape[1], 1) or w["b3"].shape != (1,):
        raise ValueError("%s: layer shapes %s %s %s under %s do not chain to one output" % (prefix, w["w1"].shape, w["w2"].shape, w["w3"].shape, base))
    return w


def is_gated_critic(prefix: str, scope: str = "agent") -> bool:
    return any(n.startswith(scope + "/main/critic/gate") for n in read_index(prefix + ".index"))


def critic_weights(prefix: str, scope: str = "agent", state_dim: Optional[int] = None, verify_below: int = 1 << 16) -> dict:
    """The critic of a reference checkpoint (<scope>/main/critic/{0,1}/dense and the one-unit `dense`, learning/pg_agent.py:161-171) as the weights dict of
    `deepmimic_amd.heads.Critic`: w1 b1 w2 b2 w3 [H2, 1] b3 [1], s_mean s_std (+ g_mean g_std with a goal: the net reads [norm_s, norm_g]); with
    <scope>/main/critic/gate* variables ("CriticNet": "fc_2layers_gated_1024units", the AMP task agents) also the gate arrays (policy.GATE_KEYS) and goal_dim."""
    idx = read_index(prefix + ".index")
    c = scope + "/main/critic/"
    extra = {}
    if is_gated_critic(prefix, scope):
        for key, var in GATE_VARIABLES.items():
            extra[key + "_w"] = c + var + "/kernel"; extra[key + "_b"] = c + var + "/bias"
    w = _mlp_weights(idx, prefix, c, "dense", (("s_norm", "s"), ("g_norm", "g")), verify_below, extra)
    S = w["s_mean"].size if "s_mean" in w else w["w1"].shape[0]
    G = w["g_mean"].size if "g_mean" in w else 0
    if state_dim is not None and S != state_dim:
        raise ValueError("%s was trained on %d state features, the scene records %d" % (prefix, S, state_dim))
    if w["w1"].shape[0] != S + G:
        raise ValueError("%s: the critic takes %d inputs, s_norm + g_norm have %d + %d" % (prefix, w["w1"].shape[0], S, G))
    if extra:
        if G < 1 or w["gc_w"].shape[0] != G:
            raise ValueError("%s: the critic's gate takes %d inputs, g_norm has %d" % (prefix, w["gc_w"].shape[0], G))
        w["goal_dim"] = G
    return w


def disc_weights(prefix: str, scope: str = "agent", verify_below: int = 1 << 16) -> dict:
    """The AMP discriminator of a reference checkpoint (<scope>/main/disc/{0,1}/dense and `disc_logits`, learning/amp_agent.py:178-194) as the weights dict of
    `deepmimic_amd.heads.Discriminator`, with <scope>/resource/amp_obs_norm as its input normaliser (s_mean, s_std)."""
    idx = read_index(prefix + ".index")
    w = _mlp_weights(idx, prefix, scope + "/main/disc/", "disc_logits", (("amp_obs_norm", "s"),), verify_below, {})
    if "s_mean" in w and w["s_mean"].size != w["w1"].shape[0]:
        raise ValueError("%s: the discriminator takes %d inputs, amp_obs_norm has %d" % (prefix, w["w1"].shape[0], w["s_mean"].size))
    return w
