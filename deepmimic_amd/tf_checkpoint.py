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
reads those for the gated device actor; `actor_weights`, which returns the plain net's dict, refuses them and says so.

`write_checkpoint` is the writer of the same format (what `agent.save_model` calls) and `agent_variables` the variable set of the three kinds of shipped agent checkpoints."""
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


# ---- the writer (the mirror of read_index / read_tensors: one shard, uncompressed table blocks, masked CRC-32C on every block and tensor)

_DTYPE_IDS = {np.dtype(v): k for k, v in DTYPES.items()}


def _put_varint(n: int) -> bytes:
    out = b""
    while True:
        c = n & 0x7f; n >>= 7
        if n:
            out += bytes([c | 0x80])
        else:
            return out + bytes([c])


def _entry_bytes(arr: np.ndarray, offset: int, crc: int) -> bytes:
    """BundleEntryProto of one tensor; proto3 leaves a zero field out (offset 0, a dimension of size 0)"""
    shape = b""
    for d in arr.shape:
        dim = b"\x08" + _put_varint(int(d)) if d else b""
        shape += b"\x12" + _put_varint(len(dim)) + dim
    v = b"\x08" + _put_varint(_DTYPE_IDS[arr.dtype]) + b"\x12" + _put_varint(len(shape)) + shape
    if offset:
        v += b"\x20" + _put_varint(offset)
    if arr.nbytes:
        v += b"\x28" + _put_varint(arr.nbytes)
    return v + b"\x35" + struct.pack("<I", crc)


def _table_block_bytes(entries, restart_interval: int = 16) -> bytes:
    """a leveldb table block: prefix-compressed (key, value) entries, the restart array and its length"""
    out, restarts, prev = b"", [], b""
    for i, (k, v) in enumerate(entries):
        shared = 0
        if i % restart_interval == 0:
            restarts.append(len(out))
        else:
            while shared < min(len(k), len(prev)) and k[shared] == prev[shared]:
                shared += 1
        out += _put_varint(shared) + _put_varint(len(k) - shared) + _put_varint(len(v)) + k[shared:] + v
        prev = k
    restarts = restarts or [0]
    return out + b"".join(struct.pack("<I", r) for r in restarts) + struct.pack("<I", len(restarts))


def write_checkpoint(prefix: str, tensors: Dict[str, np.ndarray]) -> None:
    """`tensors` ({variable name: array of a dtype in DTYPES}) as a one-shard V2 checkpoint in tf.train.Saver's layout: `<prefix>.data-00000-of-00001` holds the
    tensors raw, little-endian, back to back in name order; `<prefix>.index` is the sorted table -- the BundleHeaderProto under the empty key, a BundleEntryProto
    per variable, one data block, an empty metaindex block, the index block, the 48-byte footer -- with the masked CRC-32C of every block and tensor.  What
    read_index / read_tensors read back bit for bit.  Whether TensorFlow's own `saver.restore` accepts the files is not tested here (no TensorFlow)."""
    if not tensors:
        raise ValueError("write_checkpoint: no tensors")
    names = sorted(tensors)
    data, entries = [], [(b"", b"\x08\x01\x1a\x02\x08\x01")]          # BundleHeaderProto: one shard, little endian, version {producer 1}
    pos = 0
    for n in names:
        if not n or not isinstance(n, str):
            raise ValueError("write_checkpoint: variable names are non-empty strings")
        a = np.asarray(tensors[n])
        if a.dtype not in _DTYPE_IDS:
            raise ValueError("%s: unsupported dtype %s" % (n, a.dtype))
        raw = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("<"))).tobytes()
        entries.append((n.encode(), _entry_bytes(a, pos, masked_crc32c(raw))))
        data.append(raw); pos += len(raw)
    blocks, at = [], 0

    def put(block: bytes) -> bytes:
        nonlocal at
        handle = _put_varint(at) + _put_varint(len(block))
        body = block + b"\x00"                                          # block type 0: uncompressed
        blocks.append(body + struct.pack("<I", masked_crc32c(body))); at += len(body) + 4
        return handle
    h_data = put(_table_block_bytes(entries))
    h_meta = put(_table_block_bytes([]))
    h_index = put(_table_block_bytes([(names[-1].encode() + b"\x00", h_data)], 1))
    foot = h_meta + h_index
    foot += b"\x00" * (40 - len(foot)) + struct.pack("<Q", TABLE_MAGIC)
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    with open(prefix + ".data-00000-of-00001", "wb") as f:
        f.write(b"".join(data))
    with open(prefix + ".index", "wb") as f:
        f.write(b"".join(blocks) + foot)


# ---- the variable set of an agent's checkpoint (what agent.save_model writes)

LEGACY_LOGSTD_WIDTH = 36         # agent/main/actor/dist_gauss_diag/logstd/bias_1 (and bias_2): see agent_variables
_GATE_SHAPES = (("gate_common/0/dense", "gc"), ("gate0/0/dense", "g0"), ("gate0/dense", "g0_bias"), ("gate0/dense_1", "g0_scale"),
                ("gate1/0/dense", "g1"), ("gate1/dense", "g1_bias"), ("gate1/dense_1", "g1_scale"))


def agent_variables(S: int, G: int, A: int, amp_size: int = 0, gated: bool = False, reward_scale: bool = False, H1: int = 1024, H2: int = 512,
                    gate_common: int = 128, gate_hidden: int = 64, scope: str = "agent") -> Dict[str, tuple]:
    """{variable name: (numpy dtype, shape)} of the checkpoint of one agent kind, as the shipped checkpoints hold it (data/policies/*/*.ckpt.index):
    plain PPO (amp_size 0), AMP single-clip (amp_size > 0) and the AMP task agents (gated actor and critic, a goal, `reward_scale`).  Every normaliser is
    mean / std / count plus the `_ph` twins of TFNormalizer's assign placeholders; `val_norm` and `logstd/bias_1` (float32 [LEGACY_LOGSTD_WIDTH] on every
    character; the single-clip AMP checkpoints also hold a `bias_2`) are leftovers of the graph the shipped policies were trained with: the current reference
    graph reads none of them, they are listed so that a written checkpoint has the shipped variable set."""
    f32, i32 = np.dtype(np.float32), np.dtype(np.int32)
    v = {}

    def mlp(base, out_name, out_dim, gate):
        v[base + "0/dense/kernel"] = (f32, (S + G, H1)); v[base + "0/dense/bias"] = (f32, (H1,))
        v[base + "1/dense/kernel"] = (f32, (H1, H2)); v[base + "1/dense/bias"] = (f32, (H2,))
        v[base + out_name + "/kernel"] = (f32, (H2, out_dim)); v[base + out_name + "/bias"] = (f32, (out_dim,))
        if gate:
            dims = dict(gc=(G, gate_common), g0=(gate_common, gate_hidden), g0_bias=(gate_hidden, H1), g0_scale=(gate_hidden, H1),
                        g1=(gate_common, gate_hidden), g1_bias=(gate_hidden, H2), g1_scale=(gate_hidden, H2))
            for var, key in _GATE_SHAPES:
                v[base + var + "/kernel"] = (f32, dims[key]); v[base + var + "/bias"] = (f32, (dims[key][1],))
    mlp(scope + "/main/actor/", "dist_gauss_diag/mean", A, gated)
    v[scope + "/main/actor/dist_gauss_diag/logstd/bias"] = (f32, (A,))
    for k in range(2 if (amp_size and not gated) else 1):
        v[scope + "/main/actor/dist_gauss_diag/logstd/bias_%d" % (k + 1)] = (f32, (LEGACY_LOGSTD_WIDTH,))
    mlp(scope + "/main/critic/", "dense", 1, gated)
    norms = [("s_norm", S), ("g_norm", G), ("a_norm", A), ("val_norm", 1)]
    if amp_size:
        v[scope + "/main/disc/0/dense/kernel"] = (f32, (amp_size, H1)); v[scope + "/main/disc/0/dense/bias"] = (f32, (H1,))
        v[scope + "/main/disc/1/dense/kernel"] = (f32, (H1, H2)); v[scope + "/main/disc/1/dense/bias"] = (f32, (H2,))
        v[scope + "/main/disc/disc_logits/kernel"] = (f32, (H2, 1)); v[scope + "/main/disc/disc_logits/bias"] = (f32, (1,))
        norms.append(("amp_obs_norm", amp_size))
    for name, size in norms:
        for k, (dt, shape) in (("mean", (f32, (size,))), ("std", (f32, (size,))), ("count", (i32, (1,)))):
            v["%s/resource/%s/%s" % (scope, name, k)] = (dt, shape); v["%s/resource/%s/%s_ph" % (scope, name, k)] = (dt, shape)
    if reward_scale:
        v[scope + "/reward_scale"] = (f32, (1,))
    return v
