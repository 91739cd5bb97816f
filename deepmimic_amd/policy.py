"""On-device policy inference: ctypes binding of `dm_policy_*` (include/dm_hip.h).

The actor of the reference's PPO / PG agents (learning/pg_agent.py:141-188, learning/nets/fc_2layers_1024units.py,
learning/normalizer.py) evaluated by hand-written MFMA kernels (deepmimic_amd/csrc/dm_policy.h) on device buffers, so a
rollout loop `states -> actions -> BatchEnv.step_device` never touches the host.  No CPU fallback.

The gated actor of the AMP task policies (learning/nets/fc_2layers_gated_1024units.py) is the same class: a weights dict that carries the gate arrays
(GATE_KEYS + "goal_dim") builds a gated context (dm_policy_create_gated).
"""
import ctypes as C
from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, u32, u64, vp
from .core import load_library


class _PolicyParams(C.Structure):
    _fields_ = [("state_dim", C.c_int), ("hidden1", C.c_int), ("hidden2", C.c_int), ("action_dim", C.c_int)] + \
               [(k, C.POINTER(C.c_float)) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "s_mean", "s_std", "a_mean", "a_std", "logstd")] + \
               [("s_clip", C.c_double)]


class _GateParams(C.Structure):
    _fields_ = [("goal_dim", C.c_int), ("gate_common", C.c_int), ("gate_hidden", C.c_int)] + \
               [(k, C.POINTER(C.c_float)) for k in ("gc_w", "gc_b", "g0_w", "g0_b", "g0_bias_w", "g0_bias_b", "g0_scale_w", "g0_scale_b",
                                                    "g1_w", "g1_b", "g1_bias_w", "g1_bias_b", "g1_scale_w", "g1_scale_b")]


# the gate of a weights dict (tf.layers.dense layout): gc_* = actor/gate_common/0/dense [G, GC]; g{i}_w / _b = actor/gate{i}/0/dense [GC, GH];
# g{i}_bias_* = actor/gate{i}/dense, g{i}_scale_* = actor/gate{i}/dense_1, [GH, H1] for i = 0 and [GH, H2] for i = 1; plus the integer "goal_dim"
GATE_KEYS = tuple(k for k, _ in _GateParams._fields_[3:])


def is_gated(weights: dict) -> bool:
    return any(weights.get(k) is not None for k in GATE_KEYS)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


PLAIN_KEYS = tuple(k for k, _ in _PolicyParams._fields_[4:15])
DM_DEVICE_PTRS, DM_WEIGHTS_OUT_IN = 1, 32      # include/dm_hip.h
# dm_policy_packed (include/dm_hip.h): the device arrays read_packed hands back, by the names of dm_policy.h PolicyDev / GateDev
PACKED_IDS = dict(w1p=0, w2p=1, w3p=2, b1=3, b2=4, b3=5, s_mean=6, s_inv_std=7, a_mean=8, a_std=9, logstd=10, wfs=11, gate_wcp=16, gate_bc=17,
                  gate_wep0=18, gate_be0=19, gate_wbp0=20, gate_bb0=21, gate_wsp0=22, gate_bs0=23,
                  gate_wep1=24, gate_be1=25, gate_wbp1=26, gate_bb1=27, gate_wsp1=28, gate_bs1=29)


class Policy:
    """weights: dict with w1 [S,H1], b1 [H1], w2 [H1,H2], b2 [H2], w3 [H2,A], b3 [A] (tf.layers.dense layout) and optional
    s_mean, s_std, a_mean, a_std, logstd.  With the arrays of GATE_KEYS and "goal_dim" (the last goal_dim of the S input columns are the goal) the
    context is the gated actor: same calls, the goal either as forward_device_ex's block or inside the state rows."""

    def __init__(self, weights: dict, device_id: int = 0, s_clip: float = 0.0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        w = {k: (None if weights.get(k) is None else np.ascontiguousarray(weights[k], dtype=np.float32)) for k in
             ("w1", "b1", "w2", "b2", "w3", "b3", "s_mean", "s_std", "a_mean", "a_std", "logstd")}
        self.S, self.H1 = w["w1"].shape
        self.H2, self.A = w["w3"].shape
        if w["w2"].shape != (self.H1, self.H2) or w["b1"].shape != (self.H1,) or w["b2"].shape != (self.H2,) or w["b3"].shape != (self.A,):
            raise ValueError("inconsistent layer shapes")
        pp = _PolicyParams(self.S, self.H1, self.H2, self.A, *[_fp(w[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "s_mean", "s_std", "a_mean", "a_std", "logstd")],
                           float(s_clip))
        self.h = C.c_void_p()
        self.device_id = int(device_id)
        self.gate_dims = None
        self.gated = is_gated(weights)
        if self.gated:
            missing = [k for k in GATE_KEYS + ("goal_dim",) if weights.get(k) is None]
            if missing:
                raise ValueError("gated actor: no %s in the weights" % ", ".join(missing))
            gw = {k: np.ascontiguousarray(weights[k], dtype=np.float32) for k in GATE_KEYS}
            G = int(weights["goal_dim"]); GC = gw["gc_w"].shape[1]; GH = gw["g0_w"].shape[1]
            want = dict(gc_w=(G, GC), gc_b=(GC,))
            for i, H in ((0, self.H1), (1, self.H2)):
                want.update({"g%d_w" % i: (GC, GH), "g%d_b" % i: (GH,), "g%d_bias_w" % i: (GH, H), "g%d_bias_b" % i: (H,), "g%d_scale_w" % i: (GH, H), "g%d_scale_b" % i: (H,)})
            bad = [k for k in GATE_KEYS if gw[k].shape != want[k]]
            if bad:
                raise ValueError("inconsistent gate shapes: %s is %s, not %s" % (bad[0], gw[bad[0]].shape, want[bad[0]]))
            if not hasattr(self.lib, "dm_policy_create_gated"):
                raise RuntimeError("libdm_hip: this library has no dm_policy_create_gated (rebuild it)")
            gp = _GateParams(G, GC, GH, *[_fp(gw[k]) for k in GATE_KEYS])
            self.gate_dims = (G, GC, GH)
            rc = self.lib.dm_policy_create_gated(int(device_id), C.byref(pp), C.byref(gp), C.byref(self.h))
        else:
            rc = self.lib.dm_policy_create(int(device_id), C.byref(pp), C.byref(self.h))
        check(self.lib, rc)

    @classmethod
    def from_checkpoint(cls, prefix: str, state_dim: Optional[int] = None, **kw):
        """the actor of a reference checkpoint (`--model_files <prefix>`: learning/rl_world.py:67-85, learning/tf_agent.py:36-48; read without TensorFlow by
        deepmimic_amd/tf_checkpoint.py) with its state / action normalisers.  An agent with a goal takes [state, goal] rows (forward_device_ex's goal block);
        its g_norm rides behind s_norm.  The index decides the mapper: a checkpoint with actor/gate* variables (the AMP task policies) gives the gated actor."""
        from . import tf_checkpoint
        gated = tf_checkpoint.is_gated_checkpoint(prefix)
        w = (tf_checkpoint.gated_actor_weights if gated else tf_checkpoint.actor_weights)(prefix, state_dim=state_dim)
        if "g_mean" in w:
            w["s_mean"] = np.concatenate([w["s_mean"], w["g_mean"]]); w["s_std"] = np.concatenate([w["s_std"], w["g_std"]])
        return cls(w, **kw)

    def forward_device(self, states_ptr: int, n: int, actions_ptr: int, logp_ptr: int = 0, sample: bool = False, seed: int = 0,
                       step: int = 0, env_id_offset: int = 0, stream: int = 0):
        """raw device pointers (e.g. torch.Tensor.data_ptr()); asynchronous on `stream` (a hipStream_t handle, 0 = null stream)."""
        check(self.lib, self.lib.dm_policy_forward(self.h, vp(states_ptr), int(n), vp(actions_ptr), vp(logp_ptr), int(bool(sample)), u64(seed), u32(step),
                                                   int(env_id_offset), vp(stream)))

    def forward_device_ex(self, states_ptr: int, n: int, actions_ptr: int, goals_ptr: int = 0, goal_dim: int = 0, logp_ptr: int = 0, exp_flags_ptr: int = 0,
                          exp_rate: float = 1.0, sample: bool = False, seed: int = 0, step: int = 0, env_id_offset: int = 0, stream: int = 0):
        """`_decide_action` of learning/pg_agent.py:214-221 for a batch (include/dm_hip.h dm_policy_forward_ex): goal block as its own input,
        per-row exploration coin with probability `exp_rate`, EXP flags out"""
        check(self.lib, self.lib.dm_policy_forward_ex(self.h, vp(states_ptr), vp(goals_ptr), int(goal_dim), int(n), vp(actions_ptr), vp(logp_ptr), vp(exp_flags_ptr),
                                                      C.c_double(exp_rate), int(bool(sample)), u64(seed), u32(step), int(env_id_offset), vp(stream)))

    def forward_host_ex(self, states, goals=None, exp_rate=1.0, sample=False, seed=0, step=0, env_id_offset=0):
        """emulator-build convenience for forward_device_ex: returns (actions, logp, exp_flags)"""
        s = np.ascontiguousarray(states, dtype=np.float32); n = s.shape[0]
        g = None if goals is None else np.ascontiguousarray(goals, dtype=np.float32)
        a = np.zeros((n, self.A), np.float32); lp = np.zeros(n, np.float32); fl = np.zeros(n, np.int32)
        self.forward_device_ex(s.ctypes.data, n, a.ctypes.data, 0 if g is None else g.ctypes.data, 0 if g is None else g.shape[1], lp.ctypes.data, fl.ctypes.data,
                               exp_rate, sample, seed, step, env_id_offset)
        return a, lp, fl

    def forward_host(self, states, sample=False, seed=0, step=0, env_id_offset=0):
        """Convenience for tests on the CPU emulator build, where "device" memory is host memory."""
        s = np.ascontiguousarray(states, dtype=np.float32)
        n = s.shape[0]
        a = np.zeros((n, self.A), np.float32); lp = np.zeros(n, np.float32)
        self.forward_device(s.ctypes.data, n, a.ctypes.data, lp.ctypes.data, sample, seed, step, env_id_offset)
        return a, lp

    def info(self) -> dict:
        """dm_policy_info (include/dm_hip.h): the padded widths K1 / N3, whether the one-launch actor's weight stream exists, and the
        dm_policy_path id and row count of the last forward call (path -1 before any); gated / goal_dim: a gated context and the goal columns its
        gate reads (the launch is then (path, gated)); gated_fused: the fused stream it holds is the gated one (k_policy_fused<.., true>)"""
        out = (C.c_int32 * 8)()
        check(self.lib, self.lib.dm_policy_info(self.h, out))
        return dict(K1=int(out[0]), N3=int(out[1]), fused=bool(out[2]), path=int(out[3]), rows=int(out[4]), gated=bool(out[5]), goal_dim=int(out[6]),
                    gated_fused=bool(out[7]))

    # ---- new weights into the live context (include/dm_hip.h dm_policy_set_weights): one kernel launch packs them in place
    def weight_shapes(self, out_in: bool = False) -> dict:
        """the shape of every array set_weights* takes, by key: 2-D arrays [in, out] (tf.layers.dense), or [out, in] (torch.nn.Linear.weight) with out_in"""
        S, H1, H2, A = self.S, self.H1, self.H2, self.A
        sh = dict(w1=(S, H1), b1=(H1,), w2=(H1, H2), b2=(H2,), w3=(H2, A), b3=(A,), s_mean=(S,), s_std=(S,), a_mean=(A,), a_std=(A,), logstd=(A,))
        if self.gated:
            G, GC, GH = self.gate_dims
            sh.update(gc_w=(G, GC), gc_b=(GC,))
            for i, H in ((0, H1), (1, H2)):
                sh.update({"g%d_w" % i: (GC, GH), "g%d_b" % i: (GH,), "g%d_bias_w" % i: (GH, H), "g%d_bias_b" % i: (H,), "g%d_scale_w" % i: (GH, H), "g%d_scale_b" % i: (H,)})
        return {k: (v[::-1] if out_in else v) for k, v in sh.items()}

    def _set_weights(self, ptrs: dict, flags: int, stream: int):
        if not hasattr(self.lib, "dm_policy_set_weights"):
            raise RuntimeError("libdm_hip: this library has no dm_policy_set_weights (rebuild it)")
        unknown = [k for k in ptrs if k not in PLAIN_KEYS + GATE_KEYS + ("goal_dim",)]
        if unknown:
            raise ValueError("set_weights: unknown key %s" % unknown[0])
        fp = lambda k: C.cast(C.c_void_p(int(ptrs[k])), C.POINTER(C.c_float)) if ptrs.get(k) else None
        pp = _PolicyParams(self.S, self.H1, self.H2, self.A, *[fp(k) for k in PLAIN_KEYS], 0.0)
        gp = None
        if self.gated or any(k in ptrs for k in GATE_KEYS):       # (a gate for a plain context: the library refuses it)
            G, GC, GH = self.gate_dims if self.gated else (int(ptrs.get("goal_dim", 0)), 0, 0)
            gp = C.byref(_GateParams(G, GC, GH, *[fp(k) for k in GATE_KEYS]))
        check(self.lib, self.lib.dm_policy_set_weights(self.h, C.byref(pp), gp, int(flags), vp(stream)))

    def set_weights(self, weights: dict):
        """host arrays under the constructor's keys (and GATE_KEYS); a missing key keeps what the context holds.  Staged through a device temporary; synchronous."""
        want = self.weight_shapes()
        w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items() if v is not None and k != "goal_dim"}
        for k, a in w.items():
            if k in want and a.shape != want[k]:
                raise ValueError("set_weights: %s is %s, not %s" % (k, a.shape, want[k]))
        self._set_weights({k: a.ctypes.data for k, a in w.items()}, 0, 0)

    def set_weights_device(self, ptrs: dict, out_in: bool = False, stream: int = 0):
        """raw device addresses of fp32 arrays (4-byte aligned is enough) under the same keys, shapes as weight_shapes(out_in); asynchronous on `stream`:
        no allocation, no host copy, no synchronisation.  Ordering against forwards on other streams is the caller's."""
        self._set_weights(ptrs, DM_DEVICE_PTRS | (DM_WEIGHTS_OUT_IN if out_in else 0), stream)

    def set_weights_torch(self, tensors: dict, layout: str = "in_out", stream=None):
        """torch tensors on the policy's device, e.g. layout="out_in" with the .weight / .bias of torch.nn.Linear layers after an optimiser step.  Runs on torch's
        current stream unless `stream` (a torch.cuda.Stream or a raw handle) is given: enqueue it behind the optimiser step and in front of the next forward."""
        import torch
        if layout not in ("in_out", "out_in"):
            raise ValueError('layout must be "in_out" or "out_in"')
        want = self.weight_shapes(layout == "out_in")
        dev = torch.device("cuda", self.device_id)
        ptrs = {}
        for k, t in tensors.items():
            if t is None or k == "goal_dim":
                continue
            if k not in want:
                raise ValueError("set_weights: unknown key %s" % k)
            ptrs[k] = tensor_arg(k, t, dev, torch.float32, [want[k]]).data_ptr()
        self.set_weights_device(ptrs, layout == "out_in", stream_handle(dev, stream))

    def read_packed(self, name: str) -> np.ndarray:
        """the bytes (uint8) of one packed device array as the kernels read it (PACKED_IDS: w1p .. logstd, wfs, gate_*); synchronises the device.
        RuntimeError where the context holds no such array (wfs on widths without the fused kernel, gate_* on a plain context)."""
        if not hasattr(self.lib, "dm_policy_read_packed"):
            raise RuntimeError("libdm_hip: this library has no dm_policy_read_packed (rebuild it)")
        n = C.c_size_t(0)
        check(self.lib, self.lib.dm_policy_read_packed(self.h, PACKED_IDS[name], None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        check(self.lib, self.lib.dm_policy_read_packed(self.h, PACKED_IDS[name], out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.dm_policy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reference_forward(weights: dict, states, s_clip=np.inf, bf16=False):
    """Plain numpy statement of the same actor (fp32; bf16=True rounds operands to bfloat16 at the points the kernels do).
    Returns the mode action and the normalised mean.  With the gate arrays (GATE_KEYS, "goal_dim") it is the gated actor: the gate reads the normalised,
    clipped goal columns; xg, c, e_i are rounded where the kernels round them, sigma, beta and the gated pre-activation are fp32."""
    def r(x):
        if not bf16:
            return x.astype(np.float32)
        u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    S = weights["w1"].shape[0]
    s = np.asarray(states, dtype=np.float32)
    sm = weights.get("s_mean"); ss = weights.get("s_std")
    x = (s - (0 if sm is None else sm.astype(np.float32))) * (np.float32(1) / (np.float32(1) if ss is None else ss.astype(np.float32)))
    x = np.clip(x, -s_clip, s_clip)
    if is_gated(weights):
        f32 = np.float32
        dense = lambda v, k: (r(v).astype(np.float64) @ r(weights[k + "_w"]).astype(np.float64) + weights[k + "_b"]).astype(f32)
        c = np.maximum(dense(x[:, S - int(weights["goal_dim"]):], "gc"), 0)
        h = x
        for i, (wk, bk) in enumerate((("w1", "b1"), ("w2", "b2"))):
            e = np.maximum(dense(c, "g%d" % i), 0)
            beta = dense(e, "g%d_bias" % i)
            with np.errstate(over="ignore"):
                sigma = (f32(2) / (f32(1) + np.exp(-dense(e, "g%d_scale" % i)))).astype(f32)
            pre = (r(h).astype(np.float64) @ r(weights[wk]).astype(np.float64) + weights[bk]).astype(f32)
            h = np.maximum((sigma.astype(np.float64) * pre + beta).astype(f32), 0)
    else:
        h = np.maximum(r(x).astype(np.float64) @ r(weights["w1"]).astype(np.float64) + weights["b1"], 0).astype(np.float32)
        h = np.maximum(r(h).astype(np.float64) @ r(weights["w2"]).astype(np.float64) + weights["b2"], 0).astype(np.float32)
    m = (r(h).astype(np.float64) @ r(weights["w3"]).astype(np.float64) + weights["b3"]).astype(np.float32)
    am = weights.get("a_mean"); as_ = weights.get("a_std")
    a = m * (1 if as_ is None else as_) + (0 if am is None else am)
    return a.astype(np.float32), m


def random_weights(S, A, H1=1024, H2=512, seed=0, init_output_scale=0.01, noise=0.05, gated_goal_dim=0, gate_common=128, gate_hidden=64):
    """Random-init weights of the reference architecture: Xavier-uniform hidden layers (learning/tf_util.py:27-39), uniform
    (+-init_output_scale) output layer, logstd = log(noise) (pg_agent.py:147-158).  gated_goal_dim = G > 0 adds the gate of
    fc_2layers_gated_1024units.py on the last G of the S columns: Xavier kernels, zero biases (drawn after the plain layers, which stay what they are)."""
    rng = np.random.default_rng(seed)
    def xav(i, o):
        lim = np.sqrt(6.0 / (i + o)); return rng.uniform(-lim, lim, size=(i, o)).astype(np.float32)
    w = _plain_random_weights(rng, xav, S, A, H1, H2, init_output_scale, noise)
    if gated_goal_dim:
        G, GC, GH = int(gated_goal_dim), gate_common, gate_hidden
        w.update(goal_dim=G, gc_w=xav(G, GC), gc_b=np.zeros(GC, np.float32))
        for i, H in ((0, H1), (1, H2)):
            w.update({"g%d_w" % i: xav(GC, GH), "g%d_b" % i: np.zeros(GH, np.float32), "g%d_bias_w" % i: xav(GH, H), "g%d_bias_b" % i: np.zeros(H, np.float32),
                      "g%d_scale_w" % i: xav(GH, H), "g%d_scale_b" % i: np.zeros(H, np.float32)})
    return w


def _plain_random_weights(rng, xav, S, A, H1, H2, init_output_scale, noise):
    return dict(w1=xav(S, H1), b1=np.zeros(H1, np.float32), w2=xav(H1, H2), b2=np.zeros(H2, np.float32),
                w3=rng.uniform(-init_output_scale, init_output_scale, size=(H2, A)).astype(np.float32), b3=np.zeros(A, np.float32),
                logstd=np.full(A, np.log(noise), np.float32))
