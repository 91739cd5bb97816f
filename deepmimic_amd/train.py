"""PPO actor and critic minibatch updates on the device (libdm_hip.so `dm_train_*`, deepmimic_amd/csrc/dm_train.h, include/dm_hip.h): what the reference's
PPOAgent._update_actor / _update_critic and MPISolver.update do (learning/ppo_agent.py:95-139, 286-309, learning/solvers/mpi_solver.py:33-54) for the plain
three-layer nets, on the `Policy` context that samples -- the forward pass runs on the context's own kernels, so the trained net IS the sampling net.

    tr = ActorTrainer.from_policy(actor, weights, stepsize=..., momentum=0.9)       # owns the [3, P] tensor (params, momentum, grads) and the workspace
    tr.grad(states, actions, old_logp, adv, goals=...)                               # gradients into tr.grads, statistics into tr.stats()
    all_reduce_gradients(tr)                                                         # (deepmimic_amd/dist.py, several ranks)
    tr.step(grad_scale=1.0 / world)                                                  # momentum SGD on the fp32 masters, then the refresh of the context

A checkpoint is `torch.save(tr.buf)`.  A fused training kernel is out of scope.

Every trainer takes `optimizer="adam"`, `betas`, `eps`, `max_grad_norm` and `skip_nonfinite` (`dm_train_opt_step`, deepmimic_amd/csrc/dm_optim.h): Adam on the fp32
masters, global-norm clipping of the (all-reduced, scaled) gradient and a step that is skipped when a gradient element is not finite, all decided on the device --
`tr.grad_norm()`, `tr.grad_scale_applied()`, `tr.skipped()` are views of `tr.opt_state`, the [8] float64 device tensor, and the checkpoint is then `tr.buf` ([4, P] with
Adam: row 3 is v) plus `tr.opt_state`.  With the defaults nothing changes: the old entry points, buf [3, P].  A step-size schedule is assigning `tr.stepsize`.

The gated nets of the AMP task agents (fc_2layers_gated_1024units as ActorNet and CriticNet; `dm_train_gated_*`, deepmimic_amd/csrc/dm_train_gated.h) have trainers of
their own with the same surface, `GatedActorTrainer` / `GatedCriticTrainer`, on a gated `Policy` or on the context inside a gated `heads.Critic`
(`GatedCriticTrainer.from_policy(critic.net, weights, ...)`): the parameter block carries the gate's fourteen arrays behind the six plain ones (`gated_layout`), the
backward pass runs through sigma, beta and the gate's hidden layers, and the step refreshes the gate in the context too.  The plain trainers refuse a gated context.

The AMP discriminator update (AMPAgent._step_disc, learning/amp_agent.py:134-207, 251-257, 356-377; `dm_train_disc_grad`) is `DiscTrainer`, on the context inside a
`heads.Discriminator`, so that the net that scores the style reward is the net that was trained:

    dt = DiscTrainer.from_policy(disc.net, weights, stepsize=..., momentum=0.9, weight_decay=DiscWeightDecay)
    dt.grad(expert_obs, agent_obs, grad_penalty=10.0, logit_reg=0.05)                # the two batches as dm_amp_expert_draw / dm_replay_sample fill them
    all_reduce_gradients(dt); dt.step(grad_scale=1.0 / world)                        # disc.eval_* now scores with the new weights

`reference_grad` / `reference_step` / `reference_disc_grad` / `reference_gated_grad` are the numpy statements of the arithmetic (the specification of include/dm_hip.h): the same
rounding points -- bf16 operands, the head's fp32 operations one by one, the library's own exp -- with the contractions accumulated in float64."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, vp
from .policy import GATE_KEYS

KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")
GATED_KEYS = KEYS + GATE_KEYS           # the gated parameter block: matrices and their bias vectors alternate
LN_2PI = np.float32(1.8378770664093453)


class _ActorCfg(C.Structure):
    _fields_ = [("ratio_clip", C.c_double), ("bound_weight", C.c_double), ("a_bound_min", C.POINTER(C.c_float)), ("a_bound_max", C.POINTER(C.c_float))]


# ---- the parameter block and the workspace

# A block is its keys in order and their shapes: arrays back to back, matrices (even places) and their bias vectors (odd places) alternating.

def _block_layout(keys, shapes: dict) -> dict:
    out, at = {}, 0
    for k in keys:
        out[k] = (at, shapes[k]); at += int(np.prod(shapes[k]))
    out["P"] = at
    return out


def _block_pack(keys, arrays: dict, dtype=np.float32) -> np.ndarray:
    """the arrays of a dict back to back (dtype None: as they are)"""
    return np.concatenate([np.ascontiguousarray(arrays[k], dtype=dtype).reshape(-1) for k in keys])


def _block_views(flat, keys, lay: dict) -> dict:
    return {k: flat[lay[k][0]:lay[k][0] + int(np.prod(lay[k][1]))].reshape(lay[k][1]) for k in keys}


def _block_matrix_mask(keys, lay: dict) -> np.ndarray:
    m = np.zeros(lay["P"], bool)
    for v in _block_views(m, keys[0::2], lay).values():
        v[...] = True
    return m


def layout(S: int, H1: int, H2: int, A: int) -> dict:
    """{key: (offset in floats, shape)} of the parameter block, and "P" -> its length"""
    return _block_layout(KEYS, dict(w1=(S, H1), b1=(H1,), w2=(H1, H2), b2=(H2,), w3=(H2, A), b3=(A,)))


def pack_params(weights: dict) -> np.ndarray:
    """the float32 parameter block of a weights dict (w1 .. b3, tf.layers.dense layout)"""
    return _block_pack(KEYS, weights)


def unpack_params(flat, S: int, H1: int, H2: int, A: int) -> dict:
    """views of a parameter block under the keys w1 .. b3 (numpy array or torch tensor)"""
    return _block_views(flat, KEYS, layout(S, H1, H2, A))


def workspace_layout(H1: int, H2: int, A: int, n: int) -> dict:
    """{name: (byte offset, dtype, shape)} of what a *_grad call leaves in its workspace (include/dm_hip.h); "bytes": the total"""
    N3 = (A + 31) // 32 * 32
    out, at = {}, 0
    for name, dt, shape in (("z3", np.float32, (n, N3)), ("dz3", np.uint16, (n, N3)), ("dz2", np.uint16, (n, H2)), ("dz1", np.uint16, (n, H1)),
                            ("part", np.float64, ((n + 15) // 16, 8))):
        out[name] = (at, dt, shape); at += int(np.prod(shape)) * np.dtype(dt).itemsize
    out["bytes"] = at
    return out


def _need(policy, symbol: str):
    """the library's entry point `symbol`; a library from before it refuses by name"""
    call = getattr(policy.lib, symbol, None)
    if call is None:
        raise RuntimeError("libdm_hip: this library has no %s (rebuild it)" % symbol)
    return call


def _int_call(policy, symbol: str, *args) -> int:
    """an entry point that returns a count or a size, < 0 where it refuses"""
    v = _need(policy, symbol)(policy.h, *(int(a) for a in args))
    check(policy.lib, v < 0)
    return int(v)


def param_count(policy) -> int:
    return _int_call(policy, "dm_train_param_count")


def workspace_bytes(policy, n: int) -> int:
    return _int_call(policy, "dm_train_workspace_bytes", n)


def actor_grad_device(policy, params_ptr: int, states_ptr: int, n: int, actions_ptr: int, old_logp_ptr: int, adv_ptr: int, grads_ptr: int, stats_ptr: int,
                      workspace_ptr: int, workspace_nbytes: int, ratio_clip: float = 0.2, bound_weight: float = 10.0, a_bound_min=None, a_bound_max=None,
                      goals_ptr: int = 0, goal_dim: int = 0, logp_ptr: int = 0, stream: int = 0, gated: bool = False):
    """raw device pointers (ints); a_bound_min / a_bound_max: host arrays of A un-normalised entries or None; asynchronous on `stream`.  gated: dm_train_gated_actor_grad,
    the same parameter list on a gated context and its block and workspace"""
    call = _need(policy, "dm_train_gated_actor_grad" if gated else "dm_train_actor_grad")
    lo = None if a_bound_min is None else np.ascontiguousarray(a_bound_min, dtype=np.float32)
    hi = None if a_bound_max is None else np.ascontiguousarray(a_bound_max, dtype=np.float32)
    for b in (lo, hi):
        if b is not None and b.shape != (policy.A,):
            raise ValueError("action bounds must have %d entries" % policy.A)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    cfg = _ActorCfg(float(ratio_clip), float(bound_weight), fp(lo), fp(hi))
    check(policy.lib, call(policy.h, vp(params_ptr), vp(states_ptr), vp(goals_ptr), int(goal_dim), int(n), vp(actions_ptr), vp(old_logp_ptr), vp(adv_ptr),
                           C.cast(C.pointer(cfg), C.c_void_p), vp(grads_ptr), vp(stats_ptr), vp(logp_ptr), vp(workspace_ptr), int(workspace_nbytes), vp(stream)))


def value_grad_device(policy, params_ptr: int, states_ptr: int, n: int, targets_ptr: int, grads_ptr: int, stats_ptr: int, workspace_ptr: int, workspace_nbytes: int,
                      goals_ptr: int = 0, goal_dim: int = 0, values_ptr: int = 0, stream: int = 0, gated: bool = False):
    call = _need(policy, "dm_train_gated_value_grad" if gated else "dm_train_value_grad")
    check(policy.lib, call(policy.h, vp(params_ptr), vp(states_ptr), vp(goals_ptr), int(goal_dim), int(n), vp(targets_ptr), vp(grads_ptr), vp(stats_ptr), vp(values_ptr),
                           vp(workspace_ptr), int(workspace_nbytes), vp(stream)))


def sgd_step_device(policy, params_ptr: int, momentum_ptr: int, grads_ptr: int, P: int, stepsize: float, momentum: float, weight_decay: float = 0.0,
                    grad_scale: float = 1.0, stream: int = 0, lib=None):
    """policy None: the step alone (pass `lib`); with a policy its context is refreshed from the new masters"""
    lib = policy.lib if policy is not None else lib
    if not hasattr(lib, "dm_train_sgd_step"):
        raise RuntimeError("libdm_hip: this library has no dm_train_* entry points (rebuild it)")
    check(lib, lib.dm_train_sgd_step(policy.h if policy is not None else None, vp(params_ptr), vp(momentum_ptr), vp(grads_ptr), int(P), float(stepsize), float(momentum),
                                     float(weight_decay), float(grad_scale), vp(stream)))


# ---- Adam, global-norm clipping and the non-finite guard (dm_train_opt_step, deepmimic_amd/csrc/dm_optim.h)

class _OptCfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("skip_nonfinite", C.c_int32), ("stepsize", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("grad_scale", C.c_double), ("max_grad_norm", C.c_double)]


OPT_KINDS = {"momentum": 0, "adam": 1}                      # DM_OPT_MOMENTUM, DM_OPT_ADAM
OPT_STATE = ("t", "pow1", "pow2", "skipped", "norm", "scale", "nonfinite", "reserved")          # the eight words of state_dev
OPT_CHUNK, OPT_THREADS = 1024, 256                          # elements per partial of the norm pass, threads per workgroup


def opt_workspace_layout(P: int) -> dict:
    """{name: (byte offset, dtype, shape)} of what dm_train_opt_step leaves in its workspace: the control record, then the norm pass's partials -- group b owns the
    elements [OPT_CHUNK b, OPT_CHUNK (b + 1)), thread t of it the elements OPT_CHUNK b + t + OPT_THREADS k; "groups": their number; "bytes": the total"""
    G = (int(P) + OPT_CHUNK - 1) // OPT_CHUNK
    ctrl = np.dtype([("skip", np.int32), ("s", np.float32), ("alpha", np.float64), ("ic2", np.float64), ("pad", np.float64)])
    return dict(ctrl=(0, ctrl, (1,)), sum=(32, np.float64, (G,)), count=(32 + 8 * G, np.float64, (G,)), groups=G, bytes=32 + 16 * G)


def opt_workspace_bytes(P: int, lib) -> int:
    if not hasattr(lib, "dm_train_opt_workspace_bytes"):
        raise RuntimeError("libdm_hip: this library has no dm_train_opt_workspace_bytes (rebuild it)")
    v = lib.dm_train_opt_workspace_bytes(int(P))
    check(lib, v < 0)
    return int(v)


def opt_step_device(policy, params_ptr: int, m_ptr: int, v_ptr: int, grads_ptr: int, P: int, state_ptr: int, workspace_ptr: int, workspace_nbytes: int, stepsize: float,
                    kind: str = "adam", beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
                    max_grad_norm=None, skip_nonfinite: bool = False, stream: int = 0, lib=None):
    """raw device pointers (ints).  kind "momentum" (beta1 is the momentum, v_ptr may be 0) or "adam"; max_grad_norm None: no clipping; state_ptr: double[8], zero
    before the first step.  policy None: the step alone (pass `lib`); with a policy -- plain, gated or a discriminator's -- its context is refreshed from the masters"""
    lib = policy.lib if policy is not None else lib
    if not hasattr(lib, "dm_train_opt_step"):
        raise RuntimeError("libdm_hip: this library has no dm_train_opt_step (rebuild it)")
    k = OPT_KINDS.get(kind, kind)
    cfg = _OptCfg(int(k) if isinstance(k, (int, np.integer)) else -1, 1 if skip_nonfinite else 0, float(stepsize), float(beta1), float(beta2), float(eps),
                  float(weight_decay), float(grad_scale), 0.0 if max_grad_norm is None else float(max_grad_norm))
    check(lib, lib.dm_train_opt_step(policy.h if policy is not None else None, C.cast(C.pointer(cfg), C.c_void_p), vp(params_ptr), vp(m_ptr), vp(v_ptr), vp(grads_ptr),
                                     int(P), vp(state_ptr), vp(workspace_ptr), int(workspace_nbytes), vp(stream)))


def read_activations(policy, which: str, n: int) -> np.ndarray:
    """test support: the first n rows of "s16" [n, K1], "h1" or "h2" as the last call left them, bf16 bits (uint16); synchronises"""
    _need(policy, "dm_train_read_activations")
    width = dict(s16=policy.info()["K1"], h1=policy.H1, h2=policy.H2)[which]
    out = np.zeros((int(n), width), np.uint16)
    check(policy.lib, policy.lib.dm_train_read_activations(policy.h, ("s16", "h1", "h2").index(which), int(n), out.ctypes.data, out.nbytes))
    return out


# ---- the trainers

class _Trainer:
    """Owns buf [3, P] float32 = (params, momentum, grads) -- with optimizer="adam" [4, P]: (params, m, grads, v) -- and the workspace, on `device` (the policy's GPU;
    "cpu" with the emulator build of the tests, where device memory is host memory).  Every call runs on torch's current stream."""
    N_STATS = 0
    GATED = False
    # what a trainer of another kind of net replaces: the block's length, packing and views, the workspace's size and the step
    _param_count = staticmethod(param_count)
    _pack = staticmethod(pack_params)
    _unpack = staticmethod(lambda flat, p: unpack_params(flat, p.S, p.H1, p.H2, p.A))
    _workspace_bytes = staticmethod(workspace_bytes)
    _step = staticmethod(sgd_step_device)

    def __init__(self, policy, buf, stepsize: float, momentum: float, weight_decay: float, optimizer: str = "momentum", betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm=None, skip_nonfinite: bool = False):
        """With the defaults the step is dm_train_sgd_step / dm_train_gated_sgd_step and buf is [3, P].  optimizer "adam" (buf [4, P]: row 1 is m, row 3 is v),
        max_grad_norm (global-norm clipping of the scaled gradient) or skip_nonfinite (no step when a gradient element is NaN or +-inf) take the step through
        dm_train_opt_step, which keeps its decisions in `opt_state`, the [8] float64 device tensor (OPT_STATE); a checkpoint is then buf plus opt_state.  `stepsize`
        stays a plain attribute: a schedule is the caller assigning it between steps."""
        import torch
        _need(policy, "dm_train_gated_actor_grad" if self.GATED else "dm_train_actor_grad")
        if optimizer not in OPT_KINDS:
            raise ValueError("optimizer must be \"momentum\" or \"adam\"")
        self.policy, self.buf = policy, buf
        self.P = self._param_count(policy)
        self.optimizer = optimizer
        rows = 4 if optimizer == "adam" else 3
        tensor_arg("buf", buf, buf.device, torch.float32, [(rows, self.P)])
        self.device = buf.device
        self.params, self.momentum, self.grads = buf[0], buf[1], buf[2]
        self.second_moment = buf[3] if rows == 4 else None
        self.stepsize, self.mom, self.weight_decay = float(stepsize), float(momentum), float(weight_decay)
        self.betas, self.eps, self.max_grad_norm, self.skip_nonfinite = (float(betas[0]), float(betas[1])), float(eps), max_grad_norm, bool(skip_nonfinite)
        self._stats = torch.zeros(self.N_STATS, dtype=torch.float64, device=self.device)
        self._work, self._work_bytes, self._work_key = None, 0, None
        self.opt_state = None
        if optimizer != "momentum" or max_grad_norm is not None or skip_nonfinite:
            _need(policy, "dm_train_opt_step")
            self.opt_state = torch.zeros(len(OPT_STATE), dtype=torch.float64, device=self.device)
            self._opt_bytes = opt_workspace_bytes(self.P, policy.lib)
            self._opt_work = torch.zeros((self._opt_bytes + 15) // 16 * 2, dtype=torch.float64, device=self.device)

    @classmethod
    def from_policy(cls, policy, weights: dict, stepsize: float, momentum: float = 0.9, weight_decay: float = 0.0, device=None, optimizer: str = "momentum", **opt):
        """masters from the weights dict the policy was built from (zero momentum), then `sync()`.  opt: betas, eps, max_grad_norm, skip_nonfinite of __init__"""
        import torch
        dev = torch.device("cuda", policy.device_id) if device is None else torch.device(device)
        flat = cls._pack(weights)
        buf = torch.zeros((4 if optimizer == "adam" else 3, flat.size), dtype=torch.float32, device=dev)
        buf[0].copy_(torch.from_numpy(flat))
        tr = cls(policy, buf, stepsize, momentum, weight_decay, optimizer=optimizer, **opt)
        tr.sync()
        return tr

    def _stream(self):
        return stream_handle(self.device) if self.device.type == "cuda" else 0

    def views(self, which: str = "params") -> dict:
        """w1 .. b3 (a gated trainer: and the gate's arrays) as views of params / momentum / grads"""
        return self._unpack(getattr(self, which), self.policy)

    def sync(self):
        """packs the masters into the context (the precondition of grad: its bf16 weights are the rounding of params)"""
        self.policy.set_weights_device({k: v.data_ptr() for k, v in self.views().items()}, stream=self._stream())

    def _workspace(self, sizer, *rows: int):
        """(pointer, bytes) of a workspace that holds a call of `rows` (one count, or one per batch): it grows to sizer(policy, *rows) and never shrinks in any count"""
        if rows != self._work_key:                       # (the counts of the last growth again: the steady state of a learner, one comparison)
            have = self._work_key or (0,) * len(rows)
            if any(r > h for r, h in zip(rows, have)):
                import torch
                self._work_key = tuple(max(r, h) for r, h in zip(rows, have))
                self._work_bytes = sizer(self.policy, *self._work_key)
                self._work = torch.zeros((self._work_bytes + 15) // 16 * 2, dtype=torch.float64, device=self.device)
        return self._work.data_ptr(), self._work_bytes

    def _rows(self, states, goals):
        import torch
        n = int(states.shape[0]) if states.dim() == 2 else -1
        G = 0 if goals is None else (int(goals.shape[1]) if goals.dim() == 2 else -1)
        tensor_arg("states", states, self.device, torch.float32, [(n, self.policy.S - max(G, 0))])
        if goals is not None:
            tensor_arg("goals", goals, self.device, torch.float32, [(n, G)])
        return n, G

    def step(self, grad_scale: float = 1.0):
        if self.opt_state is None:
            return self._step(self.policy, self.params.data_ptr(), self.momentum.data_ptr(), self.grads.data_ptr(), self.P, self.stepsize, self.mom, self.weight_decay,
                              grad_scale, stream=self._stream())
        adam = self.optimizer == "adam"
        opt_step_device(self.policy, self.params.data_ptr(), self.momentum.data_ptr(), self.second_moment.data_ptr() if adam else 0, self.grads.data_ptr(), self.P,
                        self.opt_state.data_ptr(), self._opt_work.data_ptr(), self._opt_bytes, self.stepsize, self.optimizer, self.betas[0] if adam else self.mom,
                        self.betas[1], self.eps, self.weight_decay, grad_scale, self.max_grad_norm, self.skip_nonfinite, stream=self._stream())

    def _opt_word(self, name: str):
        if self.opt_state is None:
            raise RuntimeError("this trainer keeps no optimiser state: the default momentum step measures nothing (max_grad_norm, skip_nonfinite or optimizer=\"adam\")")
        return self.opt_state[OPT_STATE.index(name)]

    def grad_norm(self):
        """|grad_scale| |grads| of the last step, a 0-dim float64 device view of opt_state (no synchronisation); 0 when neither clipping nor the guard is on"""
        return self._opt_word("norm")

    def grad_scale_applied(self):
        """the clipping factor min(1, max_grad_norm / (norm + 1e-6)) of the last step, a device view"""
        return self._opt_word("scale")

    def skipped(self):
        """the number of steps the non-finite guard has skipped, a device view"""
        return self._opt_word("skipped")

    def stats(self):
        """the statistics of the last grad call, a float64 device tensor (no synchronisation here)"""
        return self._stats


class ActorTrainer(_Trainer):
    """stats(): {n, -mean min(l0, l1), bound loss, clip_frac, mean ratio, mean logp_new}"""
    N_STATS = 6

    def grad(self, states, actions, old_logp, adv, goals=None, ratio_clip: float = 0.2, bound_weight: float = 10.0, a_bound_min=None, a_bound_max=None, logp_out=None):
        import torch
        n, G = self._rows(states, goals)
        tensor_arg("actions", actions, self.device, torch.float32, [(n, self.policy.A)])
        tensor_arg("old_logp", old_logp, self.device, torch.float32, [(n,)]); tensor_arg("adv", adv, self.device, torch.float32, [(n,)])
        if logp_out is not None:
            tensor_arg("logp_out", logp_out, self.device, torch.float32, [(n,)])
        ws, nbytes = self._workspace(self._workspace_bytes, n)
        actor_grad_device(self.policy, self.params.data_ptr(), states.data_ptr(), n, actions.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), self.grads.data_ptr(),
                          self._stats.data_ptr(), ws, nbytes, ratio_clip, bound_weight, a_bound_min, a_bound_max, 0 if goals is None else goals.data_ptr(), G,
                          0 if logp_out is None else logp_out.data_ptr(), self._stream(), self.GATED)


class CriticTrainer(_Trainer):
    """stats(): {0.5 mean (tar - v)^2, mean v}"""
    N_STATS = 2

    def grad(self, states, targets, goals=None, values_out=None):
        import torch
        n, G = self._rows(states, goals)
        tensor_arg("targets", targets, self.device, torch.float32, [(n,)])
        if values_out is not None:
            tensor_arg("values_out", values_out, self.device, torch.float32, [(n,)])
        ws, nbytes = self._workspace(self._workspace_bytes, n)
        value_grad_device(self.policy, self.params.data_ptr(), states.data_ptr(), n, targets.data_ptr(), self.grads.data_ptr(), self._stats.data_ptr(), ws, nbytes,
                          0 if goals is None else goals.data_ptr(), G, 0 if values_out is None else values_out.data_ptr(), self._stream(), self.GATED)


# ---- the gated nets (dm_train_gated_*)

def gated_layout(S: int, H1: int, H2: int, A: int, G: int, GC: int, GH: int) -> dict:
    """{key: (offset in floats, shape)} of the gated parameter block -- the six plain arrays, then the gate's in the order of dm_policy_gate_params -- and "P" -> its length"""
    shapes = dict(w1=(S, H1), b1=(H1,), w2=(H1, H2), b2=(H2,), w3=(H2, A), b3=(A,), gc_w=(G, GC), gc_b=(GC,))
    for i, H in ((0, H1), (1, H2)):
        shapes.update({"g%d_w" % i: (GC, GH), "g%d_b" % i: (GH,), "g%d_bias_w" % i: (GH, H), "g%d_bias_b" % i: (H,), "g%d_scale_w" % i: (GH, H), "g%d_scale_b" % i: (H,)})
    return _block_layout(GATED_KEYS, shapes)


def gated_dims(weights: dict) -> tuple:
    """(S, H1, H2, A, G, GC, GH) of a gated weights dict"""
    S, H1 = np.shape(weights["w1"]); H2, A = np.shape(weights["w3"])
    return S, H1, H2, A, int(weights["goal_dim"]), np.shape(weights["gc_w"])[1], np.shape(weights["g0_w"])[1]


def pack_gated_params(weights: dict) -> np.ndarray:
    """the float32 parameter block of a gated weights dict (GATED_KEYS, tf.layers.dense layout)"""
    return _block_pack(GATED_KEYS, weights)


def unpack_gated_params(flat, S: int, H1: int, H2: int, A: int, G: int, GC: int, GH: int) -> dict:
    """views of a gated parameter block under GATED_KEYS (numpy array or torch tensor)"""
    return _block_views(flat, GATED_KEYS, gated_layout(S, H1, H2, A, G, GC, GH))


def gated_workspace_layout(H1: int, H2: int, A: int, G: int, GC: int, GH: int, n: int) -> dict:
    """{name: (byte offset, dtype, shape)} of what a gated *_grad call leaves in its workspace: the pieces of `workspace_layout` (dz2 / dz1 hold dp_1 / dp_0), then the
    gate split, the gate's activations and their gradients, bf16; "bytes": the total"""
    KG = (G + 31) // 32 * 32
    out = workspace_layout(H1, H2, A, n)
    at = out.pop("bytes")
    for name, width in (("du1", H2), ("du0", H1), ("da1", H2), ("da0", H1), ("xg", KG), ("c", GC), ("e0", GH), ("e1", GH), ("dze0", GH), ("dze1", GH), ("dzc", GC)):
        out[name] = (at, np.uint16, (n, width)); at += (n * width * 2 + 15) // 16 * 16
    out["bytes"] = at
    return out


def gated_param_count(policy) -> int:
    return _int_call(policy, "dm_train_gated_param_count")


def gated_workspace_bytes(policy, n: int) -> int:
    return _int_call(policy, "dm_train_gated_workspace_bytes", n)


def gated_sgd_step_device(policy, params_ptr: int, momentum_ptr: int, grads_ptr: int, P: int, stepsize: float, momentum: float, weight_decay: float = 0.0,
                          grad_scale: float = 1.0, stream: int = 0):
    """the momentum step on a gated block (weight decay on its ten matrices), then the refresh of the context, gate included; the net is required"""
    _need(policy, "dm_train_gated_sgd_step")
    check(policy.lib, policy.lib.dm_train_gated_sgd_step(policy.h, vp(params_ptr), vp(momentum_ptr), vp(grads_ptr), int(P), float(stepsize), float(momentum),
                                                         float(weight_decay), float(grad_scale), vp(stream)))


GATED_READ = ("s16", "h1", "h2", "sigma0", "beta0", "sigma1", "beta1")


def read_gated(policy, which: str, n: int) -> np.ndarray:
    """test support: the first n rows of "s16" [n, K1], "h1", "h2" (bf16 bits, uint16) or "sigma0", "beta0" [n, H1], "sigma1", "beta1" [n, H2] (float32) as the last call
    left them; synchronises"""
    _need(policy, "dm_train_gated_read")
    i = GATED_READ.index(which)
    width = (policy.info()["K1"], policy.H1, policy.H2, policy.H1, policy.H1, policy.H2, policy.H2)[i]
    out = np.zeros((int(n), width), np.uint16 if i < 3 else np.float32)
    check(policy.lib, policy.lib.dm_train_gated_read(policy.h, i, int(n), out.ctypes.data, out.nbytes))
    return out


class _GatedHooks:
    """what turns a trainer into the one of a gated context: the gated block, workspace and step"""
    GATED = True
    _param_count = staticmethod(gated_param_count)
    _pack = staticmethod(pack_gated_params)
    _unpack = staticmethod(lambda flat, p: unpack_gated_params(flat, p.S, p.H1, p.H2, p.A, *p.gate_dims))
    _workspace_bytes = staticmethod(gated_workspace_bytes)
    _step = staticmethod(gated_sgd_step_device)


class GatedActorTrainer(_GatedHooks, ActorTrainer):
    """ActorTrainer on a gated `Policy`: views() has the twenty arrays of GATED_KEYS, sync() and step() refresh the gate as well"""


class GatedCriticTrainer(_GatedHooks, CriticTrainer):
    """CriticTrainer on a gated context with one output, e.g. `from_policy(critic.net, weights, ...)` of a gated `heads.Critic`"""


# ---- the AMP discriminator update

class _DiscCfg(C.Structure):
    _fields_ = [("grad_penalty", C.c_double), ("logit_reg", C.c_double)]


DISC_STATS = ("loss_ls", "acc_expert", "acc_agent", "prob_agent", "abs_logit_agent", "grad_penalty", "logit_reg", "weight_decay")


def disc_workspace_layout(S: int, H1: int, H2: int, n_expert: int, n_agent: int) -> dict:
    """{name: (byte offset, dtype, shape)} of what dm_train_disc_grad leaves in its workspace (include/dm_hip.h): the pieces of `workspace_layout` for all rows, then the
    penalty's stages on the expert rows; "bytes": the total"""
    n, ne, K1 = n_expert + n_agent, n_expert, (S + 63) // 64 * 64
    out = workspace_layout(H1, H2, 1, n)
    at = out.pop("bytes")
    for name, dt, shape in (("g2", np.uint16, (ne, H2)), ("g1", np.uint16, (ne, H1)), ("a", np.uint16, (ne, K1)), ("t1", np.uint16, (ne, H1)), ("t2", np.uint16, (ne, H2)),
                            ("sq", np.float32, (ne, K1 // 32)), ("wn", np.float64, (64, 2))):
        out[name] = (at, dt, shape); at += (int(np.prod(shape)) * np.dtype(dt).itemsize + 15) // 16 * 16
    out["bytes"] = at
    return out


def disc_workspace_bytes(policy, n_expert: int, n_agent: int) -> int:
    return _int_call(policy, "dm_train_disc_workspace_bytes", n_expert, n_agent)


def disc_grad_device(policy, params_ptr: int, expert_ptr: int, n_expert: int, agent_ptr: int, n_agent: int, grads_ptr: int, stats_ptr: int, workspace_ptr: int,
                     workspace_nbytes: int, grad_penalty: float = 10.0, logit_reg: float = 0.05, logits_ptr: int = 0, stream: int = 0):
    """raw device pointers (ints): the two observation batches [n_expert, S] and [n_agent, S], stats double[8] (DISC_STATS), logits [n_expert + n_agent] optional,
    expert rows first; asynchronous on `stream`"""
    _need(policy, "dm_train_disc_grad")
    cfg = _DiscCfg(float(grad_penalty), float(logit_reg))
    check(policy.lib, policy.lib.dm_train_disc_grad(policy.h, vp(params_ptr), vp(expert_ptr), int(n_expert), vp(agent_ptr), int(n_agent), C.cast(C.pointer(cfg), C.c_void_p),
                                                    vp(grads_ptr), vp(stats_ptr), vp(logits_ptr), vp(workspace_ptr), int(workspace_nbytes), vp(stream)))


class DiscTrainer(_Trainer):
    """The discriminator's update on the context of a `heads.Discriminator` (`from_policy(disc.net, weights, ...)`; weight_decay is DiscWeightDecay).
    stats(): float64[8] in the order of DISC_STATS = STATS -- the least-squares loss, acc_expert, acc_agent, mean sigmoid(y) and mean |y| over the agent rows, the gradient
    penalty 0.5 mean_e |dy/dx|^2, 0.5 |w3|^2, 0.5 sum_k |W_k|^2; `stat(name)` picks one, `loss()` is the reference's Disc_Loss."""
    N_STATS = 8
    STATS = DISC_STATS

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        _need(self.policy, "dm_train_disc_grad")
        self._coef = (0.0, 0.0)

    def grad(self, expert_obs, agent_obs, grad_penalty: float = 10.0, logit_reg: float = 0.05, logits_out=None):
        import torch
        ne = int(expert_obs.shape[0]) if expert_obs.dim() == 2 else -1
        na = int(agent_obs.shape[0]) if agent_obs.dim() == 2 else -1
        tensor_arg("expert_obs", expert_obs, self.device, torch.float32, [(ne, self.policy.S)])
        tensor_arg("agent_obs", agent_obs, self.device, torch.float32, [(na, self.policy.S)])
        if logits_out is not None:
            tensor_arg("logits_out", logits_out, self.device, torch.float32, [(ne + na,)])
        ws, nbytes = self._workspace(disc_workspace_bytes, ne, na)
        disc_grad_device(self.policy, self.params.data_ptr(), expert_obs.data_ptr(), ne, agent_obs.data_ptr(), na, self.grads.data_ptr(), self._stats.data_ptr(), ws, nbytes,
                         grad_penalty, logit_reg, 0 if logits_out is None else logits_out.data_ptr(), self._stream())
        self._coef = (float(grad_penalty), float(logit_reg))

    def stat(self, name: str):
        return self._stats[self.STATS.index(name)]

    def loss(self):
        """Disc_Loss of the last grad call (a 0-dim float64 device tensor): least squares + DiscWeightDecay 0.5 sum |W_k|^2 + logit_reg 0.5 |w3|^2 + grad_penalty penalty"""
        s = self._stats
        return s[0] + self.weight_decay * s[7] + self._coef[1] * s[6] + self._coef[0] * s[5]


# ---- numpy statements of the arithmetic (host; the tests hold the kernels to them)

def bf16_bits(x) -> np.ndarray:
    """round-to-nearest-even bf16 of float32 values, as uint16 bits; a NaN stays a quiet NaN"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    return bf16_value(bf16_bits(x))


def fma32(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays, one rounding: the product is exact in float64, the sum is rounded to odd there (Boldo-Melquiond), then to float32"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def reference_exp(x) -> np.ndarray:
    """dm_train.h exp_det, operation by operation, in float32"""
    f = np.float32
    x = np.asarray(x, dtype=f)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        xc = np.minimum(np.maximum(x, f(-104.0)), f(89.0))
        xc = np.where(np.isnan(x), f(0), xc)
        kf = np.rint(xc * f(1.44269504088896341))
        r = fma32(kf, f(-0.693359375), xc); r = fma32(kf, f(2.12194440e-4), r)
        p = fma32(r, f(1.9875691500e-4), f(1.3981999507e-3))
        for coef in (8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = fma32(p, r, f(coef))
        y = fma32(p, r * r, r) + f(1.0)
        out = np.ldexp(y, kf.astype(np.int32)).astype(f)
        return np.where(np.isnan(x), x, out)


def _tree16(v):
    """the sum over the last axis (16 lanes) as the xor butterfly takes it: adjacent pairs, four times; float32"""
    for _ in range(4):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lane_sum(terms, N3: int):
    """sum over the N3 columns (zeros in the padding) as k_train_head takes it: lane c adds its columns c, 16 + c, .. ascending, then the tree over c; float32"""
    t = terms.reshape(terms.shape[:-1] + (N3 // 16, 16))
    s = np.zeros(t.shape[:-2] + (16,), np.float32)
    for b in range(N3 // 16):
        s = s + t[..., b, :]
    return _tree16(s)


def reference_actor_head(z3, actions, old_logp, adv, a_mean, a_std, logstd, ratio_clip=0.2, bound_weight=10.0, a_bound_min=None, a_bound_max=None):
    """The actor head on given z3 [n, >= A] float32 (the padding columns are ignored), every operation in float32 as k_train_head orders it: dict(dz3 [n, N3] uint16 bf16 bits,
    logp [n], g [n], ratio [n], stats float64[6]).  Exact: the kernel's bits on the same z3."""
    f = np.float32
    n, A = actions.shape
    N3 = (A + 31) // 32 * 32
    mu = np.zeros((n, N3), f); mu[:, :A] = np.asarray(z3, f)[:, :A]
    a_mean, a_std, logstd = (np.asarray(v, f) for v in (a_mean, a_std, logstd))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = (np.asarray(actions, f) - a_mean) / a_std
        sg = reference_exp(logstd)
        u = np.zeros((n, N3), f); u[:, :A] = (x - mu[:, :A]) / sg
        # q: per lane fmaf(u, u, q) over its columns ascending, then the tree
        ub = u.reshape(n, N3 // 16, 16)
        q = np.zeros((n, 16), f)
        for b in range(N3 // 16):
            live = (16 * b + np.arange(16)) < A
            q = np.where(live, fma32(ub[:, b], ub[:, b], q), q)
        q = _tree16(q)
        ls = np.zeros(N3, f); ls[:A] = logstd
        sls = _lane_sum(ls, N3)
        cst = (f(-0.5) * f(A)) * LN_2PI - sls
        logp = fma32(f(-0.5), q, cst)
        ratio = reference_exp(logp - np.asarray(old_logp, f))
        eps = f(ratio_clip); lo_c, hi_c = f(1.0) - eps, f(1.0) + eps
        adv = np.asarray(adv, f); nf = f(n)
        l0 = adv * ratio; l1 = adv * np.minimum(np.maximum(ratio, lo_c), hi_c)
        first = ~(l0 > l1)
        g = np.where(first, -(l0 / nf), f(0)).astype(f)
        dz = (g[:, None] * (u[:, :A] / sg)).astype(f)
        viol = np.zeros(n)
        if a_bound_min is not None:
            lo = (np.asarray(a_bound_min, f) - a_mean) / a_std; hi = (np.asarray(a_bound_max, f) - a_mean) / a_std
            vlo = np.minimum(mu[:, :A] - lo, f(0)); vhi = np.maximum(mu[:, :A] - hi, f(0))
            dz = fma32(f(bound_weight) / nf, vlo + vhi, dz)
            viol = (vlo.astype(np.float64) ** 2 + vhi.astype(np.float64) ** 2).sum(axis=1)
        bits = np.zeros((n, N3), np.uint16); bits[:, :A] = bf16_bits(dz)
        dn = float(n)
        stats = np.array([dn, -(np.where(first, l0, l1).astype(np.float64).sum() / dn), 0.5 * viol.sum() / dn,
                          (np.abs(ratio - f(1.0)) > eps).sum() / dn, ratio.astype(np.float64).sum() / dn, logp.astype(np.float64).sum() / dn])
    return dict(dz3=bits, logp=logp, g=g, ratio=ratio, stats=stats)


def reference_value_head(z3, targets):
    """the critic head on given z3 [n, >= 1]: dict(dz3 [n, 32] bf16 bits, values [n], stats float64[2])"""
    f = np.float32
    v = np.asarray(z3, f)[:, 0]; n = v.shape[0]
    e = v - np.asarray(targets, f)
    bits = np.zeros((n, 32), np.uint16); bits[:, 0] = bf16_bits(e / f(n))
    return dict(dz3=bits, values=v, stats=np.array([0.5 * (e.astype(np.float64) ** 2).sum() / n, v.astype(np.float64).sum() / n]))


def reference_forward_bf16(weights: dict, states, s_clip=np.inf):
    """s16 [n, S], h1, h2 as bf16 VALUES (float32) and z3 [n, A] float32 of the plain actor: the rounding points of the device forward, float64 accumulation"""
    f = np.float32
    s = np.asarray(states, f)
    sm, ss = weights.get("s_mean"), weights.get("s_std")
    x = (s - (f(0) if sm is None else np.asarray(sm, f))) * (f(1) / (f(1) if ss is None else np.asarray(ss, f)))
    s16 = bf16_round(np.clip(x, -s_clip, s_clip))
    lin = lambda h, w, b: (h.astype(np.float64) @ bf16_round(weights[w]).astype(np.float64)).astype(f) + np.asarray(weights[b], f)
    h1 = bf16_round(np.maximum(lin(s16, "w1", "b1"), f(0)))
    h2 = bf16_round(np.maximum(lin(h1, "w2", "b2"), f(0)))
    return s16, h1, h2, lin(h2, "w3", "b3")


def reference_backward(weights: dict, s16, h1, h2, dz3_bits):
    """the backward pass from bf16 dz3 [n, N3] (bits) and the saved bf16 activations (values): dict(grads float32 [P], dz2, dz1 bf16 bits); float64 accumulation"""
    f = np.float32
    A = np.asarray(weights["w3"]).shape[1]
    dz3 = bf16_value(dz3_bits)[:, :A].astype(np.float64)
    g = {}
    g["w3"] = h2.astype(np.float64).T @ dz3; g["b3"] = dz3.sum(axis=0)
    dz2_bits = bf16_bits(np.where(h2 != 0, (dz3 @ bf16_round(weights["w3"]).astype(np.float64).T).astype(f), f(0)))
    dz2 = bf16_value(dz2_bits).astype(np.float64)
    g["w2"] = h1.astype(np.float64).T @ dz2; g["b2"] = dz2.sum(axis=0)
    dz1_bits = bf16_bits(np.where(h1 != 0, (dz2 @ bf16_round(weights["w2"]).astype(np.float64).T).astype(f), f(0)))
    dz1 = bf16_value(dz1_bits).astype(np.float64)
    g["w1"] = s16.astype(np.float64).T @ dz1; g["b1"] = dz1.sum(axis=0)
    return dict(grads=_block_pack(KEYS, g), dz2=dz2_bits, dz1=dz1_bits)


def _reference_head(z3, head: str, weights: dict, kw: dict) -> dict:
    """the head of a *_grad call on z3 at the device's rounding points: reference_actor_head with a_mean / a_std / logstd from the weights (absent: 0 / 1 / 0), or
    reference_value_head"""
    if head != "actor":
        return reference_value_head(z3, **kw)
    dflt = lambda k, v: np.full(z3.shape[1], v, np.float32) if weights.get(k) is None else weights[k]
    return reference_actor_head(z3, a_mean=dflt("a_mean", 0), a_std=dflt("a_std", 1), logstd=dflt("logstd", 0), **kw)


def reference_grad(weights: dict, states, head: str, s_clip=np.inf, **kw):
    """The whole *_grad call in numpy.  head "actor": kw = actions, old_logp, adv[, ratio_clip, bound_weight, a_bound_min, a_bound_max] (a_mean, a_std, logstd from the
    weights); head "critic": kw = targets.  `states` holds the goal columns.  dict(grads, stats, dz3, dz2, dz1, z3, s16, h1, h2 and the head's own outputs)."""
    s16, h1, h2, z3 = reference_forward_bf16(weights, states, s_clip)
    hd = _reference_head(z3, head, weights, kw)
    out = dict(hd); out.update(reference_backward(weights, s16, h1, h2, hd["dz3"]))
    out.update(z3=z3, s16=s16, h1=h1, h2=h2)
    return out


def reference_step(params, momentum, grads, stepsize, mom, weight_decay=0.0, grad_scale=1.0, matrix_mask=None, exact=True):
    """The momentum step per element: g = grad_scale grad (+ weight_decay w on the entries of matrix_mask, `matrix_mask_of`) and v = mom v + g in float64, where the
    products of float32 values are exact, v rounded to float32 once; then the master from the stored v.  exact: w = fmaf(-stepsize, v, w), the kernel's bits; else
    w - stepsize v in float64, rounded once.  Returns (params, momentum)."""
    f = np.float32
    w, v, g = (np.asarray(a, f) for a in (params, momentum, grads))
    mask = np.zeros(w.shape, bool) if matrix_mask is None else np.asarray(matrix_mask, bool)
    lr, mo, wd, gs = (float(f(x)) for x in (stepsize, mom, weight_decay, grad_scale))
    w64 = w.astype(np.float64)
    gg = gs * g.astype(np.float64)
    gg = np.where(mask, gg + wd * w64, gg)
    vv = (mo * v.astype(np.float64) + gg).astype(f)
    if exact:
        return fma32(f(-lr), vv, w), vv
    return (w64 - lr * vv.astype(np.float64)).astype(f), vv


def _tree_fold(x: np.ndarray) -> np.ndarray:
    """dmb::block_sum over the last axis (OPT_THREADS entries): x[t] += x[t + w], w = 128 .. 1"""
    x = np.array(x, np.float64)
    w = x.shape[-1] // 2
    while w >= 1:
        x[..., :w] = x[..., :w] + x[..., w:2 * w]
        w //= 2
    return x[..., 0]


def reference_grad_norm(grads, partition: Optional[dict] = None, grad_scale: float = 1.0):
    """k_opt_sq and the fold of k_opt_begin in their own order (partition: opt_workspace_layout(P), the default): thread t of group b adds the squares of its elements
    OPT_CHUNK b + t + OPT_THREADS k in float64, k ascending, the threads by the tree, the groups by contiguous runs per thread and the tree.
    Returns (sum, count of non-finite elements, norm = |grad_scale| sqrt(sum), the groups' (sums, counts))."""
    g = np.asarray(grads, np.float32).reshape(-1)
    G = (opt_workspace_layout(g.size) if partition is None else partition)["groups"]
    pad = np.zeros(G * OPT_CHUNK, np.float32); pad[:g.size] = g                       # (an element past P adds + 0.0: the sum keeps its bits)
    x = pad.reshape(G, OPT_CHUNK // OPT_THREADS, OPT_THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        s, bad = np.zeros((G, OPT_THREADS)), np.zeros((G, OPT_THREADS))
        for k in range(x.shape[1]):
            d = x[:, k].astype(np.float64)
            s = s + d * d
            bad = bad + ~np.isfinite(x[:, k])
        gs, gc = _tree_fold(s), _tree_fold(bad)
        per = (G + OPT_THREADS - 1) // OPT_THREADS
        def fold(part):
            runs = np.zeros(per * OPT_THREADS); runs[:G] = part
            t = np.zeros(OPT_THREADS)
            for k in range(per):
                t = t + runs.reshape(OPT_THREADS, per)[:, k]
            return float(_tree_fold(t))
        total, count = fold(gs), fold(gc)
        return total, count, float(abs(np.float64(grad_scale)) * np.sqrt(np.float64(total))), (gs, gc)


def reference_opt_begin(state, cfg: dict, total: float, count: float):
    """k_opt_begin: (the new state float64[8], dict(skip, s float32, alpha, ic2)).  cfg: kind, stepsize, beta1, beta2, grad_scale and optionally max_grad_norm,
    skip_nonfinite; total / count: of reference_grad_norm -- 0, 0 when neither clipping nor the guard is on (the norm pass does not run)"""
    d, f = np.float64, np.float32
    st = np.array(state, d)
    mx = cfg.get("max_grad_norm")
    clip = mx is not None and mx > 0 and np.isfinite(mx)
    guard = bool(cfg.get("skip_nonfinite"))
    if not (clip or guard):
        total, count = 0.0, 0.0
    B1, B2, gsc = d(f(cfg["beta1"])), d(f(cfg.get("beta2", 0.999))), d(cfg.get("grad_scale", 1.0))
    adam = OPT_KINDS.get(cfg["kind"], cfg["kind"]) == 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = abs(gsc) * np.sqrt(d(total))
        scale = d(1.0)
        if clip:
            q = d(mx) / (norm + d(1e-6))
            scale = q if (q < 1.0 or q != q) else d(1.0)
        skip = guard and count > 0
        t = st[0]
        p1, p2 = (d(1.0), d(1.0)) if t == 0 else (st[1], st[2])
        if skip:
            st[3] += 1.0
        else:
            t = t + 1.0; p1 = p1 * B1; p2 = p2 * B2
            st[0], st[1], st[2] = t, p1, p2
        st[4], st[5], st[6] = norm, scale, count
        ctrl = dict(skip=bool(skip), s=f(gsc * scale), alpha=d(cfg["stepsize"]) / (d(1.0) - p1) if adam else d(0.0), ic2=d(1.0) / (d(1.0) - p2) if adam else d(0.0))
    return st, ctrl


def reference_adam_step(params, m, v, grads, s, alpha, ic2, beta1, beta2, eps, weight_decay=0.0, matrix_mask=None):
    """k_opt_step<ADAM> per element, every written operation one float64 rounding, m', v', w' rounded once to float32: g = s grad (+ wd w on matrix_mask),
    m' = B1 m + (1 - B1) g, v' = B2 v + ((1 - B2) g) g, w' = w - (alpha m') / (sqrt(v' ic2) + eps) with the stored m', v'.  Returns (params, m, v)."""
    d, f = np.float64, np.float32
    w, m, v, g = (np.asarray(a, f) for a in (params, m, v, grads))
    mask = np.zeros(w.shape, bool) if matrix_mask is None else np.asarray(matrix_mask, bool)
    B1, B2, wd, e = (d(f(x)) for x in (beta1, beta2, weight_decay, eps))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        w64 = w.astype(d)
        gg = d(f(s)) * g.astype(d)
        gg = np.where(mask, gg + wd * w64, gg)
        m1 = (B1 * m.astype(d) + (d(1.0) - B1) * gg).astype(f)
        v1 = (B2 * v.astype(d) + (d(1.0) - B2) * gg * gg).astype(f)
        w1 = (w64 - d(alpha) * m1.astype(d) / (np.sqrt(v1.astype(d) * d(ic2)) + e)).astype(f)
    return w1, m1, v1


def reference_opt_step(state, cfg: dict, params, m, v, grads, matrix_mask=None):
    """one whole dm_train_opt_step from the three mirrors and reference_step: (params, m, v, state); v passes through with kind "momentum" (None allowed)"""
    total, count, _, _ = reference_grad_norm(grads, grad_scale=cfg.get("grad_scale", 1.0))
    st, c = reference_opt_begin(state, cfg, total, count)
    f = np.float32
    if c["skip"]:
        return np.asarray(params, f).copy(), np.asarray(m, f).copy(), None if v is None else np.asarray(v, f).copy(), st
    wd = cfg.get("weight_decay", 0.0)
    if OPT_KINDS.get(cfg["kind"], cfg["kind"]) == 1:
        return reference_adam_step(params, m, v, grads, c["s"], c["alpha"], c["ic2"], cfg["beta1"], cfg.get("beta2", 0.999), cfg.get("eps", 1e-8), wd, matrix_mask) + (st,)
    with np.errstate(invalid="ignore", over="ignore"):
        w1, m1 = reference_step(params, m, grads, cfg["stepsize"], cfg["beta1"], wd, c["s"], matrix_mask)
    return w1, m1, None if v is None else np.asarray(v, f).copy(), st


def matrix_mask_of(S: int, H1: int, H2: int, A: int) -> np.ndarray:
    return _block_matrix_mask(KEYS, layout(S, H1, H2, A))


# ---- the discriminator update in numpy

def reference_disc_head(z3, n_expert: int, n_agent: int):
    """k_train_disc_head on given z3 [n, >= 1] (expert rows first), every operation in float32 as the kernel orders it: dict(dz3 [n, 32] bf16 bits, logits [n],
    stats float64[5] = the first five of DISC_STATS).  Exact on the same z3 (the statistics up to the order of the float64 sums)."""
    f = np.float32
    y = np.asarray(z3, f)[:, 0]; n = y.shape[0]
    assert n == n_expert + n_agent
    expert = np.arange(n) < n_expert
    with np.errstate(invalid="ignore", over="ignore"):
        e = y - np.where(expert, f(1), f(-1))
        bits = np.zeros((n, 32), np.uint16); bits[:, 0] = bf16_bits((f(0.5) * e) / np.where(expert, f(n_expert), f(n_agent)))
        e2 = e.astype(np.float64) ** 2
        ya = y[~expert]
        sig = f(1) / (f(1) + reference_exp(-ya))
        de, da = float(n_expert), float(n_agent)
        stats = np.array([0.5 * (0.5 * e2[expert].sum() / de + 0.5 * e2[~expert].sum() / da), (y[expert] > 0).sum() / de, (ya < 0).sum() / da,
                          sig.astype(np.float64).sum() / da, np.abs(ya).astype(np.float64).sum() / da])
    return dict(dz3=bits, logits=y, stats=stats)


def reference_row_squares(gx, K1: int):
    """k_train_dgrad<true>'s |gx|^2 partials of fp32 gx [n, S]: per block of 32 columns (zeros behind S) lane c takes v0 v0 then fmaf(v1, v1, .) over its columns c, 16 + c,
    then the tree over c; float32 [n, K1 / 32]"""
    f = np.float32
    n, S = gx.shape
    v = np.zeros((n, K1), f); v[:, :S] = gx
    v = v.reshape(n, K1 // 32, 2, 16)
    with np.errstate(over="ignore", invalid="ignore"):
        return _tree16(fma32(v[:, :, 1], v[:, :, 1], v[:, :, 0] * v[:, :, 0]))


def reference_disc_penalty(weights: dict, h1, h2, grad_penalty: float):
    """The penalty path on the saved bf16 activations of the EXPERT rows (values): dict(g2, g1, a [n_e, K1], t1, t2 as bf16 bits, gx float32 [n_e, S], sq float32
    [n_e, K1 / 32], w1, w2, w3: the penalty's own gradient contributions in float32); the rounding points of include/dm_hip.h, contractions in float64"""
    f, d = np.float32, np.float64
    S = np.asarray(weights["w1"]).shape[0]; K1 = (S + 63) // 64 * 64
    ne = h1.shape[0]
    W1, W2 = bf16_round(weights["w1"]).astype(d), bf16_round(weights["w2"]).astype(d)
    w3 = bf16_round(np.asarray(weights["w3"], f).reshape(-1))
    with np.errstate(over="ignore", invalid="ignore"):
        g2 = np.where(h2 != 0, w3[None, :], f(0)).astype(f)
        g1 = bf16_round(np.where(h1 != 0, (g2.astype(d) @ W2.T).astype(f), f(0)))
        gx = (g1.astype(d) @ W1.T).astype(f)
        a = np.zeros((ne, K1), f); a[:, :S] = bf16_round(gx * (f(grad_penalty) / f(ne)))
        t1 = bf16_round(np.where(h1 != 0, (a[:, :S].astype(d) @ W1).astype(f), f(0)))
        t2 = bf16_round(np.where(h2 != 0, (t1.astype(d) @ W2).astype(f), f(0)))
        out = dict(g2=bf16_bits(g2), g1=bf16_bits(g1), a=bf16_bits(a), t1=bf16_bits(t1), t2=bf16_bits(t2), gx=gx, sq=reference_row_squares(gx, K1),
                   w1=(a[:, :S].astype(d).T @ g1.astype(d)).astype(f), w2=(t1.astype(d).T @ g2.astype(d)).astype(f), w3=t2.astype(d).sum(axis=0).astype(f))
    return out


def reference_disc_grad(weights: dict, expert_obs, agent_obs, grad_penalty: float = 10.0, logit_reg: float = 0.05, s_clip=np.inf):
    """The whole dm_train_disc_grad call in numpy: dict(grads, stats float64[8], logits, z3, s16, h1, h2, dz3, dz2, dz1 and, with a penalty, g2, g1, gx, sq, a, t1, t2).
    Rounding order of a gradient element: the least-squares value, + the penalty value (one float32 add), then on w3 fmaf(logit_reg, w3, .)."""
    f, d = np.float32, np.float64
    ne, na = np.asarray(expert_obs).shape[0], np.asarray(agent_obs).shape[0]
    w = dict(weights); w["w3"] = np.asarray(w["w3"], f).reshape(-1, 1); w["b3"] = np.asarray(w["b3"], f).reshape(1)
    s16, h1, h2, z3 = reference_forward_bf16(w, np.concatenate([np.asarray(expert_obs, f), np.asarray(agent_obs, f)]), s_clip)
    hd = reference_disc_head(z3, ne, na)
    out = dict(hd); out.update(reference_backward(w, s16, h1, h2, hd["dz3"]))
    out.update(z3=z3, s16=s16, h1=h1, h2=h2)
    S, H1 = w["w1"].shape; H2 = w["w2"].shape[1]
    g = {k: v.copy() for k, v in unpack_params(out["grads"].copy(), S, H1, H2, 1).items()}
    pen_stat = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        if grad_penalty > 0:
            pen = reference_disc_penalty(w, h1[:ne], h2[:ne], grad_penalty)
            out.update({k: pen[k] for k in ("g2", "g1", "gx", "sq", "a", "t1", "t2")})
            g["w1"] = g["w1"] + pen["w1"]; g["w2"] = g["w2"] + pen["w2"]; g["w3"] = g["w3"] + pen["w3"].reshape(-1, 1)
            pen_stat = 0.5 * pen["sq"].astype(d).sum() / float(ne)
        elif logit_reg > 0:
            g["w3"] = g["w3"] + f(0)
        if logit_reg > 0:
            g["w3"] = fma32(f(logit_reg), w["w3"], g["w3"])
    out["grads"] = _block_pack(KEYS, g)
    sqs = {k: (np.asarray(w[k], f).astype(d) ** 2).sum() for k in ("w1", "w2", "w3")}
    out["stats"] = np.concatenate([hd["stats"], [pen_stat, 0.5 * sqs["w3"], 0.5 * (sqs["w1"] + sqs["w2"] + sqs["w3"])]])
    return out


# ---- the gated update in numpy

def reference_gated_forward_bf16(weights: dict, states, s_clip=np.inf, rounded=True):
    """The forward pass of the gated net at the rounding points of dm_policy.h GateDev, contractions in float64: dict(s16 [n, S], xg [n, G], c, e0, e1, h1, h2 -- bf16 VALUES
    --, sigma0, beta0, u0, sigma1, beta1, u1 (u_i = W_i h + b_i as the gate split recomputes it) and z3 [n, A], float32).  sigma uses numpy's exp: the platform's, like the
    device's own expf, so it is the device's bits only where sigma is exactly 0, 1 or 2.  rounded=False: nothing is rounded, every array float64."""
    d = np.float64
    f = np.float32 if rounded else d
    R = bf16_round if rounded else (lambda x: np.asarray(x, d))
    F = lambda x: np.asarray(x).astype(f)
    S, G = np.shape(weights["w1"])[0], int(weights["goal_dim"])
    sm, ss = weights.get("s_mean"), weights.get("s_std")
    inv_std = np.float32(1) / (np.float32(1) if ss is None else np.asarray(ss, np.float32))        # the context holds 1 / s_std as a float32 array: a parameter, not a rounding point
    x = (F(states) - (f(0) if sm is None else F(sm))) * F(inv_std)
    out = dict(s16=R(np.clip(x, -s_clip, s_clip)))
    out["xg"] = out["s16"][:, S - G:]
    # one dense layer: the float64 contraction of (bf16) operands rounded to float32, then the bias by one float32 add
    dense = lambda h, wk, bk: F(np.asarray(h, d) @ np.asarray(R(weights[wk]), d)) + F(weights[bk])
    gate = lambda h, k: dense(h, k + "_w", k + "_b")
    out["c"] = R(np.maximum(gate(out["xg"], "gc"), f(0)))
    h = out["s16"]
    for i in (0, 1):
        e = R(np.maximum(gate(out["c"], "g%d" % i), f(0)))
        beta = gate(e, "g%d_bias" % i)
        with np.errstate(over="ignore"):
            sigma = F(f(2) / (f(1) + np.exp(-gate(e, "g%d_scale" % i))))
        u = dense(h, "w%d" % (i + 1), "b%d" % (i + 1))
        p = fma32(sigma, u, beta) if rounded else sigma * u + beta
        h = R(np.maximum(p, f(0)))
        out.update({"e%d" % i: e, "beta%d" % i: beta, "sigma%d" % i: sigma, "u%d" % i: u, "h%d" % (i + 1): h})
    out["z3"] = dense(h, "w3", "b3")
    return out


def reference_gate_split(dp, u, sigma, rounded=True):
    """k_train_gate_split per element: (du, da) = (bf16(dp sigma), bf16((dp u) ds)) with ds = sigma fmaf(-0.5, sigma, 1), every operation in float32, as bf16 VALUES;
    rounded=False: the same algebra in float64"""
    if not rounded:
        dp, u, sigma = (np.asarray(v, np.float64) for v in (dp, u, sigma))
        return dp * sigma, dp * u * (sigma * (1.0 - 0.5 * sigma))
    f = np.float32
    dp, u, sigma = (np.asarray(v, f) for v in (dp, u, sigma))
    with np.errstate(invalid="ignore", over="ignore"):
        ds = sigma * fma32(f(-0.5), sigma, f(1.0))
        return bf16_round(dp * sigma), bf16_round((dp * u) * ds)


def reference_gated_backward(weights: dict, fwd: dict, dz3, rounded=True):
    """The backward pass from dz3 [n, A] (values) and the arrays of reference_gated_forward_bf16: dict(grads {key: array} over GATED_KEYS, and the stages dp1, dp0, du1, du0,
    da1, da0, dze0, dze1, dzc as values); contractions in float64, results float32 and the stages bf16 where the device stores them (rounded=False: float64 throughout)"""
    d = np.float64
    f = np.float32 if rounded else d
    R = bf16_round if rounded else (lambda x: np.asarray(x, d))
    W = lambda k: np.asarray(R(weights[k]), d)
    mm = lambda a, b: np.asarray(a, d) @ np.asarray(b, d)
    # bf16((sum of dz W^T over the pairs) . [h != 0]): one float64 contraction, rounded to float32, masked, rounded to bf16
    back = lambda h, *pairs: R(np.where(h != 0, sum(mm(dz, W(k).T) for dz, k in pairs).astype(f), f(0)))
    g, st = {}, {}
    def wb(wk, bk, a, dz):
        g[wk] = mm(np.asarray(a).T, dz).astype(f); g[bk] = np.asarray(dz, d).sum(axis=0).astype(f)
    dz3 = np.asarray(dz3, d)
    wb("w3", "b3", fwd["h2"], dz3)
    st["dp1"] = back(fwd["h2"], (dz3, "w3"))
    st["du1"], st["da1"] = reference_gate_split(st["dp1"], fwd["u1"], fwd["sigma1"], rounded)
    wb("w2", "b2", fwd["h1"], st["du1"])
    st["dp0"] = back(fwd["h1"], (st["du1"], "w2"))
    st["du0"], st["da0"] = reference_gate_split(st["dp0"], fwd["u0"], fwd["sigma0"], rounded)
    wb("w1", "b1", fwd["s16"], st["du0"])
    for i in (0, 1):
        e, dp, da = fwd["e%d" % i], st["dp%d" % i], st["da%d" % i]
        wb("g%d_bias_w" % i, "g%d_bias_b" % i, e, dp)
        wb("g%d_scale_w" % i, "g%d_scale_b" % i, e, da)
        st["dze%d" % i] = back(e, (dp, "g%d_bias_w" % i), (da, "g%d_scale_w" % i))
        wb("g%d_w" % i, "g%d_b" % i, fwd["c"], st["dze%d" % i])
    st["dzc"] = back(fwd["c"], (st["dze0"], "g0_w"), (st["dze1"], "g1_w"))
    wb("gc_w", "gc_b", fwd["xg"], st["dzc"])
    return dict(st, grads=g)


def _head64(z3, head: str, weights: dict, kw: dict):
    """the heads in float64, nothing rounded: dz3 [n, A] of the PPO surrogate + bound loss (actor) or of 0.5 MSE (critic)"""
    d = np.float64
    z3 = np.asarray(z3, d); n, A = z3.shape
    if head != "actor":
        return (z3 - np.asarray(kw["targets"], d)[:, None]) / n
    dflt = lambda k, v: np.full(A, v, d) if weights.get(k) is None else np.asarray(weights[k], d)
    mean, std, sg = dflt("a_mean", 0), dflt("a_std", 1), np.exp(dflt("logstd", 0))
    u = ((np.asarray(kw["actions"], d) - mean) / std - z3) / sg
    logp = -0.5 * (u ** 2).sum(axis=1) - 0.5 * A * np.log(2 * np.pi) - np.log(sg).sum()
    ratio, adv, eps = np.exp(logp - np.asarray(kw["old_logp"], d)), np.asarray(kw["adv"], d), kw.get("ratio_clip", 0.2)
    l0, l1 = adv * ratio, adv * np.clip(ratio, 1 - eps, 1 + eps)
    dz = np.where(~(l0 > l1), -(l0 / n), 0.0)[:, None] * (u / sg)
    if kw.get("a_bound_min") is not None:
        lo, hi = (np.asarray(kw["a_bound_min"], d) - mean) / std, (np.asarray(kw["a_bound_max"], d) - mean) / std
        dz = dz + kw.get("bound_weight", 10.0) / n * (np.minimum(z3 - lo, 0) + np.maximum(z3 - hi, 0))
    return dz


def reference_gated_grad(weights: dict, states, head: str, s_clip=np.inf, rounded=True, **kw):
    """The whole dm_train_gated_*_grad call in numpy (kw as reference_grad; `states` holds the goal columns): the arrays of reference_gated_forward_bf16 and
    reference_gated_backward, `grads` also flat as "flat" [P], and with rounded=True the head's own outputs (dz3 bits, logp / values, stats).  rounded=False drops every
    bf16 and float32 rounding -- the algebra alone, for a check against autograd."""
    out = reference_gated_forward_bf16(weights, states, s_clip, rounded)
    if not rounded:
        dz3 = _head64(out["z3"], head, weights, kw)
    else:
        hd = _reference_head(out["z3"], head, weights, kw)
        out.update(hd)
        dz3 = bf16_value(hd["dz3"])[:, :out["z3"].shape[1]]
    out.update(reference_gated_backward(weights, out, dz3, rounded))
    out["flat"] = _block_pack(GATED_KEYS, out["grads"], dtype=None)
    return out


def gated_matrix_mask_of(S: int, H1: int, H2: int, A: int, G: int, GC: int, GH: int) -> np.ndarray:
    """the entries of a gated block under the weight decay: its ten matrices"""
    return _block_matrix_mask(GATED_KEYS, gated_layout(S, H1, H2, A, G, GC, GH))
