"""Scalar heads of the device nets: the critic and the AMP discriminator evaluated on device buffers (ctypes binding of `dm_policy_eval_scalar`,
include/dm_hip.h; kernels: the HEAD = 1 instantiations of deepmimic_amd/csrc/dm_policy.h).

Both are the actor's two-layer MLP with ONE output column and another last step, finished in the launch that evaluates the net:

* `Critic` (learning/pg_agent.py:161-171, gated in the AMP task agents): v = clip(y, lo, hi) (learning/amp_agent.py:441-443; no bounds: PPO), then val_fail /
  val_succ where `terminate` is Fail (1) / Succ (2) (learning/ppo_agent.py:262-264);
* `Discriminator` (learning/amp_agent.py:178-194, on amp_obs_norm-normalised `info["amp_obs"]`): r = reward_scale * max(0, 1 - 0.25 (1 - y)^2), then
  (1 - task_reward_lerp) r + task_reward_lerp * task_r with a task reward (amp_agent.py:294-297, 393-434).

`row_mask` (int32 per row) switches rows off: they get `fill`, and in the one-launch kernel (reference widths) a whole 32-row tile of them leaves before its
first weight request -- critic values on `info["terminal_obs"]` are read only where the step was done.  On the per-layer route (other widths,
DM_POLICY_LAYERED=1) only the last launch honours the mask: layers 1 and 2 still run for every row.  `raw=True` also hands back y (the discriminator's
logit).  A head holds a `Policy` context with action_dim = 1, so `set_weights*` refresh it in place after an optimiser step like the actor.  No CPU fallback.
"""
import ctypes as C
from typing import Optional

import numpy as np

from .binding import check, stream_handle, tensor_arg, vp
from .policy import Policy, is_gated

VALUE, STYLE = 0, 1          # include/dm_hip.h DM_SCALAR_HEAD_VALUE / DM_SCALAR_HEAD_STYLE
TERM_FAIL, TERM_SUCC = 1, 2  # eTerminate


class _ScalarHead(C.Structure):
    _fields_ = [("kind", C.c_int), ("lo", C.c_float), ("hi", C.c_float), ("val_fail", C.c_float), ("val_succ", C.c_float), ("terminate_dev", C.c_void_p),
                ("scale", C.c_float), ("lerp", C.c_float), ("task_reward_dev", C.c_void_p), ("row_mask_dev", C.c_void_p), ("fill", C.c_float)]


class _ScalarNet:
    """one net with a single output on the device: weights as `Policy` takes them with w3 [H2, 1], b3 [1]; a_mean / a_std / logstd are not part of it"""

    def __init__(self, weights: dict, device_id: int = 0, s_clip: float = 0.0, lib_path: Optional[str] = None):
        w = {k: v for k, v in weights.items() if k not in ("a_mean", "a_std", "logstd")}
        w["w3"] = np.asarray(w["w3"], dtype=np.float32).reshape(np.asarray(w["w2"]).shape[1], -1)
        w["b3"] = np.asarray(w["b3"], dtype=np.float32).reshape(-1)
        if w["w3"].shape[1] != 1 or w["b3"].shape != (1,):
            raise ValueError("a scalar head needs one output unit: w3 is %s, b3 %s" % (w["w3"].shape, w["b3"].shape))
        self.net = Policy(w, device_id=device_id, s_clip=s_clip, lib_path=lib_path)
        self.lib = self.net.lib
        if not hasattr(self.lib, "dm_policy_eval_scalar"):
            raise RuntimeError("libdm_hip: this library has no dm_policy_eval_scalar (rebuild it)")
        self.device_id, self.S, self.gated = self.net.device_id, self.net.S, self.net.gated

    @staticmethod
    def _checkpoint_weights(w: dict) -> dict:
        if "g_mean" in w:
            w["s_mean"] = np.concatenate([w["s_mean"], w.pop("g_mean")]); w["s_std"] = np.concatenate([w["s_std"], w.pop("g_std")])
        return w

    def _head(self, **kw) -> _ScalarHead:
        raise NotImplementedError

    def _eval(self, head: _ScalarHead, states_ptr, n, out_ptr, goals_ptr, goal_dim, raw_ptr, stream):
        check(self.lib, self.lib.dm_policy_eval_scalar(self.net.h, vp(states_ptr), vp(goals_ptr), int(goal_dim), int(n), C.byref(head), vp(out_ptr), vp(raw_ptr),
                                                       vp(stream)))

    def eval_device(self, states_ptr: int, n: int, out_ptr: int, goals_ptr: int = 0, goal_dim: int = 0, raw_ptr: int = 0, row_mask_ptr: int = 0, fill: float = 0.0,
                    stream: int = 0, **rows):
        """raw device pointers (ints); out / raw [n] float32, row_mask [n] int32; **rows: the head's per-row inputs as pointers (`terminate_ptr` for the critic,
        `task_reward_ptr` for the discriminator).  Asynchronous on the HIP stream `stream` (0 = the null stream)."""
        self._eval(self._head(row_mask=row_mask_ptr, fill=fill, **rows), states_ptr, n, out_ptr, goals_ptr, goal_dim, raw_ptr, stream)

    def eval_torch(self, states, goals=None, row_mask=None, fill: float = 0.0, raw: bool = False, stream=None, **rows):
        """torch tensors on the head's device; leading dimensions are rows (`[T, N, S]` is T * N rows).  row_mask and the per-row inputs (`terminate`,
        `task_reward`) have the leading shape; a bool mask is converted.  Returns out, or (out, raw_y), of the leading shape, on torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device_id)
        lead = tuple(states.shape[:-1]); n = int(np.prod(lead, dtype=np.int64)) if lead else 1

        def flat(name, x, dtype, width=None):
            if x is None:
                return None
            if dtype == torch.int32 and x.dtype == torch.bool:
                x = x.to(torch.int32)
            return tensor_arg(name, x, dev, dtype, [lead + ((width,) if width is not None else ())], contiguous=False).contiguous()
        G = 0 if goals is None else int(goals.shape[-1])
        s = flat("states", states, torch.float32, self.S - G); g = flat("goals", goals, torch.float32, G)
        m = flat("row_mask", row_mask, torch.int32)
        per_row = {k + "_ptr": flat(k, v, torch.int32 if k == "terminate" else torch.float32) for k, v in rows.items()}
        out = torch.empty(lead, dtype=torch.float32, device=dev); y = torch.empty(lead, dtype=torch.float32, device=dev) if raw else None
        if n:
            self.eval_device(s.data_ptr(), n, out.data_ptr(), 0 if g is None else g.data_ptr(), G, 0 if y is None else y.data_ptr(), 0 if m is None else m.data_ptr(),
                             fill, stream_handle(dev, stream), **{k: (0 if t is None else t.data_ptr()) for k, t in per_row.items()})
        return (out, y) if raw else out

    def eval_host(self, states, goals=None, row_mask=None, fill: float = 0.0, **rows):
        """emulator-build convenience ("device" memory is host memory): numpy in, (out, raw_y) out"""
        s = np.ascontiguousarray(states, dtype=np.float32); n = s.shape[0]
        g = None if goals is None else np.ascontiguousarray(goals, dtype=np.float32)
        m = None if row_mask is None else np.ascontiguousarray(row_mask, dtype=np.int32)
        keep = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.int32 if k == "terminate" else np.float32)) for k, v in rows.items()}
        out = np.zeros(n, np.float32); y = np.zeros(n, np.float32)
        self.eval_device(s.ctypes.data, n, out.ctypes.data, 0 if g is None else g.ctypes.data, 0 if g is None else g.shape[1], y.ctypes.data,
                         0 if m is None else m.ctypes.data, fill, 0, **{k + "_ptr": (0 if v is None else v.ctypes.data) for k, v in keep.items()})
        return out, y

    def info(self) -> dict:
        """dm_policy_scalar_info: the dm_policy_path id that served the last eval (-1 before any), its rows, head kind and whether it was masked; plus the
        context's own dm_policy_info under "net" """
        out = (C.c_int32 * 4)()
        check(self.lib, self.lib.dm_policy_scalar_info(self.net.h, out))
        return dict(path=int(out[0]), rows=int(out[1]), kind=int(out[2]), masked=bool(out[3]), net=self.net.info())

    # new weights into the live context: the actor's calls on the underlying context (keys of the constructor; a_mean / a_std / logstd do not exist here)
    def weight_shapes(self, out_in: bool = False) -> dict:
        return {k: v for k, v in self.net.weight_shapes(out_in).items() if k not in ("a_mean", "a_std", "logstd")}

    def set_weights(self, weights: dict):
        self.net.set_weights(weights)

    def set_weights_device(self, ptrs: dict, out_in: bool = False, stream: int = 0):
        self.net.set_weights_device(ptrs, out_in, stream)

    def set_weights_torch(self, tensors: dict, layout: str = "in_out", stream=None):
        self.net.set_weights_torch(tensors, layout, stream)

    def close(self):
        self.net.close()


class Critic(_ScalarNet):
    """weights: the `Policy` dict of the critic net (w1 [S + G, H1] ... w3 [H2, 1], b3 [1], s_mean / s_std over state and goal columns; with GATE_KEYS and
    "goal_dim" the gated critic).  lo / hi: the value clip (None: none); val_fail / val_succ: what a Fail / Succ row gets when `terminate` is given."""

    def __init__(self, weights: dict, lo: Optional[float] = None, hi: Optional[float] = None, val_fail: float = 0.0, val_succ: float = 0.0, **kw):
        super().__init__(weights, **kw)
        self.lo = -np.inf if lo is None else float(lo); self.hi = np.inf if hi is None else float(hi)
        self.val_fail, self.val_succ = float(val_fail), float(val_succ)

    @classmethod
    def from_checkpoint(cls, prefix: str, state_dim: Optional[int] = None, **kw):
        """the critic of a reference checkpoint (plain or gated: the index decides), s_norm / g_norm as its input normaliser"""
        from . import tf_checkpoint
        return cls(cls._checkpoint_weights(tf_checkpoint.critic_weights(prefix, state_dim=state_dim)), **kw)

    def _head(self, row_mask=0, fill=0.0, terminate_ptr=0):
        return _ScalarHead(VALUE, self.lo, self.hi, self.val_fail, self.val_succ, terminate_ptr or None, 0.0, 0.0, None, row_mask or None, float(fill))


class Discriminator(_ScalarNet):
    """weights: the plain `Policy` dict of the discriminator (w1 [amp_obs_size, H1] ... w3 [H2, 1], b3 [1], s_mean / s_std = amp_obs_norm).
    reward_scale, task_reward_lerp: the agent's RewardScale and TaskRewardLerp (None: style reward only; a task reward passed to eval is then refused)."""

    def __init__(self, weights: dict, reward_scale: float = 1.0, task_reward_lerp: Optional[float] = None, **kw):
        if is_gated(weights):
            raise ValueError("the AMP discriminator is the plain fc_2layers_1024units net: no gate arrays")
        super().__init__(weights, **kw)
        self.reward_scale = float(reward_scale); self.task_reward_lerp = None if task_reward_lerp is None else float(task_reward_lerp)

    @classmethod
    def from_checkpoint(cls, prefix: str, **kw):
        from . import tf_checkpoint
        return cls(tf_checkpoint.disc_weights(prefix), **kw)

    def _head(self, row_mask=0, fill=0.0, task_reward_ptr=0):
        if task_reward_ptr and self.task_reward_lerp is None:
            raise ValueError("a task reward needs task_reward_lerp (the agent's TaskRewardLerp)")
        return _ScalarHead(STYLE, 0.0, 0.0, 0.0, 0.0, None, self.reward_scale, self.task_reward_lerp or 0.0, task_reward_ptr or None, row_mask or None, float(fill))


def reference_value(y, lo=-np.inf, hi=np.inf, terminate=None, val_fail=0.0, val_succ=0.0, row_mask=None, fill=0.0):
    """numpy statement of the value head on the net's output y (float64): min(max(y, lo), hi) with a NaN y -> lo, then the terminate override, then the mask"""
    y = np.asarray(y, dtype=np.float64)
    v = np.fmin(np.fmax(y, lo), hi)
    if terminate is not None:
        t = np.asarray(terminate)
        v = np.where(t == TERM_FAIL, val_fail, np.where(t == TERM_SUCC, val_succ, v))
    return v if row_mask is None else np.where(np.asarray(row_mask) != 0, v, fill)


def reference_style_reward(y, scale=1.0, lerp=None, task_reward=None, row_mask=None, fill=0.0):
    """numpy statement of the style head on the logit y (float64): scale * max(0, 1 - 0.25 (1 - y)^2), blended with a task reward; a NaN y -> 0"""
    y = np.asarray(y, dtype=np.float64)
    d = 1.0 - y
    r = np.fmax(1.0 - 0.25 * d * d, 0.0) * scale
    if task_reward is not None:
        r = (1.0 - lerp) * r + lerp * np.asarray(task_reward, dtype=np.float64)
    return r if row_mask is None else np.where(np.asarray(row_mask) != 0, r, fill)


def reference_forward(weights: dict, states, s_clip=np.inf, bf16=False):
    """the net's output y [n] in numpy: `policy.reference_forward` of the same arrays with the one output column and no action normaliser"""
    from .policy import reference_forward as actor_reference
    w = {k: v for k, v in weights.items() if k not in ("a_mean", "a_std", "logstd")}
    w["w3"] = np.asarray(w["w3"], dtype=np.float32).reshape(np.asarray(w["w2"]).shape[1], 1); w["b3"] = np.asarray(w["b3"], dtype=np.float32).reshape(1)
    return actor_reference(w, states, s_clip=s_clip, bf16=bf16)[1][:, 0]
