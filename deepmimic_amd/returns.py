"""TD(lambda) returns over a device-resident rollout (libdm_hip.so `dm_td_lambda_returns`, deepmimic_amd/csrc/dm_returns.h): the critic targets of the
reference's learner -- RLUtil.compute_return (learning/rl_util.py:3-18) per path under the end-of-path rules of learning/ppo_agent.py:251-284 -- for T
control steps of N envs whose records never left HBM.  Everything is time-major, row t = step t of the N envs, the way a sampler stacks the outputs
of `TorchVecEnv.step`:

    rewards [T, N]        reward of step t
    values [T + 1, N]     critic on the observation the action of step t was taken from; row T: on the observation after the last step
    term_values [T, N]    critic on info["terminal_obs"] / info["terminal_goal"] of step t; used only where done[t] is set
    terminate, done, valid [T, N] int32   info["terminate"], the `done` of step t, info["valid"]

Behind a step that is not done stands values[t + 1]; behind a done step val_fail / val_succ (terminate Fail / Succ) or term_values[t] (Null: episode timer,
clip end).  A window cut at T is bootstrapped from values[T] like a Null end -- the one deviation from the reference, which stores whole paths only.
`mask` is 0 for the steps of an episode that ended invalid inside the window (the reference's driver discards it).  The arithmetic is fp64 in the
reference's association with one rounding to fp32.  The advantage (returns - values[:T]), its normalisation, the value clipping and the minibatches
are `deepmimic_amd.ppo_batch`'s."""
from __future__ import annotations

from typing import Optional

from .binding import check, stream_handle, tensor_arg, vp
from .core import load_library


def td_lambda_returns(T: int, N: int, rewards_ptr: int, values_ptr: int, term_values_ptr: int, terminate_ptr: int, done_ptr: int, valid_ptr: int,
                      gamma: float, td_lambda: float, val_fail: float, val_succ: float, returns_ptr: int, mask_ptr: int = 0,
                      stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints; valid_ptr and mask_ptr may be 0), asynchronous on the HIP stream `stream` (0 = the null stream) of `device_id`."""
    lib = load_library(lib_path)
    check(lib, lib.dm_td_lambda_returns(int(device_id), int(T), int(N), vp(rewards_ptr), vp(values_ptr), vp(term_values_ptr), vp(terminate_ptr), vp(done_ptr), vp(valid_ptr),
                                         float(gamma), float(td_lambda), float(val_fail), float(val_succ), vp(returns_ptr), vp(mask_ptr), vp(stream)))


def td_lambda_returns_torch(rewards, values, term_values, terminate, done, valid, gamma: float, td_lambda: float, val_fail: float, val_succ: float,
                            lib_path: Optional[str] = None):
    """The same on torch tensors of one GPU, on torch's current stream: returns (returns [T, N] float32, mask [T, N] int32).  `done` may be a bool
    tensor (what `TorchVecEnv.step` hands out) or int32; `valid` may be None (every episode valid)."""
    import torch
    if rewards.dim() != 2:
        raise ValueError("rewards must be [T, N]")
    T, N = int(rewards.shape[0]), int(rewards.shape[1])
    dev = rewards.device
    if dev.type != "cuda":
        raise ValueError("td_lambda_returns_torch needs GPU tensors (deepmimic_amd has no CPU path)")
    if done.dtype == torch.bool:
        done = done.to(torch.int32)
    f32, i32 = torch.float32, torch.int32
    tensor_arg("rewards", rewards, dev, f32, [(T, N)]); tensor_arg("values", values, dev, f32, [(T + 1, N)]); tensor_arg("term_values", term_values, dev, f32, [(T, N)])
    tensor_arg("terminate", terminate, dev, i32, [(T, N)]); tensor_arg("done", done, dev, i32, [(T, N)])
    if valid is not None:
        tensor_arg("valid", valid, dev, i32, [(T, N)])
    returns = torch.empty((T, N), dtype=torch.float32, device=dev); mask = torch.empty((T, N), dtype=torch.int32, device=dev)
    td_lambda_returns(T, N, rewards.data_ptr(), values.data_ptr(), term_values.data_ptr(), terminate.data_ptr(), done.data_ptr(),
                      valid.data_ptr() if valid is not None else 0, gamma, td_lambda, val_fail, val_succ, returns.data_ptr(), mask.data_ptr(),
                      stream=stream_handle(dev), device_id=dev.index or 0, lib_path=lib_path)
    return returns, mask


def critic_returns_torch(critic, obs, goals, terminal_obs, terminal_goal, terminate, done, valid, rewards, gamma: float, td_lambda: float,
                         lib_path: Optional[str] = None, return_values: bool = False, bounds=None):
    """TD(lambda) targets of a stacked rollout straight from a `deepmimic_amd.heads.Critic`: obs [T + 1, N, S] (row T: the observation after the last step),
    goals [T + 1, N, G] or None, terminal_obs [T, N, S] / terminal_goal [T, N, G] (info["terminal_obs"] / info["terminal_goal"] of every step), the flags and
    rewards [T, N].  Two critic launches -- values on obs, and term_values on terminal_obs under row_mask = done, so tiles without a finished episode cost
    nothing -- then dm_td_lambda_returns with the critic's val_fail / val_succ.  The Fail / Succ override is td_lambda_returns' own rule, so the values stay
    the net's (clipped) output.  Returns (returns [T, N] float32, mask [T, N] int32), and the values [T + 1, N] behind them as a third item if
    `return_values` (what `ppo_batch.advantages_torch` takes); all on torch's current stream.
    bounds: an `amp_rewards.AmpRewards` -- the AMP agents' value clip (learning/amp_agent.py:441-443): both evaluations are clipped in place to the tracker's
    device-resident bounds over 1 - discount (term_values under row_mask = done) before dm_td_lambda_returns, bit for bit what a `Critic(lo, hi)` rebuilt from a host
    copy of the bounds gives, without the host read.  None: nothing changes."""
    import torch
    T = int(rewards.shape[0])
    if int(obs.shape[0]) != T + 1:
        raise ValueError("obs must be [T + 1, N, S] for rewards [T, N]")
    done_i = done.to(torch.int32) if done.dtype == torch.bool else done
    values = critic.eval_torch(obs, goals)
    term_values = critic.eval_torch(terminal_obs, terminal_goal, row_mask=done_i, fill=0.0)
    if bounds is not None:
        bounds.clip_torch(values, out=values)
        bounds.clip_torch(term_values, row_mask=done_i, fill=0.0, out=term_values)
    ret, mask = td_lambda_returns_torch(rewards, values, term_values, terminate, done_i, valid, gamma, td_lambda, critic.val_fail, critic.val_succ, lib_path=lib_path)
    return (ret, mask, values) if return_values else (ret, mask)
