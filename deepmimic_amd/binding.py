"""The one ctypes layer between the learner-side modules and libdm_hip.so (include/dm_hip.h): the signatures of the entry points they call, which
`core.load_library` declares once when it opens the library, and the few conversions every call makes -- a device address, a 64 / 32-bit key, the error check -- plus the two
checks of the torch front ends (a tensor argument, a stream handle).  A new entry point adds one row to SIGNATURES and calls through these.

The environment calls of core.py (dm_step_batch and the like) are not in the table: they pass every argument as a ctypes object."""
import ctypes as C

_i, _p, _d, _i64, _u64, _u32, _sz = C.c_int, C.c_void_p, C.c_double, C.c_int64, C.c_uint64, C.c_uint32, C.c_size_t
_pi32 = C.POINTER(C.c_int32)

# name -> (argtypes, restype or None for int); the parameter lists of include/dm_hip.h, every pointer a void* (tests/test_abi.py counts them against the header)
SIGNATURES = {
    "dm_last_error": ([], C.c_char_p),
    "dm_motion_duration": ([_p], _d),
    "dm_refrand_double": ([_p, _d, _d], _d),
    "dm_refrand_exp": ([_p, _d], _d),
    "dm_refrand_norm": ([_p, _d, _d], _d),
    "dm_amp_expert_draw": ([_p, _i, _u64, _p, _p, _p, _p], None),
    "dm_policy_forward": ([_p, _p, _i, _p, _p, _i, _u64, _u32, _i, _p], None),
    "dm_policy_forward_ex": ([_p, _p, _p, _i, _i, _p, _p, _p, _d, _i, _u64, _u32, _i, _p], None),
    "dm_policy_info": ([_p, _pi32], None),
    "dm_policy_set_weights": ([_p, _p, _p, _i, _p], None),
    "dm_policy_read_packed": ([_p, _i, _p, _sz, C.POINTER(_sz)], None),
    "dm_policy_eval_scalar": ([_p, _p, _p, _i, _i, _p, _p, _p, _p], None),
    "dm_policy_scalar_info": ([_p, _pi32], None),
    "dm_policy_bind_obs_normalizer": ([_p, _p, _i, _p], None),
    "dm_norm_create": ([_i, _i, _p, _d, _d, _p], None),
    "dm_norm_destroy": ([_p], None),
    "dm_norm_record": ([_p, _p, _i, _i, _p], None),
    "dm_norm_pending": ([_p, _p, _p], None),
    "dm_norm_update": ([_p, _p], None),
    "dm_norm_set": ([_p, _p, _p, _i64, _p], None),
    "dm_norm_get": ([_p, _p, _p, _p, _p, _p], None),
    "dm_norm_set_state": ([_p, _p, _p, _p, _i64, _p], None),
    "dm_norm_normalize": ([_p, _p, _i, _p, _p], None),
    "dm_td_lambda_returns": ([_i, _i, _i] + [_p] * 6 + [_d] * 4 + [_p] * 3, None),
    "dm_ppo_workspace_bytes": ([_i, _i], _i64),
    "dm_ppo_advantages": ([_i, _i, _i] + [_p] * 4 + [_d] * 4 + [_p] * 7 + [_i64, _p], None),
    "dm_ppo_gather": ([_i, _p, _p, _i64, _i, _u64, _u32, _i, _p, _p, _p], None),
    "dm_replay_append": ([_i, _p, _i, _i, _p, _p, _p, _p, _i, _u64, _u32, _p, _p, _p], None),
    "dm_replay_sample": ([_i, _p, _i, _p, _i, _u64, _u32, _p, _p, _p], None),
    "dm_episode_workspace_bytes": ([_i], _i64),
    "dm_episode_stats": ([_i, _i, _i] + [_p] * 10 + [_i, _i, _p, _i64, _p], None),
    "dm_amp_batch_rewards_workspace": ([_i, _i], _i64),
    "dm_amp_batch_rewards": ([_i, _i, _i] + [_p] * 4 + [_d] * 2 + [_p] * 5 + [_i64, _p], None),
    "dm_amp_value_clip": ([_i, _i, _p, _p, _d, _p, _d, _p, _p], None),
    "dm_time_warp_dims": ([_p, _pi32], None),
    "dm_time_warp_sample": ([_p, _p, _p, _p, _i, _p], None),
    "dm_time_warp_align": ([_i, _i, _i, _i, _i, _p, _p, _p, _d, _p, _p, _p], None),
    "dm_link_state_dims": ([_p, _pi32], None),
    "dm_link_state": ([_p, _i, _p, _p, _p, _p, _p], None),
    "dm_reset_where": ([_p, _p, _p, _p], None),
    "dm_kin_query": ([_p, _i, _p, _p, _i, _p, _p, _p, _p], None),
    "dm_reset_where_at": ([_p] * 8, None),
    "dm_state_pool_bytes": ([_p, _i], _i64),
    "dm_state_pool_dims": ([_p, _pi32], None),
    "dm_state_save": ([_p, _p, _i, _p, _p, _p], None),
    "dm_state_restore": ([_p, _p, _i, _p, _p, _i, _p, _p, _p], None),
    "dm_push_where": ([_p, _p, _p, _p, _p, _p, _i, _p], None),
    "dm_push_state": ([_p, _p], None),
    "dm_train_param_count": ([_p], _i64),
    "dm_train_workspace_bytes": ([_p, _i], _i64),
    "dm_train_actor_grad": ([_p] * 4 + [_i] * 2 + [_p] * 8 + [_i64, _p], None),
    "dm_train_value_grad": ([_p] * 4 + [_i] * 2 + [_p] * 5 + [_i64, _p], None),
    "dm_train_sgd_step": ([_p] * 4 + [_i64] + [_d] * 4 + [_p], None),
    "dm_train_read_activations": ([_p, _i, _i, _p, _sz], None),
    "dm_train_disc_workspace_bytes": ([_p, _i, _i], _i64),
    "dm_train_disc_grad": ([_p] * 3 + [_i, _p, _i] + [_p] * 5 + [_i64, _p], None),
    "dm_train_gated_param_count": ([_p], _i64),
    "dm_train_gated_workspace_bytes": ([_p, _i], _i64),
    "dm_train_gated_actor_grad": ([_p] * 4 + [_i] * 2 + [_p] * 8 + [_i64, _p], None),
    "dm_train_gated_value_grad": ([_p] * 4 + [_i] * 2 + [_p] * 5 + [_i64, _p], None),
    "dm_train_gated_sgd_step": ([_p] * 4 + [_i64] + [_d] * 4 + [_p], None),
    "dm_train_gated_read": ([_p, _i, _i, _p, _sz], None),
    "dm_train_opt_workspace_bytes": ([_i64], _i64),
    "dm_train_opt_step": ([_p] * 6 + [_i64, _p, _p, _i64, _p], None),
    "dm_math_probe": ([_i, _i, _i, _i, _p, _p, _p], None),
    "dm_wave_probe": ([_i, _i, _i, _i, _i, _p, _p, _p], None),
}


def declare(lib):
    """SIGNATURES onto the functions `lib` exports (an older build lacks the newest entry points: their callers refuse it by name)"""
    for name, (argtypes, restype) in SIGNATURES.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.argtypes = argtypes
            if restype is not None:
                f.restype = restype


def vp(p):
    """a device (or host) address held as a Python int; 0 / None is NULL"""
    return C.c_void_p(int(p)) if p else None


def u64(x):
    return C.c_uint64(int(x) & (2 ** 64 - 1))


def u32(x):
    return C.c_uint32(int(x) & 0xFFFFFFFF)


def check(lib, rc):
    if rc != 0:
        raise RuntimeError("libdm_hip: %s" % lib.dm_last_error().decode())


def tensor_arg(name, x, dev, dtype, shapes, contiguous=True):
    """x must be a torch tensor on `dev` of `dtype` with one of `shapes` (and contiguous): ValueError otherwise.  Returns x."""
    import torch
    if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype != dtype or tuple(x.shape) not in shapes or (contiguous and not x.is_contiguous()):
        raise ValueError("%s must be a %s%s tensor of shape %s on %s" % (name, "contiguous " if contiguous else "", str(dtype).replace("torch.", ""),
                                                                        " or ".join(str(tuple(s)) for s in shapes), dev))
    return x


def stream_handle(dev, stream=None):
    """the hipStream_t handle (int) of `stream` -- a torch.cuda.Stream or a raw handle -- or of torch's current stream on `dev`"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(dev)
    return int(getattr(stream, "cuda_stream", stream))
