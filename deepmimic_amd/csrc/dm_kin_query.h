// The kinematic character at caller-given times and a masked reset whose clip, clip time and yaw the caller may give: the entry points of k_kin_query and
// k_env_reset_where_at (dm_device.h, the object of the reset / query / probe family).  Included at the end of dm_host.cpp (shares its runtime shim).  The contract is
// in include/dm_hip.h (dm_kin_query, dm_reset_where_at), the Python layer in deepmimic_amd/kin_query.py.  Both calls are asynchronous on the context's stream and read
// nothing back; every refusal stands before the launch.
#pragma once

extern "C" {

int dm_kin_query(dm_ctx* ctx, int K, const double* times_dev, const int32_t* clips_dev, int flags, float* links_dev, float* env_dev, float* pose_dev, float* vel_dev) {
    if (!ctx) return fail("dm_kin_query: null ctx");
    CtxBase* c = ctx->c;
    if (!times_dev) return fail("dm_kin_query: null times_dev");
    if (K < 1 || K > dmk::KQ_MAX_K) return fail("dm_kin_query: K must be in [1, 64]");
    if (c->hm.F < 1 || c->hm.frames.empty()) return fail("dm_kin_query: the scene has no kinematic character (no motion frames)");
    if (flags & ~dmk::KQ_ALL_FLAGS) return fail("dm_kin_query: unknown flag bits");
    if (clips_dev && !(flags & dmk::KQ_TIMES_ABSOLUTE)) return fail("dm_kin_query: clips_dev needs DM_KIN_TIMES_ABSOLUTE (an offset from the env's clock belongs to the env's own clip)");
    DevGuard guard(c->device_id);
    return launch_status(c->kin_query(K, times_dev, clips_dev, flags, links_dev, env_dev, pose_dev, vel_dev));
}

int dm_reset_where_at(dm_ctx* ctx, const int32_t* mask_dev, const int32_t* clips_dev, const double* times_dev, const double* yaw_dev, float* states_dev, float* goals_dev,
                      int32_t* bad_dev) {
    if (!ctx) return fail("dm_reset_where_at: null ctx");
    CtxBase* c = ctx->c;
    if (!mask_dev) return fail("dm_reset_where_at: null mask_dev");
    if (!states_dev) return fail("dm_reset_where_at: null states_dev");
    if (goals_dev && !c->goal_size) return fail("dm_reset_where_at: goals_dev on a scene without a goal");
    if (c->has_tape()) return fail("dm_reset_where_at: a draw tape is bound (dm_set_draw_tape): the tape route draws on the host, resets go through dm_reset");
    DevGuard guard(c->device_id);
    return launch_status(c->reset_where_at(mask_dev, clips_dev, times_dev, yaw_dev, states_dev, goals_dev, bad_dev));
}

}  // extern "C"
