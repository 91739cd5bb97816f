// Link states as device tensors and the reset selected by a device mask: the entry points of k_link_state and k_env_reset_where (dm_device.h, the object of the
// reset / query / probe family).  Included at the end of dm_host.cpp (shares its runtime shim).  The contract is in include/dm_hip.h (dm_link_state*, dm_reset_where),
// the Python layer in deepmimic_amd/link_state.py.  Both calls are asynchronous on the context's stream and read nothing back; every refusal stands before the launch.
#pragma once

extern "C" {

int dm_link_state_dims(const dm_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return fail("dm_link_state_dims: null argument");
    const CtxBase* c = ctx->c;
    out[0] = c->hm.J; out[1] = dmk::LS_LINK_W; out[2] = dmk::LS_ENV_W; out[3] = c->hm.P; out[4] = c->has_obj() ? dmk::LS_OBJ_W : 0;
    return 0;
}

int dm_link_state(dm_ctx* ctx, int which, float* links_dev, float* env_dev, float* pose_dev, float* vel_dev, float* obj_dev) {
    if (!ctx) return fail("dm_link_state: null ctx");
    CtxBase* c = ctx->c;
    if (which != 0 && which != 1) return fail("dm_link_state: which must be 0 (the simulated character) or 1 (the kinematic character)");
    if (which == 1 && (c->hm.F < 1 || c->hm.frames.empty())) return fail("dm_link_state: the scene has no kinematic character (no motion frames)");
    if (obj_dev && !c->has_obj()) return fail("dm_link_state: obj_dev on a context without a free body (not a dribble_amp scene)");
    DevGuard guard(c->device_id);
    return launch_status(c->link_state(which, links_dev, env_dev, pose_dev, vel_dev, obj_dev));
}

int dm_reset_where(dm_ctx* ctx, const int32_t* mask_dev, float* states_dev, float* goals_dev) {
    if (!ctx) return fail("dm_reset_where: null ctx");
    CtxBase* c = ctx->c;
    if (!mask_dev) return fail("dm_reset_where: null mask_dev");
    if (!states_dev) return fail("dm_reset_where: null states_dev");
    if (goals_dev && !c->goal_size) return fail("dm_reset_where: goals_dev on a scene without a goal");
    if (c->has_tape()) return fail("dm_reset_where: a draw tape is bound (dm_set_draw_tape): the tape route draws on the host, resets go through dm_reset");
    DevGuard guard(c->device_id);
    return launch_status(c->reset_where(mask_dev, states_dev, goals_dev));
}

}  // extern "C"
