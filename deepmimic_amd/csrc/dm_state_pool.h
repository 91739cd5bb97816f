// A pool of whole env records in device memory: the entry points of k_state_save and k_state_restore (dm_device.h, the object of the reset / query / probe family).
// Included at the end of dm_host.cpp (shares its runtime shim).  The contract is in include/dm_hip.h (dm_state_pool_*, dm_state_save, dm_state_restore), the slot
// layout in dm_types.h (StatePoolLayout), the Python layer in deepmimic_amd/state_pool.py.  The pool is the caller's memory, as with dm_replay_*; save and restore
// are asynchronous on the context's stream and read nothing back; every refusal stands before the launch.
#pragma once

namespace {
int state_pool_args(const char* fn, const CtxBase* c, const void* pool, int slots, const void* mask, const void* slots_dev) {
    const std::string f(fn);
    if (!pool) return fail(f + ": null pool_dev");
    if (!mask) return fail(f + ": null mask_dev");
    if (!slots_dev) return fail(f + ": null slots_dev");
    if (slots <= 0) return fail(f + ": slots must be positive");
    if ((((uintptr_t)pool) & 15) != 0) return fail(f + ": the pool must be 16-byte aligned");
    if (c->has_tape()) return fail(f + ": a draw tape is bound (dm_set_draw_tape): the tape's positions live on the host and are not part of a record");
    return 0;
}
}  // namespace

extern "C" {

int64_t dm_state_pool_bytes(const dm_ctx* ctx, int slots) {
    if (!ctx) { fail("dm_state_pool_bytes: null ctx"); return -1; }
    if (slots <= 0) { fail("dm_state_pool_bytes: slots must be positive"); return -1; }
    return (int64_t)slots * ctx->c->state_pool_layout().bytes;
}

int dm_state_pool_dims(const dm_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return fail("dm_state_pool_dims: null argument");
    const dmk::StatePoolLayout lay = ctx->c->state_pool_layout();
    out[0] = lay.bytes;
    for (int k = 0; k < dmk::SP_NSEG; ++k) out[1 + k] = lay.off[k];
    return 0;
}

int dm_state_save(dm_ctx* ctx, void* pool_dev, int slots, const int32_t* mask_dev, const int32_t* slots_dev, int32_t* bad_dev) {
    if (!ctx) return fail("dm_state_save: null ctx");
    CtxBase* c = ctx->c;
    if (state_pool_args("dm_state_save", c, pool_dev, slots, mask_dev, slots_dev)) return -1;
    DevGuard guard(c->device_id);
    return launch_status(c->state_save(pool_dev, slots, mask_dev, slots_dev, bad_dev));
}

int dm_state_restore(dm_ctx* ctx, const void* pool_dev, int slots, const int32_t* mask_dev, const int32_t* slots_dev, int flags, float* states_dev, float* goals_dev,
                     int32_t* bad_dev) {
    if (!ctx) return fail("dm_state_restore: null ctx");
    CtxBase* c = ctx->c;
    if (state_pool_args("dm_state_restore", c, pool_dev, slots, mask_dev, slots_dev)) return -1;
    if (flags & ~dmk::SP_ALL_FLAGS) return fail("dm_state_restore: unknown flag bits");
    if (goals_dev && !c->goal_size) return fail("dm_state_restore: goals_dev on a scene without a goal");
    DevGuard guard(c->device_id);
    return launch_status(c->state_restore(pool_dev, slots, mask_dev, slots_dev, flags, states_dev, goals_dev, bad_dev));
}

}  // extern "C"
