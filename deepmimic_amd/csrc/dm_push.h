// Task-chosen pushes from device tensors and the forces that are acting: the entry points of k_push_where and k_push_state (dm_device.h, the object of the
// reset / query / probe family).  Included at the end of dm_host.cpp (shares its runtime shim).  The contract is in include/dm_hip.h (dm_push_where, dm_push_state),
// the columns in dm_types.h (PS_*), the Python layer in deepmimic_amd/pushes.py.  Both calls are asynchronous on the context's stream and read nothing back; every
// refusal stands before the launch.
#pragma once

extern "C" {

int dm_push_where(dm_ctx* ctx, const int32_t* mask_dev, const int32_t* links_dev, const double* forces_dev, const double* durations_dev, const int32_t* slots_dev,
                  int flags, int32_t* bad_dev) {
    if (!ctx) return fail("dm_push_where: null ctx");
    CtxBase* c = ctx->c;
    if (!mask_dev) return fail("dm_push_where: null mask_dev");
    if (!links_dev) return fail("dm_push_where: null links_dev");
    if (!forces_dev) return fail("dm_push_where: null forces_dev");
    if (!durations_dev) return fail("dm_push_where: null durations_dev");
    if (flags & ~dmk::PS_ALL_FLAGS) return fail("dm_push_where: unknown flag bits");
    if (!c->has_pert()) return fail("dm_push_where: the context has no perturbation rows (enable_rand_perturbs is off)");
    DevGuard guard(c->device_id);
    return launch_status(c->push_where(mask_dev, links_dev, forces_dev, durations_dev, slots_dev, flags, bad_dev));
}

int dm_push_state(dm_ctx* ctx, float* out_dev) {
    if (!ctx) return fail("dm_push_state: null ctx");
    CtxBase* c = ctx->c;
    if (!out_dev) return fail("dm_push_state: null out_dev");
    if (!c->has_pert()) return fail("dm_push_state: the context has no perturbation rows (enable_rand_perturbs is off)");
    DevGuard guard(c->device_id);
    return launch_status(c->push_state(out_dev));
}

}  // extern "C"
