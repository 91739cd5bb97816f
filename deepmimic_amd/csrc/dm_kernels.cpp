// One kernel family of libdm_hip.so (dm_families.h) per object file.  Compiled as
//     hipcc ... -DDM_TU_F64=<0|1> -DDM_TU_ID=<family> -c dm_kernels.cpp -o k_<prec>_<family>.o
// (deepmimic_amd/csrc/Makefile; tests/emu/Makefile the same with g++ -DDM_EMU).
// The kernels themselves live in dm_device.h / dm_device_duo.h; this file only holds their launchers (dm_launch.h).
// Loop variants and tuning constants are properties of the kernel classes and constants in the headers (dm_types.h: PIPE, ClsBipedFb<YFULL>; DuoSim::YFULL; kPrio*, kXdRows, ...):
// a -D that changed the body of shared inline code would give one template instantiation different bodies in different objects.  The retired knobs fail the build.
#if defined(DM_YPREF) || defined(DM_LCPREF) || defined(DM_ELPREF) || defined(DM_TFPREF) || defined(DM_STPREF) || defined(DM_PAIRPREF) || defined(DM_DRPREF) || \
    defined(DM_YPREF_DENSE_FENCE) || defined(DM_DUO_YFULL) || defined(DM_DUO_YPMAX) || defined(DM_DUO_XD) || defined(DM_DUO_WIDE_FALLBACK) || defined(DM_XD_ROWS) || \
    defined(DM_XD_YSOPQ) || defined(DM_XD_YSUNI) || defined(DM_XD_YSLANE) || defined(DM_XCD_MAP) || defined(DM_FB_RREG) || defined(DM_FB_PRIO) || defined(DM_DOG_RREG) || \
    defined(DM_LT_WAVES) || defined(DM_BT_WAVES) || defined(DM_OBJ_WAVES) || defined(DM_PRIO) || defined(DM_PRIO_CHOL) || defined(DM_PRIO_Y) || defined(DM_PRIO_BACK) || \
    defined(DM_PRIO_KIN) || defined(DM_PRIO_ONE_CHOL) || defined(DM_PRIO_ONE_Y) || defined(DM_PRIO_ONE_BACK) || defined(DM_PRIO_ONE_KIN) || defined(DM_PRIO_BASE) || \
    defined(DM_PRIO_MID) || defined(DM_PRIO_LO) || defined(DM_PRIO_HI) || defined(DM_PRIO_LATE)
#error "retired -D knob: edit the constant or the class property in dm_types.h / dm_device.h / dm_device_duo.h instead (one body per template instantiation)"
#endif
#include "dm_launch.h"
#include "dm_device_duo.h"
#if DM_TU_ID == DM_MISC_FAMILY
#include "dm_wave_probe.h"    // test support: one wave-level primitive of the two headers above per launch (this object only)
#endif

namespace dmk {

template <typename Real, int ID>
void launch_step_family(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StepIO<Real>& io, const DebugTaps<Real>& dbg) {
    typedef typename StepFamily<ID>::C C;
    constexpr int V = StepFamily<ID>::VARIANT;
    // (if constexpr: a plain if would put both kernels into every object)
    if constexpr (StepFamily<ID>::PACK == 2) RT_LAUNCH((k_env_step_duo<Real, V == SV_TAPS, V == SV_AMP || V == SV_V2, V == SV_V2, C>), grid, s, m, st, io, dbg);
    else RT_LAUNCH((k_env_step<Real, C, V == SV_TAPS, V == SV_AMP || V == SV_V2, V == SV_V2>), grid, s, m, st, io, dbg);
}
template <typename Real, typename C>
void launch_reset(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* env_ids, const double* kin_times, const double* max_times) {
    RT_LAUNCH((k_env_reset<Real, C>), grid, s, m, st, env_ids, kin_times, max_times);
}
template <typename Real, typename C>
void launch_query(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StepIO<Real>& io, const DebugTaps<Real>& dbg) {
    RT_LAUNCH((k_env_query<Real, C>), grid, s, m, st, io, dbg);
}
template <typename Real, typename C>
void launch_probe(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const DebugTaps<Real>& dbg, int what, double dt) {
    RT_LAUNCH((k_env_probe<Real, C>), grid, s, m, st, dbg, what, dt);
}
template <typename Real, typename C>
void launch_amp_expert(unsigned grid, rt_stream s, const ModelDev<Real>& m, const double* times, const double* ground_h, float* out, const int* clips) {
    RT_LAUNCH((k_amp_expert<Real, C>), grid, s, m, times, ground_h, out, clips);
}
template <typename Real, typename C>
void launch_time_warp_sample(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, Real* samples, int* count, const int* restart, int capacity, int* overflow) {
    RT_LAUNCH((k_time_warp_sample<Real, C>), grid, s, m, st, samples, count, restart, capacity, overflow);
}
template <typename Real, typename C>
void launch_link_state(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, int which, float* links, float* env_out, float* pose_out, float* vel_out, float* obj_out) {
    RT_LAUNCH((k_link_state<Real, C>), grid, s, m, st, which, links, env_out, pose_out, vel_out, obj_out);
}
template <typename Real, typename C>
void launch_reset_where(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, float* states, float* goals_own, float* goals) {
    RT_LAUNCH((k_env_reset_where<Real, C>), grid, s, m, st, mask, states, goals_own, goals);
}
template <typename Real, typename C>
void launch_kin_query(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, int K, const double* times, const int* clips, int flags, float* links, float* env_out, float* pose_out, float* vel_out) {
    RT_LAUNCH((k_kin_query<Real, C>), grid, s, m, st, K, times, clips, flags, links, env_out, pose_out, vel_out);
}
template <typename Real, typename C>
void launch_reset_where_at(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, const int* clips, const double* times, const double* yaws, float* states, float* goals_own, float* goals, int* bad) {
    RT_LAUNCH((k_env_reset_where_at<Real, C>), grid, s, m, st, mask, clips, times, yaws, states, goals_own, goals, bad);
}
template <typename Real, typename C>
void launch_state_save(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StatePoolLayout& lay, unsigned char* pool, int M, const int* mask, const int* slots, int* bad) {
    RT_LAUNCH((k_state_save<Real, C>), grid, s, m, st, lay, pool, M, mask, slots, bad);
}
template <typename Real, typename C>
void launch_state_restore(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StatePoolLayout& lay, const unsigned char* pool, int M, const int* mask, const int* slots, int flags, float* states, float* goals_own, float* goals, int* bad) {
    RT_LAUNCH((k_state_restore<Real, C>), grid, s, m, st, lay, pool, M, mask, slots, flags, states, goals_own, goals, bad);
}
template <typename Real>
void launch_push_where(rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, const int* links, const double* forces, const double* durs, const int* slots, int flags, int* bad) {
    RT_LAUNCH((k_push_where<Real>), (st.N + kWave - 1) / kWave, s, st.N, m.J, m.P, (const Real*)st.pose, st.pert, mask, links, forces, durs, slots, flags, bad);
}
template <typename Real>
void launch_push_state(rt_stream s, const EnvState<Real>& st, float* out) {
    RT_LAUNCH((k_push_state<Real>), (st.N + kWave - 1) / kWave, s, st.N, (const double*)st.pert, out);
}

// this object's family (dm_families.h): the reset / query / probe family expands its class lists, any other id instantiates the launcher of its row
#if DM_TU_F64
typedef double TuReal;
#else
typedef float TuReal;
#endif
#define DM_STEP_ARGS unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const StepIO<TuReal>&, const DebugTaps<TuReal>&
#if DM_TU_ID == DM_MISC_FAMILY
#define DM_INST_MISC(C)                                                                                                                                  \
    template void launch_reset<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const int*, const double*, const double*); \
    template void launch_query<TuReal, C>(DM_STEP_ARGS);                                                                                                 \
    template void launch_probe<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const DebugTaps<TuReal>&, int, double); \
    template void launch_link_state<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, int, float*, float*, float*, float*, float*); \
    template void launch_reset_where<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const int*, float*, float*, float*); \
    template void launch_kin_query<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, int, const double*, const int*, int, float*, float*, float*, float*); \
    template void launch_reset_where_at<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const int*, const int*, const double*, const double*, float*, float*, float*, int*); \
    template void launch_state_save<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const StatePoolLayout&, unsigned char*, int, const int*, const int*, int*); \
    template void launch_state_restore<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const StatePoolLayout&, const unsigned char*, int, const int*, const int*, int, float*, float*, float*, int*);
#define DM_INST_EXPERT(C)                                                                                                                                \
    template void launch_amp_expert<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const double*, const double*, float*, const int*);            \
    template void launch_time_warp_sample<TuReal, C>(unsigned, rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, TuReal*, int*, const int*, int, int*);
DM_MISC_CLASSES(DM_INST_MISC)
DM_EXPERT_CLASSES(DM_INST_EXPERT)
template void launch_wave_probe<TuReal>(unsigned, rt_stream, int, int, const double*, double*);
template void launch_push_where<TuReal>(rt_stream, const ModelDev<TuReal>&, const EnvState<TuReal>&, const int*, const int*, const double*, const double*, const int*, int, int*);
template void launch_push_state<TuReal>(rt_stream, const EnvState<TuReal>&, float*);
#else
template void launch_step_family<TuReal, DM_TU_ID>(DM_STEP_ARGS);
#endif

}  // namespace dmk
