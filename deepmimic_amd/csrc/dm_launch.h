// Launchers of the env kernels.  libdm_hip.so is built from several translation units: dm_host.cpp (tables, C-ABI, policy
// kernels) only sees these declarations; dm_kernels.cpp is compiled once per (precision, kernel family of dm_families.h) and
// instantiates exactly one family per object file (Makefile: k_<prec>_<id>.o), so the 30+ step-kernel instantiations compile in parallel.
#pragma once
#ifdef DM_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include "dm_families.h"

#ifdef DM_EMU
typedef void* rt_stream;
#define RT_LAUNCH(kern, grid, stream, ...) emu::launch((unsigned)(grid), 64, [&]() { kern(__VA_ARGS__); })
#define RT_LAUNCH4(kern, grid, stream, ...) emu::launch((unsigned)(grid), 256, [&]() { kern(__VA_ARGS__); })
#else
typedef hipStream_t rt_stream;
#define RT_LAUNCH(kern, grid, stream, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(64), 0, stream, __VA_ARGS__)
#define RT_LAUNCH4(kern, grid, stream, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(256), 0, stream, __VA_ARGS__)   // four wavefronts per workgroup
#endif

namespace dmk {

// the step kernel of family ID (its row of dm_families.h): k_env_step_duo for a two-per-wavefront row, k_env_step otherwise
template <typename Real, int ID>
void launch_step_family(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StepIO<Real>& io, const DebugTaps<Real>& dbg);
template <typename Real, typename C>
void launch_reset(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* env_ids, const double* kin_times, const double* max_times);
template <typename Real, typename C>
void launch_query(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StepIO<Real>& io, const DebugTaps<Real>& dbg);
template <typename Real, typename C>
void launch_probe(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const DebugTaps<Real>& dbg, int what, double dt);
template <typename Real, typename C>
void launch_amp_expert(unsigned grid, rt_stream s, const ModelDev<Real>& m, const double* times, const double* ground_h, float* out, const int* clips);
template <typename Real, typename C>
void launch_time_warp_sample(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, Real* samples, int* count, const int* restart, int capacity, int* overflow);
template <typename Real, typename C>
void launch_link_state(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, int which, float* links, float* env_out, float* pose_out, float* vel_out, float* obj_out);
template <typename Real, typename C>
void launch_reset_where(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, float* states, float* goals_own, float* goals);
template <typename Real, typename C>
void launch_kin_query(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, int K, const double* times, const int* clips, int flags, float* links, float* env_out, float* pose_out, float* vel_out);
template <typename Real, typename C>
void launch_reset_where_at(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, const int* clips, const double* times, const double* yaws, float* states, float* goals_own, float* goals, int* bad);
template <typename Real, typename C>
void launch_state_save(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StatePoolLayout& lay, unsigned char* pool, int M, const int* mask, const int* slots, int* bad);
template <typename Real, typename C>
void launch_state_restore(unsigned grid, rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const StatePoolLayout& lay, const unsigned char* pool, int M, const int* mask, const int* slots, int flags, float* states, float* goals_own, float* goals, int* bad);
// task-chosen pushes (k_push_where / k_push_state, in the object of DM_MISC_FAMILY): one lane per env, one instantiation per precision
template <typename Real>
void launch_push_where(rt_stream s, const ModelDev<Real>& m, const EnvState<Real>& st, const int* mask, const int* links, const double* forces, const double* durs, const int* slots, int flags, int* bad);
template <typename Real>
void launch_push_state(rt_stream s, const EnvState<Real>& st, float* out);
// test support (dm_wave_probe.h, in the object of DM_MISC_FAMILY): one wave-level primitive of dm_device.h / dm_device_duo.h per launch, `grid` wavefronts
template <typename Real>
void launch_wave_probe(unsigned grid, rt_stream s, int op, int arg, const double* in, double* out);

}  // namespace dmk
