// A probe for the helpers of dm_math.h: one launch evaluates ONE helper on n independent rows, so that a test can put the inputs at which a helper branches
// (a quadrant boundary of dm_sincos, w < 0, |e| > pi, dot < 0, an angle on +-pi ...) straight into it instead of hoping that a walking character produces them.
// Included at the end of dm_host.cpp (shares its runtime shim and its compile flags); needs no env context.  tests/test_math_device.py is the caller.
//
// Layout: row i reads in[i * DM_MATH_PROBE_IN ..] and writes out[i * DM_MATH_PROBE_OUT ..], doubles both.  The kernel narrows the inputs an op reads to Real
// (float unless f64), calls the dmk:: template itself -- nothing of its arithmetic is restated here -- and widens the result, which is exact.  Outputs an op does
// not produce are written as 0; rows >= n are not touched.  Which inputs an op reads: the DM_MOP_* list of include/dm_hip.h.
//
// WHAT THIS PINS: the helpers' source text, compiled with the flags of dm_host.o.  The copies inlined into the step / reset / query objects are built from the same
// text under other -mllvm flags inside much larger functions and may contract a*b+c differently; end-to-end parity (tests/parity_common.py) remains their check.
//
// One lane per row, 64-lane workgroups; a row is 18 + 12 doubles of traffic and the lanes of a wave diverge only where the helper itself branches.
#pragma once

namespace dmp {

template <typename Real> DM_HD V3<Real> nv3(const double* p) { return mk3((Real)p[0], (Real)p[1], (Real)p[2]); }
template <typename Real> DM_HD Q4<Real> nq4(const double* p) { return mkq((Real)p[0], (Real)p[1], (Real)p[2], (Real)p[3]); }
template <typename Real> DM_HD M3<Real> nm3(const double* p) { M3<Real> r; for (int i = 0; i < 9; ++i) r.m[i] = (Real)p[i]; return r; }
template <typename Real> DM_HD void wv3(double* o, const V3<Real>& v) { o[0] = (double)v.x; o[1] = (double)v.y; o[2] = (double)v.z; }
template <typename Real> DM_HD void wq4(double* o, const Q4<Real>& q) { o[0] = (double)q.w; o[1] = (double)q.x; o[2] = (double)q.y; o[3] = (double)q.z; }
template <typename Real> DM_HD void wm3(double* o, const M3<Real>& a) { for (int i = 0; i < 9; ++i) o[i] = (double)a.m[i]; }

template <typename Real>
__global__ void __launch_bounds__(64) k_math_probe(int op, int n, const double* in, double* out) {
    const int row = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (row >= n) return;
    const double* x = in + (size_t)row * DM_MATH_PROBE_IN;
    double o[DM_MATH_PROBE_OUT];
    for (int i = 0; i < DM_MATH_PROBE_OUT; ++i) o[i] = 0.0;
    switch (op) {
    case DM_MOP_SINCOS: { Real s, c; dm_sincos((Real)x[0], s, c); o[0] = (double)s; o[1] = (double)c; break; }
    case DM_MOP_ROT_Y: wm3(o, rot_y((Real)x[0])); break;
    case DM_MOP_ROT_Z: wm3(o, rot_z((Real)x[0])); break;
    case DM_MOP_NORMALIZE_ANGLE: o[0] = (double)normalize_angle((Real)x[0]); break;
    case DM_MOP_QMUL: wq4(o, qmul(nq4<Real>(x), nq4<Real>(x + 4))); break;
    case DM_MOP_QNORMALIZE: wq4(o, qnormalize(nq4<Real>(x))); break;
    case DM_MOP_QSTANDARDIZE: wq4(o, qstandardize(nq4<Real>(x))); break;
    case DM_MOP_QROT: wv3(o, qrot(nq4<Real>(x), nv3<Real>(x + 4))); break;
    case DM_MOP_QUAT_TO_ROT: wm3(o, quat_to_rot(nq4<Real>(x))); break;
    case DM_MOP_QUAT_TO_ROTVEC: wv3(o, quat_to_rotvec(nq4<Real>(x), (Real)x[4])); break;
    case DM_MOP_QUAT_THETA: o[0] = (double)quat_theta(nq4<Real>(x)); break;
    case DM_MOP_QUAT_EXP: wq4(o, quat_exp(nv3<Real>(x))); break;
    case DM_MOP_EXP_MAP_TO_QUAT: wq4(o, exp_map_to_quat(nv3<Real>(x))); break;
    case DM_MOP_QUAT_DIFF_MUL: wq4(o, quat_diff_mul(nq4<Real>(x), nv3<Real>(x + 4))); break;
    case DM_MOP_QSLERP: wq4(o, qslerp(nq4<Real>(x), (Real)x[8], nq4<Real>(x + 4), (Real)x[9])); break;
    case DM_MOP_CALC_HEADING: o[0] = (double)calc_heading(nq4<Real>(x)); break;
    case DM_MOP_CROSS: wv3(o, cross(nv3<Real>(x), nv3<Real>(x + 3))); break;
    case DM_MOP_CROSS_ADD: wv3(o, cross_add(nv3<Real>(x), nv3<Real>(x + 3), nv3<Real>(x + 6))); break;
    case DM_MOP_M3_V3: wv3(o, nm3<Real>(x) * nv3<Real>(x + 9)); break;
    case DM_MOP_TMUL: wv3(o, tmul(nm3<Real>(x), nv3<Real>(x + 9))); break;
    case DM_MOP_M3_M3: wm3(o, nm3<Real>(x) * nm3<Real>(x + 9)); break;
    default: break;                     // (the entry point refuses an unknown op before the launch)
    }
    double* y = out + (size_t)row * DM_MATH_PROBE_OUT;
    for (int i = 0; i < DM_MATH_PROBE_OUT; ++i) y[i] = o[i];
}

}  // namespace dmp

extern "C" {

int dm_math_probe(int device_id, int op, int f64, int n, const double* in_dev, double* out_dev, void* hip_stream) {
    if (n < 1) return fail("dm_math_probe: n must be >= 1");
    if (!in_dev || !out_dev) return fail("dm_math_probe: null argument");
    if (op < 0 || op >= DM_MOP_COUNT) return fail("dm_math_probe: unknown op");
    if ((long long)n * DM_MATH_PROBE_IN > 0x7fffffffLL) return fail("dm_math_probe: too many rows for one call");
    if (valid_device("dm_math_probe", device_id)) return -1;
    DevGuard guard(device_id);
    if (f64) RT_LAUNCH(dmp::k_math_probe<double>, (n + 63) / 64, (rt_stream)hip_stream, op, n, in_dev, out_dev);
    else RT_LAUNCH(dmp::k_math_probe<float>, (n + 63) / 64, (rt_stream)hip_stream, op, n, in_dev, out_dev);
    return launch_status(0);
}

}  // extern "C"
