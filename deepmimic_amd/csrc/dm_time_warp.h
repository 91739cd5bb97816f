// The test-mode return of `--scene imitate_amp` for a batch of envs: cSceneImitateAMP::CalcRewardTimeWarp (scenes/SceneImitateAMP.cpp:174-207) = the dynamic-time-
// warping alignment cost of cDynamicTimeWarper::CalcAlignment (util/DynamicTimeWarper.cpp:114-140) under cSceneImitateAMP::TimeWarpCost (:5-25, mean point distance)
// between the samples k_time_warp_sample (dm_device.h) recorded of the simulated and of the kinematic character, plus term_step_cost per sample the episode fell short
// of the buffer.  Included at the end of dm_host.cpp (shares its runtime shim).  The contract is in include/dm_hip.h (dm_time_warp_*), the Python layer in
// deepmimic_amd/time_warp.py, the same recurrence in numpy in deepmimic_amd/model.py time_warp_cost.
//
// k_time_warp_align<Real>   one wavefront per env, n = count[env] samples on both sides, cost(i, j) = d(i, j) + min(cost(i-1, j-1), cost(i-1, j), cost(i, j-1)) over
//   i, j >= 1 from cost(0, 0) = 0 and +inf along the rest of row 0 and column 0.  The rows go in strips of 64: lane l owns row i = r0 + l and sweeps the columns
//   skewed, j = 1 + s - l in step s, so that a step is one anti-diagonal of the strip and all three predecessors are at hand: cost(i, j-1) is the lane's own previous
//   value, cost(i-1, j) the lower neighbour's previous value (one lane shift per step) and cost(i-1, j-1) what that shift brought one step earlier.  Row r0 - 1 reaches
//   lane 0 through the `bound` row in LDS, which lane 63 overwrites behind lane 0's reads (63 columns behind) for the next strip.  The strip's sim rows lie in LDS
//   (row stride dim | 1 elements: lane l reads row l, every bank once), the kin rows in a ring of 128 rows refilled 64 rows at a time, coalesced, every 64 steps:
//   step s touches rows 1 + s - 63 .. 1 + s, the refill at s = 64 k replaces rows below 1 + s - 64.  Every lane runs every step (off-table lanes compute on clamped
//   indices and keep nothing), so the control flow is wave-uniform.  Distances in Real, table values in fp64, no contraction (the fp64 instantiation is held to the
//   reference's rounding); no atomics, no workgroup waits on another: two runs give the same bytes.
//   LDS per workgroup (dynamic): 8 capacity + 192 (dim | 1) sizeof(Real) bytes -- 39 KB for the humanoid's 20 s test episode in fp32 (capacity 602, dim 45).
//   Work: (n - 1)^2 cells of dim / 3 point distances, i.e. n + 62 steps per strip; the kin rows are re-read from L2 once per strip.
#pragma once

namespace dmw {

constexpr int kRows = 64, kRing = 128;           // rows of a strip (one per lane); kin rows held in LDS (two refills of kRows)
constexpr size_t kLdsMax = 160 * 1024;           // LDS of a gfx950 compute unit: one workgroup can have it all (fp64 parity build of a large character)

#ifdef DM_EMU
static std::vector<double> g_lds;                // the workgroup's dynamic LDS (the emulator runs one workgroup at a time)
#define DMW_DEV inline
#define DMW_LDS(name) double* name = dmw::g_lds.data()
static inline double lane_up(double v) { return dmk::wave_shfl(v, (int)threadIdx.x + 63); }          // from lane l - 1 (lane 0: unused)
#else
#define DMW_DEV __device__ __forceinline__
#define DMW_LDS(name) extern __shared__ double name[]
__device__ __forceinline__ double lane_up(double v) { return __shfl_up(v, 1, 64); }
#endif

struct Args {
    int capacity, dim;
    const void* samples; const int* count; const int* select;
    double term_step_cost;
    float* reward; double* cost;
};

// cSceneImitateAMP::TimeWarpCost: the point distances summed in the order p = 0 .. J - 1, then divided by J
template <typename Real> DMW_DEV Real point_cost(const Real* a, const Real* b, int J) {
#pragma clang fp contract(off)
    Real sum = 0;
#pragma unroll 5
    for (int p = 0; p < J; ++p) {                // (five points a trip: their thirty LDS reads are in flight together; one point a trip waits out the LDS latency J times a cell)
        const Real dx = b[3 * p] - a[3 * p], dy = b[3 * p + 1] - a[3 * p + 1], dz = b[3 * p + 2] - a[3 * p + 2];
        sum = sum + dm_sqrt(dx * dx + dy * dy + dz * dz);
    }
    return sum / (Real)J;
}

DMW_DEV double min3(double a, double b, double c) { const double m = c < b ? c : b; return m < a ? m : a; }      // std::min(a, std::min(b, c)); no NaN in the table

template <typename Real>
__global__ void __launch_bounds__(64) k_time_warp_align(Args a) {
#pragma clang fp contract(off)
    DMW_LDS(lds);
    const int e = (int)blockIdx.x, l = (int)threadIdx.x;
    const int cap = a.capacity, dim = a.dim, J = dim / 3, stride = dim | 1;
    const bool sel = !a.select || a.select[e] != 0;
    int n = sel ? a.count[e] : 0;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    if (n < 2) {                                 // (wave-uniform) not selected: 0; no sample: 0, as the drop-in answers; one sample: an empty table, cost 0
        if (l == 0) { a.reward[e] = n > 0 ? (float)((double)(cap - n) * a.term_step_cost) : 0.0f; if (a.cost) a.cost[e] = 0.0; }
        return;
    }
    double* bound = lds;                                             // [cap]: cost(r0 - 1, j), the row below the strip
    Real* srow = reinterpret_cast<Real*>(lds + cap);                 // [kRows][stride]: sim rows r0 .. r0 + 63
    Real* kring = srow + (size_t)kRows * stride;                     // [kRing][stride]: kin row j in slot j % kRing
    const Real* S = (const Real*)a.samples + (size_t)e * 2 * cap * dim;
    const Real* K = S + (size_t)cap * dim;
    for (int j = l; j < n; j += kRows) bound[j] = INFINITY;          // cost(0, j), j >= 1 ([0] is never read: the corner is lane 0's first diagonal)
    for (int r0 = 1; r0 < n; r0 += kRows) {
        const int rows = (n - r0 < kRows) ? n - r0 : kRows;
        __syncthreads();                                             // the previous strip is done with srow and kring, its bound row is written
        for (int t = l; t < rows * dim; t += kRows) { const int r = t / dim; srow[r * stride + (t - r * dim)] = S[(size_t)r0 * dim + t]; }
        const bool row_on = l < rows;
        const Real* mine = srow + (row_on ? l : 0) * stride;
        double cur = INFINITY;                                       // cost(i, j - 1): column 0
        double diag = (l == 0 && r0 == 1) ? 0.0 : INFINITY;          // cost(i - 1, j - 1): the corner for row 1, column 0 otherwise
        const int steps = (n - 1) + (rows - 1);
        for (int s = 0; s < steps; ++s) {
            if ((s & (kRows - 1)) == 0) {                            // kin rows 1 + s .. 1 + s + 63 over the slots of rows no lane reads any more
                __syncthreads();
                const int j0 = 1 + s, cnt = (n - j0 < kRows) ? n - j0 : kRows;
                for (int t = l; t < cnt * dim; t += kRows) { const int r = t / dim; kring[((j0 + r) & (kRing - 1)) * stride + (t - r * dim)] = K[(size_t)j0 * dim + t]; }
                __syncthreads();
            }
            const int j = 1 + s - l;
            const bool on = row_on && j >= 1 && j < n;
            const int jc = j < 1 ? 1 : (j >= n ? n - 1 : j);          // off-table lanes compute on a valid column and keep nothing
            double up = lane_up(cur);                                // cost(i - 1, j): what lane l - 1 made of column j one step ago
            if (l == 0) up = bound[jc];
            const Real d = point_cost(mine, kring + (jc & (kRing - 1)) * stride, J);
            const double v = (double)d + min3(diag, up, cur);
            diag = up;
            if (on) {
                cur = v;
                if (l == kRows - 1) bound[j] = v;
                if (r0 + l == n - 1 && j == n - 1) {                 // cost(n - 1, n - 1): cDynamicTimeWarper::GetMinAlignmentCost
                    a.reward[e] = (float)(v + (double)(cap - n) * a.term_step_cost);
                    if (a.cost) a.cost[e] = v;
                }
            }
        }
    }
}

inline size_t lds_bytes(int capacity, int dim, int f64) { return 8 * (size_t)capacity + (size_t)(kRows + kRing) * (size_t)(dim | 1) * (f64 ? 8 : 4); }

template <typename Real> static int launch_align(int n_envs, size_t bytes, rt_stream stream, const Args& a) {
#ifdef DM_EMU
    g_lds.assign(bytes / 8 + 1, 0.0);
    emu::launch((unsigned)n_envs, kRows, [&]() { k_time_warp_align<Real>(a); });
#else
    if (bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_time_warp_align<Real>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(k_time_warp_align<Real>, dim3((unsigned)n_envs), dim3(kRows), bytes, stream, a);
#endif
    return 0;
}

}  // namespace dmw

extern "C" {

int dm_time_warp_dims(const dm_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return fail("dm_time_warp_dims: null argument");
    out[0] = ctx->c->precision == 64 ? 8 : 4; out[1] = 3 * ctx->c->hm.J;
    return 0;
}

int dm_time_warp_sample(dm_ctx* ctx, void* samples_dev, int32_t* count_dev, const int32_t* restart_dev, int capacity, int32_t* overflow_dev) {
    if (!ctx) return fail("dm_time_warp_sample: null ctx");
    if (!samples_dev || !count_dev || !overflow_dev) return fail("dm_time_warp_sample: null argument (only restart_dev may be NULL)");
    if (capacity < 2) return fail("dm_time_warp_sample: capacity must be >= 2 (a restart appends two samples)");
    CtxBase* c = ctx->c;
    if (c->hm.F < 1 || c->hm.frames.empty()) return fail("dm_time_warp_sample: the scene has no kinematic character to sample (no motion frames)");
    DevGuard guard(c->device_id);
    return launch_status(c->time_warp_sample(samples_dev, count_dev, restart_dev, capacity, overflow_dev));
}

int dm_time_warp_align(int device_id, int n_envs, int capacity, int dim, int f64, const void* samples_dev, const int32_t* count_dev, const int32_t* select_dev,
                       double term_step_cost, float* reward_out_dev, double* cost_out_dev, void* hip_stream) {
    if (n_envs < 1) return fail("dm_time_warp_align: n_envs must be >= 1");
    if (!samples_dev || !count_dev || !reward_out_dev) return fail("dm_time_warp_align: null argument (only select_dev and cost_out_dev may be NULL)");
    if (capacity < 2) return fail("dm_time_warp_align: capacity must be >= 2");
    if (dim < 3 || dim % 3 != 0) return fail("dm_time_warp_align: dim must be a positive multiple of 3 (points)");
    if (((uintptr_t)samples_dev & (f64 ? 7 : 3)) != 0 || ((uintptr_t)cost_out_dev & 7) != 0) return fail("dm_time_warp_align: misaligned pointer");
    const size_t bytes = dmw::lds_bytes(capacity, dim, f64);
    if (bytes > dmw::kLdsMax) return fail("dm_time_warp_align: capacity and dim need more LDS than a compute unit has (8 capacity + 192 (dim | 1) sizeof(Real) > 160 KB)");
    if (valid_device("dm_time_warp_align", device_id)) return -1;
    DevGuard guard(device_id);
    dmw::Args a;
    a.capacity = capacity; a.dim = dim; a.samples = samples_dev; a.count = count_dev; a.select = select_dev; a.term_step_cost = term_step_cost;
    a.reward = reward_out_dev; a.cost = cost_out_dev;
    const int rc = f64 ? dmw::launch_align<double>(n_envs, bytes, (rt_stream)hip_stream, a) : dmw::launch_align<float>(n_envs, bytes, (rt_stream)hip_stream, a);
    return launch_status(rc);
}

}  // extern "C"
