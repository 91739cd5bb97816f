// Episode returns, lengths and end-cause totals over a device-resident rollout: what the reference's learner logs as Train_Return / Test_Return -- path.calc_return()
// of the finished, valid paths (learning/path.py:45-46, learning/rl_agent.py:351-365, 456-466), a path with a non-finite value never being stored
// (learning/replay_buffer.py:102-112) -- plus episode lengths and the share of falls, for records that never leave HBM.  Included at the end of dm_host.cpp (shares its
// runtime shim); needs no env context.  The contract is in include/dm_hip.h (dm_episode_stats), the same recursion in numpy in deepmimic_amd/episodes.py.
//
// k_episode_scan   one lane per env column, forward in time, as k_td_lambda walks backwards: a row's loads are coalesced across the lanes of a wave, the three or four
//                  loads of row t + 1 are requested before row t's chain (one fp64 add, one int add) runs.  A lane keeps its column's partial totals -- 24 eight-byte
//                  words, every index a compile-time constant so that they stay in registers -- and the kThreads lanes of a workgroup reduce them by the tree of
//                  dmb::block_sum (t += t + w, w = 128 .. 1) over all 24 words at once: int adds, int max, fp64 adds, fp64 min / max.  Lane 0 writes the block's
//                  partial to the caller's workspace.  Lanes past N take part in the barriers with the neutral block.
// k_episode_fold   one workgroup behind it on the same stream: thread t adds the contiguous run of partials g = t * per .. in workgroup order, the same tree, and 24
//                  threads add the result into the caller's totals; steps_seen += T * N.
// Ordering is by the stream alone: no workgroup waits on another one, and there is no floating-point atomic, so every fp64 sum has one order for given (T, N) and two
// runs on one input give the same bytes.  The histogram is the one thing that does not go through the partials: the workspace is sized by N alone and cannot hold a
// histogram of caller-chosen length per workgroup, so a finished episode adds 1 to its bin of hist_dev with an INTEGER global atomic (exact whatever the arrival
// order; finished episodes are rare: about N per episode length in steps).
//
// Traffic: T x N x 16 bytes in (12 without `valid`) and 8 out when the per-step rows are asked for -- T = 32, N = 4096 is 3 MB.  The launches are latency-bound by
// construction: a column's chain is serial in t, and the per-step use (T = 1) is two launches over 64 KB.
#pragma once

namespace dme {

constexpr int kThreads = dmb::kThreads;          // workgroup width: one lane per env column
constexpr int kInt = 12, kDbl = 12;              // words [0, 12) of a block are int64, [12, 24) are fp64 (DM_EP_* of include/dm_hip.h)
constexpr int kWords = kInt + kDbl;
static_assert(kWords == DM_EP_STEPS_SEEN && DM_EP_TOTALS_WORDS == kWords + 1, "the totals block of include/dm_hip.h");
static_assert(DM_EP_EPISODES == 0 && DM_EP_STEPS == 4 && DM_EP_LEN_MAX == 8 && DM_EP_RET_SUM == 12 && DM_EP_RET_SQ == 15 && DM_EP_RET_MIN == 18 && DM_EP_RET_MAX == 21, "the totals block");

// one block of partial totals; i[0..3] episodes, i[4..7] steps, i[8..11] len_max, d[0..2] ret_sum, d[3..5] ret_sq, d[6..8] ret_min, d[9..11] ret_max
struct Part { long long i[kInt]; double d[kDbl]; };

DMP_DEV void part_clear(Part& p) {
#pragma unroll
    for (int k = 0; k < kInt; ++k) p.i[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) p.d[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { p.d[6 + k] = INFINITY; p.d[9 + k] = -INFINITY; }
}
// word k of a block, folded with the same word of another one: sums, max (lengths), min / max (returns; never NaN: class 3 has no return words)
DMP_DEV long long fold_int(int k, long long a, long long b) { return k < 8 ? a + b : (b > a ? b : a); }
DMP_DEV double fold_dbl(int k, double a, double b) { return k < 6 ? a + b : (k < 9 ? (b < a ? b : a) : (b > a ? b : a)); }
DMP_DEV void part_fold(Part& p, const long long* qi, const double* qd, int stride) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < kInt; ++k) p.i[k] = fold_int(k, p.i[k], qi[(size_t)k * stride]);
#pragma unroll
    for (int k = 0; k < kDbl; ++k) p.d[k] = fold_dbl(k, p.d[k], qd[(size_t)k * stride]);
}
// an episode of class c (0 .. 3) that ended with return `ret` after `len` steps.  Every index is a constant under the unrolled loop: no private array in scratch
DMP_DEV void part_finish(Part& p, int c, double ret, int len) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) if (c == k) { p.i[k] += 1; p.i[4 + k] += len; if (len > p.i[8 + k]) p.i[8 + k] = len; }
    const double sq = ret * ret;
#pragma unroll
    for (int k = 0; k < 3; ++k) if (c == k) { p.d[k] += ret; p.d[3 + k] += sq; if (ret < p.d[6 + k]) p.d[6 + k] = ret; if (ret > p.d[9 + k]) p.d[9 + k] = ret; }
}
// the blocks of the kThreads threads of a workgroup folded by the tree of dmb::block_sum; thread 0 holds the result.  ri / rd: kInt / kDbl rows of kThreads words of LDS
DMP_DEV void block_fold(Part& p, long long (*ri)[kThreads], double (*rd)[kThreads]) {
    const int t = (int)threadIdx.x;
    __syncthreads();                             // (a previous use of the rows is over)
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if (t >= w && t < 2 * w) {
#pragma unroll
            for (int k = 0; k < kInt; ++k) ri[k][t] = p.i[k];
#pragma unroll
            for (int k = 0; k < kDbl; ++k) rd[k][t] = p.d[k];
        }
        __syncthreads();
        if (t < w) part_fold(p, &ri[0][t + w], &rd[0][t + w], kThreads);          // (the next level writes columns [w / 2, w): none that is read here)
    }
}

#ifdef DM_EMU
inline void hist_add(long long* p) { *p += 1; }
#else
__device__ __forceinline__ void hist_add(long long* p) { atomicAdd(reinterpret_cast<unsigned long long*>(p), 1ull); }
#endif

struct Row { float r; int term, done, valid; };  // of step t: reward and flags

struct Args {
    int T, N;
    const float* rewards; const int *terminate, *done, *valid;
    double* acc_return; int* acc_len;
    float* ep_return; int* ep_len;
    long long* totals_i; double* totals_d;       // one block of DM_EP_TOTALS_WORDS words under both types, or null
    long long* hist; int bins, bin_steps;
    long long* work_i; double* work_d;           // [groups][kWords] under both types, or null (no totals wanted)
    int groups;
};

DMP_DEV Row load_row(const Args& a, int t, int n) {
    const size_t i = (size_t)t * a.N + n;
    Row w;
    w.r = a.rewards[i]; w.term = a.terminate[i]; w.done = a.done[i];
    w.valid = a.valid ? a.valid[i] : 1;
    return w;
}

__global__ void __launch_bounds__(256) k_episode_scan(Args a) {
#pragma clang fp contract(off)
    __shared__ long long ri[kInt][kThreads];
    __shared__ double rd[kDbl][kThreads];
    const int n = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    Part p; part_clear(p);
    if (n < a.N) {
        double acc = a.acc_return[n];
        int len = a.acc_len[n];
        Row cur = load_row(a, 0, n);
        for (int t = 0; t < a.T; ++t) {
            Row next = cur;
            if (t + 1 < a.T) next = load_row(a, t + 1, n);          // in flight while this row's chain runs
            acc = acc + (double)cur.r;
            len += 1;
            const size_t i = (size_t)t * a.N + n;
            if (a.ep_return) a.ep_return[i] = (float)acc;
            if (a.ep_len) a.ep_len[i] = len;
            if (cur.done != 0) {
                const bool finite = (acc - acc) == 0.0;             // false for +-inf and NaN
                const int c = (cur.valid == 0 || !finite) ? 3 : (cur.term == TERM_FAIL) ? 1 : (cur.term == TERM_SUCC) ? 2 : 0;
                part_finish(p, c, acc, len);
                if (a.hist && c < 3) {
                    long long b = ((long long)len - 1) / a.bin_steps;
                    b = b < 0 ? 0 : (b > a.bins - 1 ? a.bins - 1 : b);          // (a carry the caller filled with a length < 1 stays inside the array)
                    hist_add(a.hist + b);
                }
                acc = 0.0; len = 0;
            }
            cur = next;
        }
        a.acc_return[n] = acc; a.acc_len[n] = len;
    }
    if (!a.work_i) return;                       // (uniform over the grid: no totals wanted, no barrier below)
    block_fold(p, ri, rd);
    if (threadIdx.x == 0) {
        long long* wi = a.work_i + (size_t)blockIdx.x * kWords; double* wd = a.work_d + (size_t)blockIdx.x * kWords;
#pragma unroll
        for (int k = 0; k < kInt; ++k) wi[k] = p.i[k];
#pragma unroll
        for (int k = 0; k < kDbl; ++k) wd[kInt + k] = p.d[k];
    }
}

__global__ void __launch_bounds__(256) k_episode_fold(Args a) {
#pragma clang fp contract(off)
    __shared__ long long ri[kInt][kThreads];
    __shared__ double rd[kDbl][kThreads];
    const int t = (int)threadIdx.x;
    const int per = (a.groups + kThreads - 1) / kThreads, g0 = t * per, g1 = (g0 + per < a.groups) ? g0 + per : a.groups;
    Part p; part_clear(p);
    for (int g = g0; g < g1; ++g) part_fold(p, a.work_i + (size_t)g * kWords, a.work_d + (size_t)g * kWords + kInt, 1);
    block_fold(p, ri, rd);
    // thread 0 holds the window's block: through LDS to the 24 threads that add one word each into the caller's totals
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < kInt; ++k) ri[k][0] = p.i[k];
#pragma unroll
        for (int k = 0; k < kDbl; ++k) rd[k][0] = p.d[k];
    }
    __syncthreads();
    if (t < kInt) a.totals_i[t] = fold_int(t, a.totals_i[t], ri[t][0]);
    else if (t < kWords) a.totals_d[t] = fold_dbl(t - kInt, a.totals_d[t], rd[t - kInt][0]);
    else if (t == kWords) a.totals_i[DM_EP_STEPS_SEEN] += (long long)a.T * a.N;
}

inline int groups_of(int N) { return (N + kThreads - 1) / kThreads; }

}  // namespace dme

extern "C" {

int64_t dm_episode_workspace_bytes(int N) {
    if (N < 1) { fail("dm_episode_workspace_bytes: N must be >= 1"); return -1; }
    return (int64_t)dme::groups_of(N) * dme::kWords * 8;
}

int dm_episode_stats(int device_id, int T, int N, const float* rewards_dev, const int32_t* terminate_dev, const int32_t* done_dev, const int32_t* valid_dev,
                     double* acc_return_dev, int32_t* acc_len_dev, float* ep_return_out, int32_t* ep_len_out, void* totals_dev, int64_t* hist_dev, int bins, int bin_steps,
                     void* work_dev, int64_t work_bytes, void* hip_stream) {
    if (T < 1 || N < 1) return fail("dm_episode_stats: T and N must be >= 1");
    if ((long long)T * N > 0x7fffffffLL) return fail("dm_episode_stats: too many elements for one call");
    if (!rewards_dev || !terminate_dev || !done_dev || !acc_return_dev || !acc_len_dev)
        return fail("dm_episode_stats: null argument (rewards, terminate, done, acc_return and acc_len are required)");
    if (hist_dev && (bins < 1 || bin_steps < 1)) return fail("dm_episode_stats: a histogram needs bins >= 1 and bin_steps >= 1");
    if ((totals_dev || hist_dev) && (!work_dev || work_bytes < dm_episode_workspace_bytes(N))) return fail("dm_episode_stats: workspace too small (dm_episode_workspace_bytes)");
    if ((((uintptr_t)acc_return_dev | (uintptr_t)totals_dev | (uintptr_t)hist_dev | (uintptr_t)((totals_dev || hist_dev) ? work_dev : nullptr)) & 7) != 0)
        return fail("dm_episode_stats: acc_return, totals, hist and the workspace must be 8-byte aligned");
    if (valid_device("dm_episode_stats", device_id)) return -1;
    DevGuard guard(device_id);
    dme::Args a;
    a.T = T; a.N = N; a.rewards = rewards_dev; a.terminate = terminate_dev; a.done = done_dev; a.valid = valid_dev;
    a.acc_return = acc_return_dev; a.acc_len = acc_len_dev; a.ep_return = ep_return_out; a.ep_len = ep_len_out;
    a.totals_i = (long long*)totals_dev; a.totals_d = (double*)totals_dev;
    a.hist = (long long*)hist_dev; a.bins = bins; a.bin_steps = bin_steps;
    a.work_i = totals_dev ? (long long*)work_dev : nullptr; a.work_d = totals_dev ? (double*)work_dev : nullptr;      // partials only where they will be folded
    a.groups = dme::groups_of(N);
    rt_stream stream = (rt_stream)hip_stream;
    RT_LAUNCH4(dme::k_episode_scan, a.groups, stream, a);
    if (totals_dev) RT_LAUNCH4(dme::k_episode_fold, 1, stream, a);
    return launch_status(0);
}

}  // extern "C"
