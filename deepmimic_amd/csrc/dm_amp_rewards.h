// AMP batch rewards, their statistics and the critic's value bounds over a device-resident rollout: what the reference's AMPAgent does between _update_disc and the
// returns -- _batch_calc_reward (learning/amp_agent.py:393-421: the scaled style reward of the WHOLE stored rollout from the discriminator as it is after its update,
// Disc_Reward_Mean / Disc_Reward_Std over it, the blend with the task reward, the running reward_min / reward_max), _lerp_reward (:423-425) and the value clip of
// _compute_batch_vals (:436-443) -- for records that never leave HBM and bounds the host never reads.  Included at the end of dm_host.cpp (shares its runtime shim);
// needs no env context.  The contract is in include/dm_hip.h (dm_amp_batch_rewards, dm_amp_value_clip), the same arithmetic in numpy in deepmimic_amd/amp_rewards.py.
//
// dm_amp_batch_rewards: four short launches ordered by the stream alone (no workgroup waits on another one, no atomics):
//     k_amp_scan   one lane per env column, backwards in time like k_td_lambda: a row's loads are coalesced across the lanes of a wave, the loads of row t - 1 are
//                  requested before row t's arithmetic runs, and the flag "the episode the scan is inside ended invalid" travels down the column -- the mask rule of
//                  k_td_lambda, from the flags alone.  Every row gets its reward (dmp::style_reward / dmp::style_blend: the functions of the scalar head's epilogue)
//                  and its mask; the column's COUNTED rows (mask 1) give a partial {count, fp64 sum of s, min r, max r}; the kScan lanes of a workgroup fold their
//                  partials by a fixed tree through LDS and lane 0 writes the group's partial to the caller's workspace.
//     k_amp_fold   one workgroup: thread t folds the contiguous run of group partials g = t * per .. in order, the same tree over kFold threads; n, the mean and this
//                  call's min / max go to stats_out, and the running bounds take them in (n = 0: untouched).
//     k_amp_dev    the scan again, reading only logits and flags: the fp64 sum of (s - mean)^2 over the counted rows, folded the same way.
//     k_amp_std    one workgroup: stats_out[DM_AMP_STAT_STD] = sqrt(sum / n)              (two passes: the mean, then the squared deviations)
// Every fp64 sum has one order for given (T, N): a column's counted rows in scan order (t = T - 1 down to 0), the kScan columns of a group by the tree
// (x[t] += x[t + w], w = kScan / 2 .. 1; lanes past N hold the neutral partial), the groups in contiguous runs per thread of the folding workgroup and the tree over
// kFold.  No product is contracted into a sum.  Two calls on one input give the same bytes.  min / max propagate a NaN (nan_min / nan_max below), as np.amin /
// np.minimum do: a NaN reward of a counted row stays visible in the bounds; rows that are not counted reach neither the bounds nor the statistics.
//
// dm_amp_value_clip: one launch, one element per thread: lo / hi from the device-resident bounds, then dmp::value_clip -- the expression of HEAD_VALUE.
//
// Traffic at T = 32, N = 4096: 0.5 MB per array, at most five arrays in and two out; every launch is latency-bound (a column's chain is serial in t).
#pragma once

namespace dma {

constexpr int kScan = 64;                        // lanes (env columns) per workgroup of the two scans: one wavefront, so N = 4096 spreads over 64 workgroups
constexpr int kFold = dmb::kThreads;             // threads of the one-workgroup folds
static_assert(DM_AMP_STAT_N == 0 && DM_AMP_STAT_MEAN == 1 && DM_AMP_STAT_STD == 2 && DM_AMP_STAT_MIN == 3 && DM_AMP_STAT_MAX == 4 && DM_AMP_STATS_WORDS == 5, "stats_out of include/dm_hip.h");

// min / max that keep a NaN of either side (np.minimum / np.maximum; fminf / fmaxf would drop it)
DMP_DEV float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
DMP_DEV float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// a partial over counted rows: their number, the fp64 sum (of s in the first scan, of (s - mean)^2 in the second), min and max of r
struct Part { double sum; int cnt; float mn, mx; };
DMP_DEV Part part_neutral() { Part p; p.sum = 0.0; p.cnt = 0; p.mn = INFINITY; p.mx = -INFINITY; return p; }
DMP_DEV void part_fold(Part& p, double sum, int cnt, float mn, float mx) { p.sum += sum; p.cnt += cnt; p.mn = nan_min(p.mn, mn); p.mx = nan_max(p.mx, mx); }

// group partials in the caller's workspace: [sum G doubles][sq G doubles][cnt G ints][min G floats][max G floats]
struct Work { double* sum; double* sq; int* cnt; float* mn; float* mx; };
inline Work carve(void* ws, int groups) {
    Work w; w.sum = (double*)ws; w.sq = w.sum + groups; w.cnt = (int*)(w.sq + groups); w.mn = (float*)(w.cnt + groups); w.mx = w.mn + groups;
    return w;
}
inline int groups_of(int N) { return (N + kScan - 1) / kScan; }

template <int W> struct Lds { double sum[W]; int cnt[W]; float mn[W], mx[W]; };
// the partials of the W threads of a workgroup folded by the tree of dmb::block_sum; thread 0 holds the result
template <int W> DMP_DEV void block_fold(Part& p, Lds<W>& l) {
    const int t = (int)threadIdx.x;
    __syncthreads();                             // (a previous use of `l` is over)
    l.sum[t] = p.sum; l.cnt[t] = p.cnt; l.mn[t] = p.mn; l.mx[t] = p.mx;
    __syncthreads();
    for (int w = W / 2; w >= 1; w >>= 1) {
        if (t < w) { l.sum[t] += l.sum[t + w]; l.cnt[t] += l.cnt[t + w]; l.mn[t] = nan_min(l.mn[t], l.mn[t + w]); l.mx[t] = nan_max(l.mx[t], l.mx[t + w]); }
        __syncthreads();
    }
    p.sum = l.sum[0]; p.cnt = l.cnt[0]; p.mn = l.mn[0]; p.mx = l.mx[0];
}

struct Args {
    int T, N;
    const float *logits, *task_r; const int *done, *valid;
    float scale, lerp;
    float* rewards; int* mask; float* bounds; double* stats;
    Work w; int groups;
};

struct Row { float y, tr; int done, valid; };    // of step t: logit, task reward, flags
// SECOND: the scan of the squared deviations reads no task reward
template <bool SECOND> DMP_DEV Row load_row(const Args& a, int t, int n) {
    const size_t i = (size_t)t * a.N + n;
    Row w;
    w.y = a.logits[i]; w.tr = (!SECOND && a.task_r) ? a.task_r[i] : 0.0f;
    w.valid = a.valid ? a.valid[i] : 1; w.done = a.valid ? a.done[i] : 0;          // (without `valid` no episode is invalid: `done` is not read)
    return w;
}

// One column, backwards in time.  First scan: rewards_out, mask_out, and {count, sum of s, min r, max r} of the counted rows; SECOND: the sum of (s - mean)^2 of the
// same rows.  Lanes past N take part in the barriers with the neutral partial.
template <bool SECOND> DMP_DEV void scan(const Args& a, double* part_sum) {
#pragma clang fp contract(off)
    __shared__ Lds<kScan> lds;
    const int n = (int)blockIdx.x * kScan + (int)threadIdx.x;
    Part p = part_neutral();
    if (n < a.N) {
        const double mean = SECOND ? a.stats[DM_AMP_STAT_MEAN] : 0.0;
        bool invalid = false;                    // the episode the scan is inside ended invalid
        Row cur = load_row<SECOND>(a, a.T - 1, n);
        for (int t = a.T - 1; t >= 0; --t) {
            Row prev = cur;
            if (t > 0) prev = load_row<SECOND>(a, t - 1, n);          // in flight while this row's arithmetic runs
            if (cur.done != 0) invalid = cur.valid == 0;
            const float s = dmp::style_reward(cur.y, a.scale);
            if (SECOND) {
                if (!invalid) { const double d = (double)s - mean; p.sum += d * d; }
            } else {
                const float r = a.task_r ? dmp::style_blend(a.lerp, cur.tr, s) : s;
                const size_t i = (size_t)t * a.N + n;
                a.rewards[i] = r;
                if (a.mask) a.mask[i] = invalid ? 0 : 1;
                if (!invalid) part_fold(p, (double)s, 1, r, r);
            }
            cur = prev;
        }
    }
    block_fold(p, lds);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = p.sum;
        if (!SECOND) { a.w.cnt[blockIdx.x] = p.cnt; a.w.mn[blockIdx.x] = p.mn; a.w.mx[blockIdx.x] = p.mx; }
    }
}

__global__ void __launch_bounds__(64) k_amp_scan(Args a) { scan<false>(a, a.w.sum); }
__global__ void __launch_bounds__(64) k_amp_dev(Args a) { scan<true>(a, a.w.sq); }

__global__ void __launch_bounds__(256) k_amp_fold(Args a) {
#pragma clang fp contract(off)
    __shared__ Lds<kFold> lds;
    const int t = (int)threadIdx.x;
    const int per = (a.groups + kFold - 1) / kFold, g0 = t * per, g1 = (g0 + per < a.groups) ? g0 + per : a.groups;
    Part p = part_neutral();
    for (int g = g0; g < g1; ++g) part_fold(p, a.w.sum[g], a.w.cnt[g], a.w.mn[g], a.w.mx[g]);
    block_fold(p, lds);
    if (t == 0) {
        a.stats[DM_AMP_STAT_N] = (double)p.cnt;
        a.stats[DM_AMP_STAT_MEAN] = p.cnt > 0 ? p.sum / (double)p.cnt : 0.0;
        a.stats[DM_AMP_STAT_MIN] = (double)p.mn; a.stats[DM_AMP_STAT_MAX] = (double)p.mx;
        if (p.cnt > 0) { a.bounds[0] = nan_min(a.bounds[0], p.mn); a.bounds[1] = nan_max(a.bounds[1], p.mx); }
    }
}

__global__ void __launch_bounds__(256) k_amp_std(Args a) {
    __shared__ double red[kFold];
    const double sq = dmb::fold_groups(a.w.sq, a.groups, red);
    const double n = a.stats[DM_AMP_STAT_N];
    if (threadIdx.x == 0) a.stats[DM_AMP_STAT_STD] = n > 0.0 ? sqrt(sq / n) : 0.0;
}

struct ClipArgs { int n; const float *values, *bounds; double discount; const int* row_mask; float fill; float* out; };

__global__ void __launch_bounds__(256) k_amp_clip(ClipArgs c) {
    const long long i = (long long)blockIdx.x * kFold + (long long)threadIdx.x;
    if (i >= c.n) return;
    const double span = 1.0 - c.discount;
    const float lo = (float)((double)c.bounds[0] / span), hi = (float)((double)c.bounds[1] / span);
    float v = c.fill;
    if (!c.row_mask || c.row_mask[i] != 0) v = dmp::value_clip(c.values[i], lo, hi);
    c.out[i] = v;
}

}  // namespace dma

extern "C" {

int64_t dm_amp_batch_rewards_workspace(int T, int N) {
    if (T < 1 || N < 1) { fail("dm_amp_batch_rewards_workspace: T and N must be >= 1"); return -1; }
    if ((long long)T * N > 0x7fffffffLL) { fail("dm_amp_batch_rewards_workspace: too many elements for one call"); return -1; }
    return (int64_t)dma::groups_of(N) * 32;      // 2 doubles, an int and 2 floats per group, rounded up to whole 8-byte words
}

int dm_amp_batch_rewards(int device_id, int T, int N, const float* logits_dev, const float* task_reward_dev, const int32_t* done_dev, const int32_t* valid_dev,
                         double reward_scale, double task_reward_lerp, float* rewards_out, int32_t* mask_out, float* bounds_dev, double* stats_out,
                         void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (T < 1 || N < 1) return fail("dm_amp_batch_rewards: T and N must be >= 1");
    if ((long long)T * N > 0x7fffffffLL) return fail("dm_amp_batch_rewards: too many elements for one call");
    if (!logits_dev || !rewards_out || !bounds_dev || !stats_out || !workspace)
        return fail("dm_amp_batch_rewards: null argument (only task_reward, done, valid and mask_out may be NULL)");
    if (valid_dev && !done_dev) return fail("dm_amp_batch_rewards: valid needs done (done may be NULL only where valid is)");
    if (task_reward_dev && !(task_reward_lerp >= 0.0 && task_reward_lerp <= 1.0)) return fail("dm_amp_batch_rewards: a task reward needs task_reward_lerp in [0, 1]");
    if (workspace_bytes < dm_amp_batch_rewards_workspace(T, N)) return fail("dm_amp_batch_rewards: workspace too small (dm_amp_batch_rewards_workspace)");
    if ((((uintptr_t)workspace | (uintptr_t)stats_out) & 7) != 0) return fail("dm_amp_batch_rewards: workspace and stats_out must be 8-byte aligned");
    if (valid_device("dm_amp_batch_rewards", device_id)) return -1;
    DevGuard guard(device_id);
    dma::Args a;
    a.T = T; a.N = N; a.logits = logits_dev; a.task_r = task_reward_dev; a.done = done_dev; a.valid = valid_dev;
    a.scale = (float)reward_scale; a.lerp = task_reward_dev ? (float)task_reward_lerp : 0.0f;
    a.rewards = rewards_out; a.mask = mask_out; a.bounds = bounds_dev; a.stats = stats_out;
    a.groups = dma::groups_of(N); a.w = dma::carve(workspace, a.groups);
    rt_stream stream = (rt_stream)hip_stream;
    RT_LAUNCH(dma::k_amp_scan, a.groups, stream, a);
    RT_LAUNCH4(dma::k_amp_fold, 1, stream, a);
    RT_LAUNCH(dma::k_amp_dev, a.groups, stream, a);
    RT_LAUNCH4(dma::k_amp_std, 1, stream, a);
    return launch_status(0);
}

int dm_amp_value_clip(int device_id, int n, const float* values_dev, const float* bounds_dev, double discount, const int32_t* row_mask_dev, double fill,
                      float* out_dev, void* hip_stream) {
    if (n < 1) return fail("dm_amp_value_clip: n must be >= 1");
    if (!values_dev || !bounds_dev || !out_dev) return fail("dm_amp_value_clip: null argument (only row_mask may be NULL)");
    if (!(discount >= 0.0 && discount < 1.0)) return fail("dm_amp_value_clip: discount must be in [0, 1)");
    if (valid_device("dm_amp_value_clip", device_id)) return -1;
    DevGuard guard(device_id);
    dma::ClipArgs c;
    c.n = n; c.values = values_dev; c.bounds = bounds_dev; c.discount = discount; c.row_mask = row_mask_dev; c.fill = (float)fill; c.out = out_dev;
    RT_LAUNCH4(dma::k_amp_clip, ((long long)n + dma::kFold - 1) / dma::kFold, (rt_stream)hip_stream, c);
    return launch_status(0);
}

}  // extern "C"
