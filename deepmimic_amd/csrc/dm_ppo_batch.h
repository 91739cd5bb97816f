// PPO training batches from a device-resident rollout: what the reference's PPOAgent._train_step (learning/ppo_agent.py:141-232) does between the returns and the
// first optimiser step -- the advantage over the explored samples, normalised and clipped (:166-172), the clipped critic targets (:167), the lists of valid and of
// explored samples, a fresh shuffle of both per epoch (:190, 211) and the gather of a minibatch's rows with wrap-around (:186-193).  Included at the end of dm_host.cpp
// (shares its runtime shim); needs no env context.
//
// dm_ppo_advantages: five short launches over the flat [T * N] arrays, ordered by the stream alone (no workgroup waits on another one, no atomics):
//     k_ppo_count    per group of kChunk samples: number of valid / exp samples and the fp64 sum of a = returns - values over the exp ones
//     k_ppo_fold     one workgroup: exclusive scan of the group counts (the groups' first slots in the two lists), the totals into counts_out, the mean into stats_out[0]
//     k_ppo_compact  per group: a stable compaction of its valid / exp indices behind the group's first slot, the clipped targets, and the sum of (a - mean)^2
//     k_ppo_std      one workgroup: stats_out[1] = sqrt(sum / n_exp)                 (two passes: the mean, then the squared deviations)
//     k_ppo_apply    adv_out = clip((a - mean) / (std + eps)) on exp samples, 0 elsewhere
// Every sum is taken in a fixed order -- a thread's samples in index order, the 256 threads of a workgroup by a fixed tree through LDS, the groups in contiguous runs
// per thread of the folding workgroup and the same tree -- so two runs on one input are bit-identical.  Memory-light: T = 32, N = 4096 is 0.5 MB per array, the
// launches are latency-bound.
//
// dm_ppo_gather: one launch copies `rows` rows of up to 8 columns.  The row at position p of the (endless) shuffled pass over a list is idx[perm(slot)], slot = p % count,
// with a fresh permutation for every pass = p / count: perm is a keyed bijection on [0, count) evaluated per row (a cycle-walking balanced Feistel network on Philox4x32-10,
// feistel_perm below), so there is no stored permutation and no sort.  A wavefront owns kGatherRows consecutive destination rows: lanes 0 .. kGatherRows - 1 each walk
// one row's permutation, then all 64 lanes copy the tile column by column, coalesced along a row on the source side and across the whole tile on the destination side.
#pragma once

namespace dmb {

constexpr int kThreads = 256;
constexpr int kPer = 4;                          // consecutive samples per thread (a thread's samples stay in index order: the compaction is stable)
constexpr int kChunk = kThreads * kPer;          // samples per workgroup = per partial
constexpr int kGatherRows = 4;                   // destination rows per wavefront of k_ppo_gather
constexpr int kMaxCols = 8;

// per-group partials in the caller's workspace: [sum G doubles][sq G doubles][count G x {valid, exp}][first G x {valid, exp}]
struct Work { double* sum; double* sq; int* cnt; int* first; };
inline Work carve(void* ws, int groups) {
    Work w; w.sum = (double*)ws; w.sq = w.sum + groups; w.cnt = (int*)(w.sq + groups); w.first = w.cnt + 2 * (size_t)groups;
    return w;
}
inline int groups_of(long long total) { return (int)((total + kChunk - 1) / kChunk); }

struct AdvArgs {
    int total;                                   // T * N
    const float *returns, *values; const int *mask, *exp_flags;
    double adv_eps, adv_clip, val_min, val_max;
    float *adv, *targets; int *valid_idx, *exp_idx, *counts; double* stats;
    Work w; int groups;
};

// the sum of one double per thread of a 256-thread workgroup, by a fixed tree; every thread gets it.  `red`: 256 doubles of LDS
DMP_DEV double block_sum(double v, double* red) {
    const int t = (int)threadIdx.x;
    __syncthreads();                             // (a previous use of `red` is over)
    red[t] = v;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}
// inclusive scan of one unsigned per thread of a 256-thread workgroup (Hillis-Steele through LDS); `sc`: 256 words of LDS
DMP_DEV unsigned block_scan(unsigned v, unsigned* sc) {
    const int t = (int)threadIdx.x;
    __syncthreads();
    sc[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const unsigned add = (t >= d) ? sc[t - d] : 0u;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    return sc[t];
}

// a thread's kPer samples: bit k of `valid` / `exp` and a[k] = returns - values (fp64) where the sample exists
struct Mine { unsigned valid, exp; double a[kPer]; long long i0; };
DMP_DEV Mine load_mine(const AdvArgs& p) {
    Mine m; m.valid = m.exp = 0u;
    m.i0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPer;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const long long i = m.i0 + k;
        m.a[k] = 0.0;
        if (i < p.total) {
            const bool v = p.mask ? p.mask[i] != 0 : true;
            const bool e = v && (p.exp_flags ? p.exp_flags[i] != 0 : true);
            if (v) m.valid |= 1u << k;
            if (e) m.exp |= 1u << k;
            if (e) m.a[k] = (double)p.returns[i] - (double)p.values[i];
        }
    }
    return m;
}
DMP_DEV unsigned bits4(unsigned m) { return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u); }

__global__ void __launch_bounds__(256) k_ppo_count(AdvArgs p) {
    __shared__ double red[kThreads];
    __shared__ unsigned sc[kThreads];
    const Mine m = load_mine(p);
    double s = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) if (m.exp >> k & 1u) s += m.a[k];
    const double sum = block_sum(s, red);
    // both counts in one word: a group holds at most kChunk = 1024 < 2^16 samples
    const unsigned c = block_scan(bits4(m.valid) | (bits4(m.exp) << 16), sc);
    if (threadIdx.x == kThreads - 1) {
        p.w.sum[blockIdx.x] = sum; p.w.cnt[2 * (size_t)blockIdx.x] = (int)(c & 0xffffu); p.w.cnt[2 * (size_t)blockIdx.x + 1] = (int)(c >> 16);
    }
}

// the sum over the groups of part[g], every thread gets it: thread t adds the contiguous run g = t * per .. in order, then the tree
DMP_DEV double fold_groups(const double* part, int groups, double* red) {
    const int per = (groups + kThreads - 1) / kThreads, g0 = (int)threadIdx.x * per, g1 = (g0 + per < groups) ? g0 + per : groups;
    double s = 0;
    for (int g = g0; g < g1; ++g) s += part[g];
    return block_sum(s, red);
}

__global__ void __launch_bounds__(256) k_ppo_fold(AdvArgs p) {
    __shared__ double red[kThreads];
    __shared__ int run[2][kThreads];
    const int t = (int)threadIdx.x;
    const int per = (p.groups + kThreads - 1) / kThreads, g0 = t * per, g1 = (g0 + per < p.groups) ? g0 + per : p.groups;
    int nv = 0, ne = 0;                          // (no sum passes total <= 2^31 - 1)
    for (int g = g0; g < g1; ++g) { nv += p.w.cnt[2 * (size_t)g]; ne += p.w.cnt[2 * (size_t)g + 1]; }
    run[0][t] = nv; run[1][t] = ne;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int av = (t >= d) ? run[0][t - d] : 0, ae = (t >= d) ? run[1][t - d] : 0;
        __syncthreads();
        run[0][t] += av; run[1][t] += ae;
        __syncthreads();
    }
    int fv = run[0][t] - nv, fe = run[1][t] - ne;           // exclusive: the first slots of this thread's run of groups
    for (int g = g0; g < g1; ++g) {
        p.w.first[2 * (size_t)g] = fv; p.w.first[2 * (size_t)g + 1] = fe;
        fv += p.w.cnt[2 * (size_t)g]; fe += p.w.cnt[2 * (size_t)g + 1];
    }
    const int n_valid = run[0][kThreads - 1], n_exp = run[1][kThreads - 1];
    const double sum = fold_groups(p.w.sum, p.groups, red);
    if (t == 0) { p.counts[0] = n_valid; p.counts[1] = n_exp; p.stats[0] = n_exp > 0 ? sum / (double)n_exp : 0.0; }
}

__global__ void __launch_bounds__(256) k_ppo_compact(AdvArgs p) {
    __shared__ double red[kThreads];
    __shared__ unsigned sc[kThreads];
    const Mine m = load_mine(p);
    const double mean = p.stats[0];
    double q = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) if (m.exp >> k & 1u) { const double d = m.a[k] - mean; q += d * d; }
    const double sq = block_sum(q, red);
    const unsigned mine = bits4(m.valid) | (bits4(m.exp) << 16);
    const unsigned before = block_scan(mine, sc) - mine;
    int sv = p.w.first[2 * (size_t)blockIdx.x] + (int)(before & 0xffffu), se = p.w.first[2 * (size_t)blockIdx.x + 1] + (int)(before >> 16);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const long long i = m.i0 + k;
        if (i < p.total) {
            if (m.valid >> k & 1u) p.valid_idx[sv++] = (int)i;
            if (m.exp >> k & 1u) p.exp_idx[se++] = (int)i;
            const double r = (double)p.returns[i];
            p.targets[i] = (float)(r < p.val_min ? p.val_min : (r > p.val_max ? p.val_max : r));
        }
    }
    if (threadIdx.x == 0) p.w.sq[blockIdx.x] = sq;
}

__global__ void __launch_bounds__(256) k_ppo_std(AdvArgs p) {
    __shared__ double red[kThreads];
    const double sq = fold_groups(p.w.sq, p.groups, red);
    const int n_exp = p.counts[1];
    if (threadIdx.x == 0) p.stats[1] = n_exp > 0 ? sqrt(sq / (double)n_exp) : 0.0;
}

__global__ void __launch_bounds__(256) k_ppo_apply(AdvArgs p) {
    const Mine m = load_mine(p);
    const double mean = p.stats[0], denom = p.stats[1] + p.adv_eps;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const long long i = m.i0 + k;
        if (i < p.total) {
            double x = 0.0;
            if (m.exp >> k & 1u) { x = (m.a[k] - mean) / denom; x = x < -p.adv_clip ? -p.adv_clip : (x > p.adv_clip ? p.adv_clip : x); }
            p.adv[i] = (float)x;
        }
    }
}

// ---- the shuffle: a keyed bijection on [0, count), count >= 1.  k = max(1, bit_length(count - 1)), h = ceil(k / 2), m = 2^h - 1; x = (L, R) = (x >> h, x & m);
// six rounds (L, R) <- (R, L ^ (F & m)) with F = word 0 of Philox4x32-10(counter = (R, round, epoch, pass), key = seed); y = (L << h) | R, and while y >= count the
// six rounds again (cycle walking: the walk follows a cycle of a bijection of [0, 2^(2h)) that starts inside [0, count), so it comes back).
DMP_DEV uint32_t feistel_perm(uint32_t x, uint32_t count, uint32_t seed_lo, uint32_t seed_hi, uint32_t epoch, uint32_t pass) {
    int k = 1;
    while (k < 32 && ((count - 1u) >> k) != 0u) ++k;
    const int h = (k + 1) / 2;
    const uint32_t msk = (1u << h) - 1u;
    uint32_t y = x;
    do {
        uint32_t L = y >> h, R = y & msk;
        for (uint32_t r = 0; r < 6; ++r) {
            uint32_t f[4]; dmp::philox4x32_10(R, r, epoch, pass, seed_lo, seed_hi, f);
            const uint32_t nr = L ^ (f[0] & msk);
            L = R; R = nr;
        }
        y = (L << h) | R;
    } while (y >= count);
    return y;
}

struct alignas(16) Q4 { uint32_t x, y, z, w; };  // one 16-byte load / store
// one wavefront copies a tile of n = rows * w elements (dwords, or 16-byte quads): element e is column e % w of tile row e / w, read from source row srow[.]
template <typename E> DMP_DEV void gather_tile(const E* src, E* dst, const int* srow, unsigned w, unsigned n, unsigned l) {
    for (unsigned e = l; e < n; e += 64u) { const unsigned r = e / w; dst[e] = src[(size_t)srow[r] * w + (e - r * w)]; }
}
struct GatherCol { const uint32_t* src; uint32_t* dst; int width, vec; };      // vec: both bases and width * 4 are multiples of 16
struct GatherArgs {
    const int* idx; const int* count; long long first; int rows; uint32_t seed_lo, seed_hi, epoch; int ncols; int* picked;
    GatherCol col[kMaxCols];
};

__global__ void __launch_bounds__(64) k_ppo_gather(GatherArgs g) {
    __shared__ int srow[kGatherRows];
    const int l = (int)threadIdx.x;
    const long long j0 = (long long)blockIdx.x * kGatherRows;
    const int nr = (g.rows - j0 < kGatherRows) ? (int)(g.rows - j0) : kGatherRows;      // rows of this tile (>= 1 by the grid size)
    const int count = *g.count;
    if (l < nr) {
        int s = -1;
        if (count > 0) {
            const long long p = g.first + j0 + l;
            const uint32_t pass = (uint32_t)(p / count), slot = (uint32_t)(p % count);
            s = g.idx[feistel_perm(slot, (uint32_t)count, g.seed_lo, g.seed_hi, g.epoch, pass)];
        }
        srow[l] = s;
        if (g.picked) g.picked[j0 + l] = s;
    }
    __syncthreads();
    if (count <= 0) return;
    for (int c = 0; c < g.ncols; ++c) {
        const GatherCol col = g.col[c];
        if (col.vec) {                            // 16 bytes per lane
            const unsigned w4 = (unsigned)col.width / 4u;
            gather_tile(reinterpret_cast<const Q4*>(col.src), reinterpret_cast<Q4*>(col.dst) + (size_t)j0 * w4, srow, w4, (unsigned)nr * w4, (unsigned)l);
        } else {
            const unsigned w = (unsigned)col.width;
            gather_tile(col.src, col.dst + (size_t)j0 * w, srow, w, (unsigned)nr * w, (unsigned)l);
        }
    }
}

}  // namespace dmb

extern "C" {

int64_t dm_ppo_workspace_bytes(int T, int N) {
    if (T < 1 || N < 1) { fail("dm_ppo_workspace_bytes: T and N must be >= 1"); return -1; }
    if ((long long)T * N > 0x7fffffffLL) { fail("dm_ppo_workspace_bytes: too many elements for one call"); return -1; }
    return (int64_t)dmb::groups_of((long long)T * N) * (2 * sizeof(double) + 4 * sizeof(int32_t));
}

int dm_ppo_advantages(int device_id, int T, int N, const float* returns_dev, const float* values_dev, const int32_t* mask_dev, const int32_t* exp_flags_dev,
                      double adv_eps, double norm_adv_clip, double val_min, double val_max, float* adv_out, float* targets_out, int32_t* valid_idx_out,
                      int32_t* exp_idx_out, int32_t* counts_out, double* stats_out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (T < 1 || N < 1) return fail("dm_ppo_advantages: T and N must be >= 1");
    if ((long long)T * N > 0x7fffffffLL) return fail("dm_ppo_advantages: too many elements for one call");
    if (!returns_dev || !values_dev || !adv_out || !targets_out || !valid_idx_out || !exp_idx_out || !counts_out || !stats_out || !workspace)
        return fail("dm_ppo_advantages: null argument (only mask and exp_flags may be NULL)");
    if (!(adv_eps >= 0)) return fail("dm_ppo_advantages: adv_eps must be >= 0");
    if (!(norm_adv_clip > 0)) return fail("dm_ppo_advantages: norm_adv_clip must be > 0");
    if (!(val_min <= val_max)) return fail("dm_ppo_advantages: val_min must be <= val_max (infinite bounds: no clipping)");
    if (workspace_bytes < dm_ppo_workspace_bytes(T, N)) return fail("dm_ppo_advantages: workspace too small (dm_ppo_workspace_bytes)");
    if ((((uintptr_t)workspace | (uintptr_t)stats_out) & 7) != 0) return fail("dm_ppo_advantages: workspace and stats_out must be 8-byte aligned");
    if (valid_device("dm_ppo_advantages", device_id)) return -1;
    DevGuard guard(device_id);
    dmb::AdvArgs p;
    p.total = T * N; p.returns = returns_dev; p.values = values_dev; p.mask = mask_dev; p.exp_flags = exp_flags_dev;
    p.adv_eps = adv_eps; p.adv_clip = norm_adv_clip; p.val_min = val_min; p.val_max = val_max;
    p.adv = adv_out; p.targets = targets_out; p.valid_idx = valid_idx_out; p.exp_idx = exp_idx_out; p.counts = counts_out; p.stats = stats_out;
    p.groups = dmb::groups_of(p.total); p.w = dmb::carve(workspace, p.groups);
    rt_stream stream = (rt_stream)hip_stream;
    RT_LAUNCH4(dmb::k_ppo_count, p.groups, stream, p);
    RT_LAUNCH4(dmb::k_ppo_fold, 1, stream, p);
    RT_LAUNCH4(dmb::k_ppo_compact, p.groups, stream, p);
    RT_LAUNCH4(dmb::k_ppo_std, 1, stream, p);
    RT_LAUNCH4(dmb::k_ppo_apply, p.groups, stream, p);
    return launch_status(0);
}

int dm_ppo_gather(int device_id, const int32_t* idx_dev, const int32_t* count_dev, int64_t first, int rows, uint64_t seed, uint32_t epoch, int ncols,
                  const dm_ppo_column* cols, int32_t* picked_out, void* hip_stream) {
    if (!idx_dev || !count_dev || !cols) return fail("dm_ppo_gather: null argument (only picked_out may be NULL)");
    if (first < 0) return fail("dm_ppo_gather: first must be >= 0");
    if (rows < 1) return fail("dm_ppo_gather: rows must be >= 1");
    if (ncols < 1 || ncols > dmb::kMaxCols) return fail("dm_ppo_gather: 1 to 8 columns per call");
    dmb::GatherArgs g;
    for (int c = 0; c < ncols; ++c) {
        if (!cols[c].src || !cols[c].dst) return fail("dm_ppo_gather: null column pointer");
        if (cols[c].width < 1) return fail("dm_ppo_gather: column width must be >= 1");
        if ((((uintptr_t)cols[c].src | (uintptr_t)cols[c].dst) & 3) != 0) return fail("dm_ppo_gather: columns are arrays of 4-byte elements (misaligned pointer)");
        g.col[c].src = (const uint32_t*)cols[c].src; g.col[c].dst = (uint32_t*)cols[c].dst; g.col[c].width = cols[c].width;
        // 16 bytes per lane only where every row of both arrays starts on a 16-byte boundary (S = 227 rows are 908 B: dwords)
        g.col[c].vec = rows_vec16(cols[c].width, {cols[c].src, cols[c].dst});
    }
    for (int c = ncols; c < dmb::kMaxCols; ++c) { g.col[c].src = nullptr; g.col[c].dst = nullptr; g.col[c].width = 0; g.col[c].vec = 0; }
    if (valid_device("dm_ppo_gather", device_id)) return -1;
    DevGuard guard(device_id);
    g.idx = idx_dev; g.count = count_dev; g.first = first; g.rows = rows; g.seed_lo = (uint32_t)(seed & 0xffffffffu); g.seed_hi = (uint32_t)(seed >> 32);
    g.epoch = epoch; g.ncols = ncols; g.picked = picked_out;
    RT_LAUNCH(dmb::k_ppo_gather, (rows + dmb::kGatherRows - 1) / dmb::kGatherRows, (rt_stream)hip_stream, g);
    return launch_status(0);
}

}  // extern "C"
