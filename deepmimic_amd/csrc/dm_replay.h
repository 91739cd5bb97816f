// The data side of AMP discriminator training on the device: the two random-storage replay buffers of the reference's AMPAgent (learning/amp_agent.py:70-77, 216-227,
// learning/replay_buffer_rand_storage.py) and the expert draws in front of k_amp_expert (amp_agent.py:244-249).  Included at the end of dm_host.cpp behind dm_ppo_batch.h,
// whose feistel_perm and gather_tile it uses; the device check, the launch status and the 16-byte rule are the runtime shim's (dm_host.cpp: valid_device, launch_status,
// rows_vec16).
//
// The store is stateless on the library side.  The caller owns buf [capacity, width] of 4-byte elements and state, an int64[2] = {size, total} on the device; {0, 0} is a
// cleared store.  No atomics, no workgroup waits on another one: every slot is a function of (state, seed, call, list position).
//
// dm_replay_append: n = min(*count, max_rows) rows of a list (idx[j], or j itself) go in.  With old = size and free = capacity - old, list row j gets the rank
//     q = j                                           when n <= capacity
//     q = perm(n, seed, call, kPassIncoming)(j)       otherwise: a rollout larger than the store keeps a uniformly chosen subset, not the earliest time steps
// and the slot
//     old + q                                         q < free                    (free slots first, in order: replay_buffer_rand_storage.py:63-66)
//     perm(old, seed, call, kPassVictim)(q - free)    free <= q < capacity        (distinct old rows: np.random.choice(curr_size, remainder, replace=False), :67-70)
//     none (slots_out = -1)                           q >= capacity               (the reference asserts n < buffer_size; here the case is defined)
// perm(count, seed, epoch, pass) is feistel_perm of dm_ppo_batch.h (include/dm_hip.h dm_ppo_gather) with epoch = call; the pass constants are
//     kPassVictim = 0x564943 ("VIC")        kPassIncoming = 0x494E43 ("INC").
// The slots of one call are distinct (q is a bijection of the list positions, the three ranges map one to one), so there is no write race.  packed_out[j] receives
// source row idx[j] for every j < n, dropped rows included: the dense rows the AMP observation normaliser records (amp_agent.py:287-292).  The new state --
// size = min(old + n, capacity), total += n -- is written by k_replay_commit, a one-thread launch BEHIND k_replay_append on the stream, so every workgroup of the copy
// reads the old state.
// Tile shape: one wavefront per workgroup, kAppendRows = 16 consecutive list rows per wavefront.  Lanes 0 .. 15 each settle one row's slot -- a walk runs only for a row
// with q >= free (victims) and, for the incoming shuffle, only when n > capacity -- then all 64 lanes copy the tile, kCopyUnroll independent loads in flight per lane before
// their stores, coalesced along a row on the store side and across the whole tile on the packed side: 16 bytes per lane where every base and 4 * width allow, dwords
// otherwise, as k_ppo_gather does.  Measured and dropped (docs/HISTORY.md section 18, both tiles' times): 4 rows per wavefront settled one at a time with every input pinned
// wave-uniform, so that the walks run on the scalar unit, and a row-by-row copy loop -- 1570 us for an iteration's two appends against 289 us with this tile.  Why was not
// traced; the reading is that a full store walks for every row, and a compute unit's one scalar unit then serialises what 64 lanes do side by side.
//
// dm_replay_sample: with size = state[0], destination row r reads slot mulhi32(w, size), w = word 0 of Philox4x32-10(counter = (r, call, kCtrSample, 0),
// key = (seed & 0xffffffff, seed >> 32)), kCtrSample = 0x534D50 ("SMP"): with replacement, as np.random.randint(0, curr_size, n) (replay_buffer_rand_storage.py:22-27).
// size == 0: dst is left untouched and picked_out gets -1.  One Philox evaluation per row and no walk, so the tile is k_ppo_gather's: kSampleRows rows per wavefront,
// lanes 0 .. kSampleRows - 1 draw, all 64 lanes copy the tile.
//
// k_amp_expert_draw: clip id and sample time of expert sample i exactly as dm_amp_expert / dm_amp_expert_clips draw them on the host with expert_calls == call.
#pragma once

namespace dmq {

constexpr int kAppendRows = 16;                  // list rows per wavefront of k_replay_append
constexpr unsigned kCopyUnroll = 8;              // loads a lane has in flight before their stores
constexpr int kSampleRows = 4;                   // destination rows per wavefront of k_replay_sample
constexpr uint32_t kPassVictim = 0x564943u, kPassIncoming = 0x494E43u, kCtrSample = 0x534D50u;

#ifdef DM_EMU
typedef dmb::Q4 Quad;                            // one 16-byte load / store
#else                                            // (not dmb::Q4 on the device: with the struct k_replay_append's unrolled copy allocates registers differently, ~1300 other lines)
typedef uint32_t Quad __attribute__((ext_vector_type(4)));
#endif

struct AppendArgs {
    uint32_t* buf; const uint32_t* src; uint32_t* packed; const int* idx; const int* count; const long long* state; int* slots;
    int capacity, width, max_rows, vec;          // vec: buf, src, packed (if given) and width * 4 are multiples of 16
    uint32_t seed_lo, seed_hi, call;
};

// the tile's n = rows * w elements (dwords, or 16-byte quads): element e is column e % w of tile row e / w, read from source row srow[.] and written to slot[.] of the
// store (if >= 0) and to element e of the packed tile (if given).  kCopyUnroll loads per lane are issued before the first store.
template <typename E> DMP_DEV void copy_tile(const E* src, E* buf, E* packed, const int* srow, const int* slot, unsigned w, unsigned n, unsigned l) {
    for (unsigned e0 = l; e0 < n; e0 += 64u * kCopyUnroll) {
        E v[kCopyUnroll]; unsigned r[kCopyUnroll], c[kCopyUnroll];
#pragma unroll
        for (unsigned u = 0; u < kCopyUnroll; ++u) {
            const unsigned e = e0 + 64u * u;
            const unsigned ec = e < n ? e : n - 1u;          // (a lane past the tile's end loads the last element again and stores nothing)
            r[u] = ec / w; c[u] = ec - r[u] * w; v[u] = src[(size_t)srow[r[u]] * w + c[u]];
        }
#pragma unroll
        for (unsigned u = 0; u < kCopyUnroll; ++u) {
            const unsigned e = e0 + 64u * u;
            if (e < n) {
                const int s = slot[r[u]];
                if (s >= 0) buf[(size_t)s * w + c[u]] = v[u];
                if (packed) packed[e] = v[u];
            }
        }
    }
}

__global__ void __launch_bounds__(64) k_replay_append(AppendArgs a) {
    __shared__ int srow[kAppendRows], slot[kAppendRows];
    const unsigned l = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * kAppendRows;
    int n = a.count ? *a.count : a.max_rows;
    n = n < 0 ? 0 : (n > a.max_rows ? a.max_rows : n);
    if (j0 >= n) return;                         // (the whole workgroup)
    const uint32_t cap = (uint32_t)a.capacity;
    long long size = a.state[0];
    const uint32_t old = size < 0 ? 0u : (size > (long long)cap ? cap : (uint32_t)size);      // (a state the caller did not corrupt is taken as it is)
    const uint32_t free_ = cap - old;
    const unsigned nr = (n - j0 < kAppendRows) ? (unsigned)(n - j0) : (unsigned)kAppendRows;
    if (l < nr) {
        const uint32_t j = (uint32_t)(j0 + l);
        uint32_t q = j;
        if ((uint32_t)n > cap) q = dmb::feistel_perm(j, (uint32_t)n, a.seed_lo, a.seed_hi, a.call, kPassIncoming);
        int s = -1;
        if (q < free_) s = (int)(old + q);
        else if (q < cap) s = (int)dmb::feistel_perm(q - free_, old, a.seed_lo, a.seed_hi, a.call, kPassVictim);
        srow[l] = a.idx ? a.idx[j] : (int)j;
        slot[l] = s;
        if (a.slots) a.slots[j] = s;
    }
    __syncthreads();
    if (a.vec) {
        const unsigned w4 = (unsigned)a.width / 4u;
        copy_tile<Quad>(reinterpret_cast<const Quad*>(a.src), reinterpret_cast<Quad*>(a.buf), a.packed ? reinterpret_cast<Quad*>(a.packed) + (size_t)j0 * w4 : nullptr,
                        srow, slot, w4, nr * w4, l);
    } else {
        const unsigned w = (unsigned)a.width;
        copy_tile<uint32_t>(a.src, a.buf, a.packed ? a.packed + (size_t)j0 * w : nullptr, srow, slot, w, nr * w, l);
    }
}

// behind k_replay_append on the stream: the state every workgroup of the copy has read is replaced
__global__ void __launch_bounds__(64) k_replay_commit(long long* state, const int* count, int max_rows, int capacity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int n = count ? *count : max_rows;
    n = n < 0 ? 0 : (n > max_rows ? max_rows : n);
    long long size = state[0];
    if (size > capacity) size = capacity;
    size += n;
    state[0] = size > capacity ? (long long)capacity : size;
    state[1] += n;
}

struct SampleArgs { const uint32_t* buf; const long long* state; uint32_t* dst; int* picked; int rows, width, vec; uint32_t seed_lo, seed_hi, call; };

__global__ void __launch_bounds__(64) k_replay_sample(SampleArgs g) {
    __shared__ int srow[kSampleRows];
    const int l = (int)threadIdx.x;
    const long long j0 = (long long)blockIdx.x * kSampleRows;
    const int nr = (g.rows - j0 < kSampleRows) ? (int)(g.rows - j0) : kSampleRows;      // rows of this tile (>= 1 by the grid size)
    const long long size = g.state[0];
    if (l < nr) {
        int s = -1;
        if (size > 0) {
            uint32_t f[4]; dmp::philox4x32_10((uint32_t)(j0 + l), g.call, kCtrSample, 0u, g.seed_lo, g.seed_hi, f);
            s = (int)(((uint64_t)f[0] * (uint64_t)(uint32_t)size) >> 32);
        }
        srow[l] = s;
        if (g.picked) g.picked[j0 + l] = s;
    }
    __syncthreads();
    if (size <= 0) return;
    if (g.vec) {                                  // 16 bytes per lane
        const unsigned w4 = (unsigned)g.width / 4u;
        dmb::gather_tile(reinterpret_cast<const dmb::Q4*>(g.buf), reinterpret_cast<dmb::Q4*>(g.dst) + (size_t)j0 * w4, srow, w4, (unsigned)nr * w4, (unsigned)l);
    } else {
        const unsigned w = (unsigned)g.width;
        dmb::gather_tile(g.buf, g.dst + (size_t)j0 * w, srow, w, (unsigned)nr * w, (unsigned)l);
    }
}

// expert sample i = blockIdx.x * 64 + lane: the draws of dm_amp_expert_clips (num_clips > 1) / dm_amp_expert (one clip) at expert_calls == call
__global__ void __launch_bounds__(64) k_amp_expert_draw(int n, uint64_t seed, uint64_t env_off, uint64_t call, int num_clips, const double* clip_cdf, const double* clip_dur,
                                                        double duration, int* clips, double* times, int* clips_out, double* times_out) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    int k = 0;
    double dur = duration;
    if (num_clips > 1) {
        const double u = dm_rand01(seed, env_off + 0x434C50ull, call, (uint64_t)i);
        while (k < num_clips - 1 && !(u < clip_cdf[k])) ++k;
        dur = clip_dur[k];
    }
    const double t = dur * dm_rand01(seed, env_off + 0x414D50ull, call, (uint64_t)i);
    clips[i] = k; times[i] = t;
    if (clips_out) clips_out[i] = k;
    if (times_out) times_out[i] = t;
}

}  // namespace dmq

extern "C" {

int dm_amp_expert_draw(dm_ctx* ctx, int n, uint64_t call, const double* ground_h_dev, float* out_dev, int32_t* clips_out_dev, double* times_out_dev) {
    if (!ctx) return fail("null ctx");
    CtxBase* c = ctx->c; DevGuard guard(c->device_id);
    if (!need_amp(c)) return -1;
    if (n < 1) return fail("dm_amp_expert_draw: n must be >= 1");
    if (!out_dev) return fail("dm_amp_expert_draw: out_dev is NULL");
    if (c->draw_cap < n) {                       // the ctx's scratch for the draws, grown on demand like d_ids: only a call that grows it allocates (and an allocation waits
        int cap = c->draw_cap > 0 ? c->draw_cap : 1024;      // for the device); the old block stays with the ctx until it is destroyed, a launch may still read it
        while (cap < n) { if (cap > 0x3fffffff) { cap = n; break; } cap *= 2; }
        double* t = (double*)c->dalloc(sizeof(double) * (size_t)cap); int* k = (int*)c->dalloc(sizeof(int) * (size_t)cap);
        if (!t || !k) return fail("device allocation failed");
        c->d_draw_times = t; c->d_draw_clips = k; c->draw_cap = cap;
    }
    const int nc = c->hm.num_clips;
    RT_LAUNCH(dmq::k_amp_expert_draw, (n + 63) / 64, c->stream, n, c->seed, (uint64_t)c->env_off, call, nc, c->d_clip_cdf, c->d_clip_dur, c->hm.duration, c->d_draw_clips,
              c->d_draw_times, clips_out_dev, times_out_dev);
    // the existing launch consumes them; a single-clip scene passes no clip list, as dm_amp_expert does
    return launch_status(c->amp_expert_clips(n, nc > 1 ? c->d_draw_clips : nullptr, c->d_draw_times, ground_h_dev, out_dev));
}

int dm_replay_append(int device_id, void* buf_dev, int capacity, int width, int64_t* state_dev, const void* src_dev, const int32_t* idx_dev, const int32_t* count_dev,
                     int max_rows, uint64_t seed, uint32_t call, void* packed_out, int32_t* slots_out, void* hip_stream) {
    if (!buf_dev || !state_dev || !src_dev) return fail("dm_replay_append: null argument (only idx, count, packed_out and slots_out may be NULL)");
    if (capacity < 1) return fail("dm_replay_append: capacity must be >= 1");
    if (width < 1) return fail("dm_replay_append: width must be >= 1");
    if (max_rows < 1) return fail("dm_replay_append: max_rows must be >= 1");
    if ((long long)capacity * width > 0x7fffffffLL) return fail("dm_replay_append: capacity * width exceeds 2^31 - 1 elements");
    if ((long long)max_rows * width > 0x7fffffffLL) return fail("dm_replay_append: max_rows * width exceeds 2^31 - 1 elements");
    if ((((uintptr_t)buf_dev | (uintptr_t)src_dev | (uintptr_t)packed_out | (uintptr_t)idx_dev | (uintptr_t)count_dev | (uintptr_t)slots_out) & 3) != 0)
        return fail("dm_replay_append: rows, lists and counts are arrays of 4-byte elements (misaligned pointer)");
    if (((uintptr_t)state_dev & 7) != 0) return fail("dm_replay_append: state must be 8-byte aligned");
    if (valid_device("dm_replay_append", device_id)) return -1;
    DevGuard guard(device_id);
    dmq::AppendArgs a;
    a.buf = (uint32_t*)buf_dev; a.src = (const uint32_t*)src_dev; a.packed = (uint32_t*)packed_out; a.idx = idx_dev; a.count = count_dev; a.state = (const long long*)state_dev;
    a.slots = slots_out; a.capacity = capacity; a.width = width; a.max_rows = max_rows;
    a.vec = rows_vec16(width, {buf_dev, src_dev, packed_out});
    a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32); a.call = call;
    rt_stream stream = (rt_stream)hip_stream;
    RT_LAUNCH(dmq::k_replay_append, (max_rows + dmq::kAppendRows - 1) / dmq::kAppendRows, stream, a);
    RT_LAUNCH(dmq::k_replay_commit, 1, stream, (long long*)state_dev, count_dev, max_rows, capacity);
    return launch_status(0);
}

int dm_replay_sample(int device_id, const void* buf_dev, int width, const int64_t* state_dev, int rows, uint64_t seed, uint32_t call, void* dst_dev, int32_t* picked_out,
                     void* hip_stream) {
    if (!buf_dev || !state_dev || !dst_dev) return fail("dm_replay_sample: null argument (only picked_out may be NULL)");
    if (width < 1) return fail("dm_replay_sample: width must be >= 1");
    if (rows < 1) return fail("dm_replay_sample: rows must be >= 1");
    if ((long long)rows * width > 0x7fffffffLL) return fail("dm_replay_sample: rows * width exceeds 2^31 - 1 elements");
    if ((((uintptr_t)buf_dev | (uintptr_t)dst_dev | (uintptr_t)picked_out) & 3) != 0) return fail("dm_replay_sample: rows are arrays of 4-byte elements (misaligned pointer)");
    if (((uintptr_t)state_dev & 7) != 0) return fail("dm_replay_sample: state must be 8-byte aligned");
    if (valid_device("dm_replay_sample", device_id)) return -1;
    DevGuard guard(device_id);
    dmq::SampleArgs g;
    g.buf = (const uint32_t*)buf_dev; g.state = (const long long*)state_dev; g.dst = (uint32_t*)dst_dev; g.picked = picked_out; g.rows = rows; g.width = width;
    g.vec = rows_vec16(width, {buf_dev, dst_dev});
    g.seed_lo = (uint32_t)(seed & 0xffffffffu); g.seed_hi = (uint32_t)(seed >> 32); g.call = call;
    RT_LAUNCH(dmq::k_replay_sample, (rows + dmq::kSampleRows - 1) / dmq::kSampleRows, (rt_stream)hip_stream, g);
    return launch_status(0);
}

}  // extern "C"
