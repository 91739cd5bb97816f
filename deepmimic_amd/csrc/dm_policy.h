// On-device policy inference: the actor of learning/pg_agent.py:141-188 / ppo_agent.py --
//   a = unnormalize_a( W3 relu(W2 relu(W1 normalize_s(s) + b1) + b2) + b3  [+ exp(logstd) * N(0,1)] )
// with the net of learning/nets/fc_2layers_1024units.py (1024, 512, ReLU) and the normalizers of learning/normalizer.py:95-102 --
// so that the 30 Hz loop (observation -> action -> 20 scene updates) never leaves the GPU.
//
// Unlike the rigid-body path this IS matrix-core work (batch 4096 x 227 x 1024 ...): three dense layers on
// v_mfma_f32_16x16x32_bf16, bf16 operands, fp32 accumulation.  One wavefront per workgroup owns a (16*MT) x (16*NT) output
// tile; A fragments come straight from the row-major activations (16 B per lane), B fragments from weights the host packed
// in fragment order ([n-tile][k-step][lane][8], one coalesced 1 KB read per fragment, L2-resident: 1.5 MB in all); bias,
// ReLU, the observation normaliser (layer 1) and the Gaussian head + action un-normaliser (layer 3) are fused into the
// prologue / epilogue.  Operand mapping: lane l carries row / column l & 15 and the 8 k-values 8 * (l >> 4) .. + 7 of the
// 32-wide k-step for both A and B (any consistent assignment sums the same products); C/D: column l & 15, rows
// 4 * (l >> 4) + reg (cdna_hip_programming.md, "Fragment layout").
#pragma once
#include <stdint.h>

namespace dmp {

struct PolicyDev {
    int S, H1, H2, A;                 // true layer widths
    int K1, N3;                       // padded: K1 = S rounded up to 64, N3 = A rounded up to 32
    const uint16_t *w1p, *w2p, *w3p;  // packed bf16 fragments
    const float *b1, *b2, *b3;        // biases (b3 padded to N3 with zeros)
    const float *s_mean, *s_inv_std;  // observation normaliser (learning/normalizer.py:95-98), S entries
    float s_clip;
    const float *a_mean, *a_std;      // action un-normaliser (:100-102), A entries
    const float *logstd;              // A entries (TFDistributionGaussianDiag, StdType.Default: a bias vector)
    const uint16_t* wfs;              // k_policy_fused: the fragments of layers 1 and 2 in the order each of its four waves consumes them (null: widths it is not compiled for)
};

struct GateDev;
// The scalar head of the device nets (include/dm_hip.h dm_scalar_head): a net with ONE output column -- the critic of learning/pg_agent.py:161-171, the AMP
// discriminator of learning/amp_agent.py:178-194 -- whose last step is not the Gaussian head but, per row, with y = acc + b3[0]:
//   HEAD_VALUE  v = min(max(y, lo), hi) (amp_agent.py:441-443; infinite bounds: PPO), then val_fail / val_succ where terminate is Fail (1) / Succ (2) (ppo_agent.py:262-264)
//   HEAD_STYLE  d = 1 - y, r = scale max(0, 1 - d^2 / 4), then (1 - lerp) r + lerp task_r with a task reward (amp_agent.py:294-297, 393-434)
// No noise is drawn, logstd / a_mean / a_std are not read, no logp is written.  row_mask (int32 per row, optional): a row whose flag is 0 gets `fill` in both outputs;
// a tile of rows whose flags are all 0 leaves before its first weight request.  raw (optional): y itself (the discriminator's logit statistics).
enum { HEAD_VALUE = 0, HEAD_STYLE = 1 };
struct ScalarHead {
    int kind;
    float lo, hi, val_fail, val_succ;
    float scale, lerp, fill;
    const int32_t* terminate;      // M or null
    const float* task_r;           // M or null
    const int32_t* row_mask;       // M or null
    float* raw;                    // M or null
};
struct PolicyIO {
    const float* states;   // M x S fp32 (RecordState of every env)
    uint16_t* s16;         // M x K1 bf16: normalised, clipped, zero-padded observations (written by k_policy_prep)
    uint16_t* h1;          // M x H1 bf16
    uint16_t* h2;          // M x H2 bf16
    float* actions;        // M x A fp32
    float* logp;           // M or null
    int M;
    int sample;            // 0: mode of the Gaussian (test / deterministic), 1: mean + std * noise
    uint32_t seed_lo, seed_hi; uint32_t step; int env_off;   // Philox4x32-10 key = (seed_lo + global env id, seed_hi), counter = (step * A + j, 0, 0, 0)
    // dm_policy_forward_ex: the last G of the S input columns come from their own [M x G] block (RecordGoal; the net's input is the concatenation
    // [norm_s, norm_g], learning/pg_agent.py:170-187), states is then M x (S - G); exp_rate < 1: a row takes the sampled action with that
    // probability and the mode otherwise (pg_agent.py:214-216 _decide_action: flip_coin(exp_params_curr.rate)), exp_flags[row] says which
    const float* goals; int G;
    float exp_rate; int32_t* exp_flags;
    unsigned long long* prof;   // measurement only (DM_POLICY_PROBE=2): per workgroup 8 timestamps (s_memtime of wave 0 at the phase boundaries)
    int probe;             // measurement only (DM_POLICY_PROBE): 1 = k_policy_fused re-reads block 0 of its weight stream forever (the stream served by the vector L1: what the L2 path costs)
    // gated actor (GateDev below), appended so that no member above moves: what k_policy_gate leaves for the GATED epilogues of layers 1 and 2, fp32 row-major
    const float *gsig0, *gbeta0;   // M x H1: sigma_0 = 2 sigmoid(.), beta_0
    const float *gsig1, *gbeta1;   // M x H2
    const GateDev* gate;           // device copy of the context's GateDev: k_policy_fused<.., true> reads the gate's first layers through it
};
// what a HEAD = 1 instantiation takes in PolicyIO's place (dm_policy_eval_scalar): the finished scalar goes to `actions` [M].  PolicyIO itself is what it was, so the
// kernel arguments of every other kernel lie where they lay.
struct ScalarIO : PolicyIO { ScalarHead sh; };
template <int HEAD> struct HeadIO { typedef PolicyIO type; };
template <> struct HeadIO<1> { typedef ScalarIO type; };

// The gate of learning/nets/fc_2layers_gated_1024units.py: a small net on the NORMALISED GOAL (the last G input columns, input_tfs[-1]) that scales and
// shifts the pre-activations of both hidden layers,
//   c = relu(Wc xg + bc)  (G -> GC);   e_i = relu(We_i c + be_i)  (GC -> GH);   beta_i = Wb_i e_i + bb_i,  sigma_i = 2 sigmoid(Ws_i e_i + bs_i)  (GH -> H_i)
//   h_i = relu(sigma_i * (W_i h_(i-1) + b_i) + beta_i)                                                     i = 0, 1  (layers 1 and 2)
// Rounding points (mirrored by deepmimic_amd/policy.py reference_forward(bf16=True)): xg, c, e_i are bf16 where they become MFMA operands (xg IS the goal block
// of the bf16 observations the main net reads); sigma, beta, acc + b and the gated pre-activation fmaf(sigma, acc + b, beta) stay fp32 (one rounding, written as
// fmaf so that device and emulator agree); h1, h2 are bf16 as in the plain actor, whose products, accumulation order and rounding points the main layers keep.
// Packed weights in the fragment order of k_policy_pack (PK_FRAG, below); KG = G rounded up to 32, GC and GH multiples of 32.
struct GateDev {
    int G, KG, GC, GH;
    const uint16_t *wcp, *wep[2], *wbp[2], *wsp[2];     // gate_common/0/dense; gate{i}/0/dense, gate{i}/dense (beta), gate{i}/dense_1 (sigma pre-activation)
    const float *bc, *be[2], *bb[2], *bs[2];
};

#ifdef DM_EMU
#define DMP_SCHED_FENCE() ((void)0)
#define DMP_DEV inline
struct bf16x8 { uint16_t v[8]; };
struct f32x4 { float v[4]; float& operator[](int i) { return v[i]; } float operator[](int i) const { return v[i]; } };
static inline float bf16_to_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
// lane-exchange emulation of the matrix-core instruction; every lane calls it from uniform control flow
static inline f32x4 mfma16(const bf16x8& a, const bf16x8& b, f32x4 c) {
    static uint16_t xa[4][64][8], xb[4][64][8];          // up to 4 wavefronts per workgroup (k_policy_gemm)
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = 0; i < 8; ++i) { xa[w][l][i] = a.v[i]; xb[w][l][i] = b.v[i]; }
    __syncthreads();
    const int col = l & 15, g = l >> 4;
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r; float acc = c[r];
        for (int g2 = 0; g2 < 4; ++g2) for (int i = 0; i < 8; ++i) acc += bf16_to_f32(xa[w][row + 16 * g2][i]) * bf16_to_f32(xb[w][col + 16 * g2][i]);
        c[r] = acc;
    }
    __syncthreads();
    return c;
}
static inline float lane_xor_f(float v, int mask) { static float x[256]; x[threadIdx.x] = v; __syncthreads(); const float r = x[threadIdx.x ^ mask]; __syncthreads(); return r; }   // (workgroups of up to four wavefronts)
#else
#define DMP_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define DMP_DEV __device__ __forceinline__
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
DMP_DEV f32x4 mfma16(const bf16x8& a, const bf16x8& b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
DMP_DEV float lane_xor_f(float v, int mask) { return __shfl_xor(v, mask, 64); }
#endif

// round to nearest even.  Never called on a NaN (some NaN payloads would carry into the sign bit): every caller passes the value through fminf / fmaxf
// first, which return their other operand -- a NaN observation becomes -s_clip (-inf without a clip), a NaN pre-activation 0; +-inf stays +-inf
DMP_DEV uint16_t f32_to_bf16(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
DMP_DEV void set8(bf16x8& f, int i, uint16_t h) {
#ifdef DM_EMU
    f.v[i] = h;
#else
    f[i] = (short)h;
#endif
}

// two floats -> two bf16 in one dword, round to nearest even: v_cvt_pk_bf16_f32 on gfx950 (one instruction instead of ten)
DMP_DEV uint32_t pack2_bf16(float a, float b) {
#ifdef DM_EMU
    return (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
#else
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
#endif
}
// four bf16 as ONE 8-byte store (dst is 8-byte aligned)
struct alignas(8) bf16x4_rec { uint32_t lo, hi; };
DMP_DEV void store4(uint16_t* dst, float a, float b, float c, float d) {
    bf16x4_rec v; v.lo = pack2_bf16(a, b); v.hi = pack2_bf16(c, d);
    *reinterpret_cast<bf16x4_rec*>(dst) = v;
}

// Philox4x32-10 (Salmon et al. 2011), the generator of deepmimic_amd/streams.py
DMP_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the exploration coin of a row: one uniform per (env, step), counter word 1 = 1 keeps it apart from the action noise of the same step
DMP_DEV float philox_coin(uint32_t env, uint32_t step, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t r[4]; philox4x32_10(step, 1, 0, 0, seed_lo + env, seed_hi, r);
    return ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
}
DMP_DEV float philox_normal(uint32_t env, uint32_t ctr, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t r[4]; philox4x32_10(ctr, 0, 0, 0, seed_lo + env, seed_hi, r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = ((float)(r[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// The scalar head's epilogue for one row < M (ScalarHead above).  Every multiply-add that may be contracted is an explicit fmaf and no other product feeds a sum, so
// device and emulator round at the same points: d (one rounding), d / 4 (exact), fmaf, the product with scale, 1 - lerp, its product with r, fmaf.  A NaN y gives
// lo (fmaxf returns its other operand) / a style reward of 0.  The three expressions are functions of their own: dm_amp_rewards.h evaluates the same ones over a stored rollout.
DMP_DEV float value_clip(float y, float lo, float hi) { return fminf(fmaxf(y, lo), hi); }
DMP_DEV float style_reward(float y, float scale) { const float d = 1.0f - y; return fmaxf(fmaf(-0.25f * d, d, 1.0f), 0.0f) * scale; }
DMP_DEV float style_blend(float lerp, float task_r, float s) { return fmaf(lerp, task_r, (1.0f - lerp) * s); }
DMP_DEV void scalar_head_store(const ScalarIO& io, int row, float y) {
    const ScalarHead& h = io.sh;
    float out = h.fill, raw = h.fill;
    if (!h.row_mask || h.row_mask[row] != 0) {
        raw = y;
        if (h.kind == HEAD_VALUE) {
            out = value_clip(y, h.lo, h.hi);
            if (h.terminate) { const int tm = h.terminate[row]; if (tm == 1) out = h.val_fail; else if (tm == 2) out = h.val_succ; }
        } else {
            out = style_reward(y, h.scale);
            if (h.task_r) out = style_blend(h.lerp, h.task_r[row], out);
        }
    }
    io.actions[row] = out;
    if (h.raw) h.raw[row] = raw;
}
// row_mask of the `rows` rows from row0 on: 0 if every flag is 0 (the addresses are uniform over the workgroup and clamped: scalar loads, one latency); fills the tile then
DMP_DEV bool scalar_head_tile_masked(const ScalarIO& io, int row0, int rows, int t) {
    if (!io.sh.row_mask) return false;
    int any = 0;
    for (int m = 0; m < rows; ++m) { const int row = row0 + m; any |= io.sh.row_mask[row < io.M ? row : io.M - 1]; }
    if (any) return false;
    if (t < rows && row0 + t < io.M) { io.actions[row0 + t] = io.sh.fill; if (io.sh.raw) io.sh.raw[row0 + t] = io.sh.fill; }
    return true;
}

// observation normaliser (learning/normalizer.py:95-98) fused with the bf16 conversion and the zero padding of K to a multiple of 32:
// one wavefront per row, coalesced reads and writes
__global__ void __launch_bounds__(64) k_policy_prep(PolicyDev p, PolicyIO io) {
    const int row = blockIdx.x, l = threadIdx.x;
    const int SS = p.S - io.G;                    // columns that come from the state block
    const float* srow = io.states + (size_t)row * SS;
    const float* grow = io.G ? io.goals + (size_t)row * io.G : nullptr;
    uint16_t* out = io.s16 + (size_t)row * p.K1;
    for (int k = l; k < p.K1; k += 64) {
        float x = 0.0f;
        if (k < p.S) { x = ((k < SS ? srow[k] : grow[k - SS]) - p.s_mean[k]) * p.s_inv_std[k]; x = fminf(fmaxf(x, -p.s_clip), p.s_clip); }
        out[k] = f32_to_bf16(x);
    }
}

// sigma = 2 sigmoid(z) in fp32.  EXACTLY 1 at z = 0 (expf(-0) = 1, 2 / 2), exactly 2 from z = +128 on (expf(-z) <= 2^-184 is 0 in fp32, and far below half
// an ulp of 1 from z = 17 on: 2 / 1) and exactly 0 from z = -128 down (expf(-z) >= 2^184 overflows to +inf, 2 / inf); any 2 / (1 + exp(-z)) on v_exp_f32 is.
DMP_DEV float gate_sigma(float z) { return 2.0f / (1.0f + expf(-z)); }

struct alignas(16) f32x4_rec { float x, y, z, w; };

// one 16-feature x 16-row tile of a gate layer, products transposed as in k_policy_fused (weight fragment = A operand, activations = B operand from LDS in
// [k-step][batch tile][lane] order): the lane holds features 16 ft + 4 (l >> 4) + r of batch row l & 15; k-steps ascending from a zero accumulator
DMP_DEV f32x4 gate_tile(const uint16_t* wp, int KS, int ft, const bf16x8* in, int bt, int l) {
    f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
    // the fragments of four k-steps are requested in one batch (one L2 latency per four, not per one: the gate's time is all latency)
    for (int k0 = 0; k0 < KS; k0 += 4) {
        bf16x8 f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = *reinterpret_cast<const bf16x8*>(wp + (((size_t)ft * KS + (k0 + u < KS ? k0 + u : KS - 1)) * 64 + l) * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) if (k0 + u < KS) acc = mfma16(f[u], in[((k0 + u) * 2 + bt) * 64 + l], acc);
    }
    return acc;
}
// bias + ReLU + bf16 of such a tile into the B-fragment order of the next gate layer (k = 16 ft + 4 g + r): 8 contiguous bytes per lane
DMP_DEV void gate_store(bf16x8* out, int ft, int bt, int c, int g, const f32x4& acc, const float* bias) {
    const int f0 = 16 * ft + 4 * g;
    store4(reinterpret_cast<uint16_t*>(out) + ((size_t)(((ft >> 1) * 2 + bt) * 64 + c + 16 * (2 * (ft & 1) + (g >> 1)))) * 8 + 4 * (g & 1),
           fmaxf(acc[0] + bias[f0], 0.0f), fmaxf(acc[1] + bias[f0 + 1], 0.0f), fmaxf(acc[2] + bias[f0 + 2], 0.0f), fmaxf(acc[3] + bias[f0 + 3], 0.0f));
}

// c (into sc) and e_0, e_1 (into se, 4 * 2 * 64 records each) of 32 rows from their goal block sx, all in B-fragment order [k-step][batch tile][lane]; called by
// every thread of a four-wave workgroup behind the barrier that completed sx, returns behind the barrier that completes se.  Shared by k_policy_gate and
// k_policy_fused<.., true>, so that both form the same c and e_i bit for bit.
DMP_DEV void gate_hidden(const GateDev& gd, const bf16x8* sx, bf16x8* sc, bf16x8* se, int w, int l, int c, int g) {
    for (int u = w; u < gd.GC / 8; u += 4) gate_store(sc, u >> 1, u & 1, c, g, gate_tile(gd.wcp, gd.KG / 32, u >> 1, sx, u & 1, l), gd.bc);
    __syncthreads();
    const int ne = gd.GH / 8;                             // units per e_i
    for (int u = w; u < 2 * ne; u += 4) { const int i = u / ne, v = u % ne; gate_store(se + i * 512, v >> 1, v & 1, c, g, gate_tile(gd.wep[i], gd.GC / 32, v >> 1, sc, v & 1, l), gd.be[i]); }
    __syncthreads();
}

// one gated 16-feature tile of k_policy_fused for one batch tile: sigma and beta from two k-steps each (GH = 64) with the gate-projection fragments as A and e_i
// as B, then relu(fmaf(sigma, acc + b, beta)) -> bf16 -> 8 bytes of the next layer's B fragment.  fbs / fbb: the lane's four scale / bias-projection biases, fp32
// bits carried in a 16-byte slot of the weight stream
DMP_DEV void gated_tile_store(uint16_t* dst, const bf16x8& fs0, const bf16x8& fs1, const bf16x8& fb0, const bf16x8& fb1, const bf16x8& fbs, const bf16x8& fbb,
                              const bf16x8& e0, const bf16x8& e1, const f32x4& acc, const float* mb) {
    f32x4 z;
#pragma unroll
    for (int r = 0; r < 4; ++r) z[r] = 0.0f;
    const f32x4 as = mfma16(fs1, e1, mfma16(fs0, e0, z)), ab = mfma16(fb1, e1, mfma16(fb0, e0, z));
    float bs[4], bb[4];
    __builtin_memcpy(bs, &fbs, 16); __builtin_memcpy(bb, &fbb, 16);
    store4(dst, fmaxf(fmaf(gate_sigma(as[0] + bs[0]), acc[0] + mb[0], ab[0] + bb[0]), 0.0f), fmaxf(fmaf(gate_sigma(as[1] + bs[1]), acc[1] + mb[1], ab[1] + bb[1]), 0.0f),
           fmaxf(fmaf(gate_sigma(as[2] + bs[2]), acc[2] + mb[2], ab[2] + bb[2]), 0.0f), fmaxf(fmaf(gate_sigma(as[3] + bs[3]), acc[3] + mb[3], ab[3] + bb[3]), 0.0f));
}

// The gate of the per-layer route: a workgroup of four wavefronts takes 32 batch rows from the goal block of the bf16 observations (k_policy_prep ran before:
// normalised, clipped, NaN already -s_clip) through c, e_0, e_1 in LDS to sigma_i / beta_i [M x H_i] fp32 in the scratch buffers of PolicyIO.  The units of
// work of a stage (feature tile x batch tile) are dealt round-robin to the waves; every count is a multiple of 4 (GC, GH multiples of 32, H_i of 64), so all
// waves make the same number of trips (the emulator's mfma16 is a workgroup-wide exchange).  Limits (checked at create): G <= 128, GC <= 256, GH <= 128.
__global__ void __launch_bounds__(256) k_policy_gate(PolicyDev p, PolicyIO io, GateDev gd) {
    constexpr int R = 32;
    __shared__ bf16x8 sx[4 * 2 * 64], sc[8 * 2 * 64], se[2][4 * 2 * 64];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, c = l & 15, g = l >> 4;
    const int row0 = (int)blockIdx.x * R;
    {
        uint16_t* const sxh = reinterpret_cast<uint16_t*>(sx);
        const int m = t & 31, row = row0 + m < io.M ? row0 + m : io.M - 1;
        const uint16_t* const src = io.s16 + (size_t)row * p.K1 + (p.S - gd.G);
        for (int k = t >> 5; k < gd.KG; k += 8)
            sxh[((size_t)((k >> 5) * 2 + (m >> 4)) * 64 + (m & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7)] = k < gd.G ? src[k] : (uint16_t)0;
    }
    __syncthreads();
    gate_hidden(gd, sx, sc, se[0], w, l, c, g);
    for (int i = 0; i < 2; ++i) {
        const int H = i ? p.H2 : p.H1;
        float* const sig = const_cast<float*>(i ? io.gsig1 : io.gsig0); float* const beta = const_cast<float*>(i ? io.gbeta1 : io.gbeta0);
        for (int u = w; u < H / 8; u += 4) {
            const int ft = u >> 1, bt = u & 1, f0 = 16 * ft + 4 * g, row = row0 + 16 * bt + c;
            const f32x4 ab = gate_tile(gd.wbp[i], gd.GH / 32, ft, se[i], bt, l), as = gate_tile(gd.wsp[i], gd.GH / 32, ft, se[i], bt, l);
            f32x4_rec vb, vs;
            vb.x = ab[0] + gd.bb[i][f0]; vb.y = ab[1] + gd.bb[i][f0 + 1]; vb.z = ab[2] + gd.bb[i][f0 + 2]; vb.w = ab[3] + gd.bb[i][f0 + 3];
            vs.x = gate_sigma(as[0] + gd.bs[i][f0]); vs.y = gate_sigma(as[1] + gd.bs[i][f0 + 1]); vs.z = gate_sigma(as[2] + gd.bs[i][f0 + 2]); vs.w = gate_sigma(as[3] + gd.bs[i][f0 + 3]);
            if (row < io.M) { *reinterpret_cast<f32x4_rec*>(beta + (size_t)row * H + f0) = vb; *reinterpret_cast<f32x4_rec*>(sig + (size_t)row * H + f0) = vs; }
        }
    }
}

// MODE 0: layer 1 (bf16 normalised observations; ReLU; bf16 out)             K = K1, N = H1
// MODE 1: layer 2 (bf16 in; ReLU; bf16 out)                                  K = H1, N = H2
// MODE 2: layer 3 (bf16 in; Gaussian head + un-normalise; fp32 actions)      K = H2, N = N3
// The k loop is software-pipelined by hand: the A / B fragments of step ks + 1 are requested before the MFMAs of step ks issue
// (two register sets), so one wave keeps its matrix core busy while the next 16-byte-per-lane reads are in flight.
// GATED (MODE 0 / 1): the epilogue reads sigma / beta of its elements from the scratch k_policy_gate filled: relu(fmaf(sigma, acc + b, beta)).
// HEAD = 1 (MODE 2, NT = 1): the scalar head (ScalarHead) -- column tile 0 only, no noise, no logp; a 16 MT-row tile that row_mask switches off leaves at once.
template <int MODE, int MT, int NT, bool GATED = false, int HEAD = 0>
__global__ void __launch_bounds__(64) k_policy_layer(PolicyDev p, typename HeadIO<HEAD>::type io) {
    const int l = threadIdx.x, c = l & 15, g = l >> 4;
    if constexpr (HEAD != 0) { if (scalar_head_tile_masked(io, (int)blockIdx.x * 16 * MT, 16 * MT, l)) return; }
    const int K = (MODE == 0) ? p.K1 : (MODE == 1 ? p.H1 : p.H2);
    const int N = (MODE == 0) ? p.H1 : (MODE == 1 ? p.H2 : p.N3);
    const int n_col_tiles = N / (16 * NT);
    // consecutive workgroups walk down the rows of one column block: they read the same weight fragments back to back
    const int row_blocks = (io.M + 16 * MT - 1) / (16 * MT);
    // MODE 2 (Gaussian head): one workgroup owns ALL N3 columns of its rows -- the log-probability is a sum over every action
    // component, so the column blocks are walked inside the workgroup (A = 36 / 58 need two blocks of 32) and logp is written once.
    const int cb_first = (MODE == 2) ? 0 : (int)blockIdx.x / row_blocks, rb = (MODE == 2) ? (int)blockIdx.x : (int)blockIdx.x % row_blocks;
    if (cb_first >= n_col_tiles || rb >= row_blocks) return;
    const int cb_last = (MODE == 2 && HEAD == 0) ? n_col_tiles : cb_first + 1;
    const int row0 = rb * 16 * MT, KS = K / 32;
    const uint16_t* wp = (MODE == 0) ? p.w1p : (MODE == 1 ? p.w2p : p.w3p);
    const uint16_t* ain = (MODE == 0) ? io.s16 : (MODE == 1 ? io.h1 : io.h2);
    float lps[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) lps[i][r] = 0.0f;

    for (int cb = cb_first; cb < cb_last; ++cb) {
    const int nt0 = cb * NT;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0f;

    const uint16_t* arow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) { const int row = row0 + 16 * i + c; arow[i] = ain + (size_t)(row < io.M ? row : 0) * K + 8 * g; }
    const uint16_t* bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = wp + ((size_t)(nt0 + j) * KS * 64 + l) * 8;

    bf16x8 a0[MT], b0[NT], a1[MT], b1[NT];
#define DMP_LOAD(A_, B_, ks_)                                                                                   \
    {                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) A_[i] = *reinterpret_cast<const bf16x8*>(arow[i] + (size_t)(ks_) * 32);      \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) B_[j] = *reinterpret_cast<const bf16x8*>(bcol[j] + (size_t)(ks_) * 512);     \
    }
#define DMP_MMA(A_, B_)                                                                                         \
    {                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                          \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[i][j] = mfma16(A_[i], B_[j], acc[i][j]);         \
    }
    if (MODE == 2) {
        // the head is tiny (N3 = 32): its time is all load latency, so the fragments of 8 k-steps are requested in one batch
        for (int kb = 0; kb < KS; kb += 8) {
            bf16x8 aa[8][MT], bb[8][NT];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (kb + u < KS) DMP_LOAD(aa[u], bb[u], kb + u)
#pragma unroll
            for (int u = 0; u < 8; ++u) if (kb + u < KS) DMP_MMA(aa[u], bb[u])
        }
    } else {
        DMP_LOAD(a0, b0, 0)
        for (int ks = 0; ks < KS; ks += 2) {          // KS is even: K1 is padded to 64, H1 and H2 are multiples of 64
            DMP_LOAD(a1, b1, ks + 1)
            DMP_MMA(a0, b0)
            if (ks + 2 < KS) DMP_LOAD(a0, b0, ks + 2)
            DMP_MMA(a1, b1)
        }
    }
#undef DMP_LOAD
#undef DMP_MMA

    if (MODE != 2) {
        const float* bias = (MODE == 0) ? p.b1 : p.b2;
        uint16_t* out = (MODE == 0) ? io.h1 : io.h2;
        const float* const gsig = (MODE == 0) ? io.gsig0 : io.gsig1; const float* const gbeta = (MODE == 0) ? io.gbeta0 : io.gbeta1;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = (nt0 + j) * 16 + c; const float bc = bias[col];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + 16 * i + 4 * g + r;
                    if (GATED) { if (row < io.M) out[(size_t)row * N + col] = f32_to_bf16(fmaxf(fmaf(gsig[(size_t)row * N + col], acc[i][j][r] + bc, gbeta[(size_t)row * N + col]), 0.0f)); }
                    else if (row < io.M) out[(size_t)row * N + col] = f32_to_bf16(fmaxf(acc[i][j][r] + bc, 0.0f));
                }
        }
    } else if constexpr (HEAD != 0) {
        // scalar head: column 0 of the tile is on the lanes c = 0, rows 4 g + r
        const float b30 = p.b3[0];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 16 * i + 4 * g + r;
                if (c == 0 && row < io.M) scalar_head_store(io, row, acc[i][0][r] + b30);
            }
    } else {
        // Gaussian head: norm_a = mean + exp(logstd) z, a = norm_a * a_std + a_mean, logp = sum_j (-z^2/2 - logstd_j) - A/2 log 2 pi
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 16 * i + 4 * g + r;
                float lp = 0.0f;
                bool explore = io.sample && row < io.M;
                if (explore && io.exp_rate < 1.0f) explore = philox_coin((uint32_t)(io.env_off + row), io.step, io.seed_lo, io.seed_hi) < io.exp_rate;
                if (io.exp_flags && c == 0 && nt0 == 0 && row < io.M) io.exp_flags[row] = explore ? 1 : 0;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = (nt0 + j) * 16 + c;
                    if (col < p.A) {
                        const float ls = p.logstd[col];
                        float z = 0.0f;
                        if (explore) z = philox_normal((uint32_t)(io.env_off + row), io.step * (uint32_t)p.A + (uint32_t)col, io.seed_lo, io.seed_hi);
                        const float na = acc[i][j][r] + p.b3[col] + expf(ls) * z;
                        if (row < io.M) io.actions[(size_t)row * p.A + col] = na * p.a_std[col] + p.a_mean[col];
                        lp += -0.5f * z * z - ls;
                    }
                }
                lps[i][r] += lp;
            }
    }
    }   // column blocks

    if (MODE == 2 && HEAD == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 16 * i + 4 * g + r;
                // the 16 lanes of a group hold 16 columns of one row (per column block); sum them, then the constant once
                float lp = lps[i][r];
                lp += lane_xor_f(lp, 1); lp += lane_xor_f(lp, 2); lp += lane_xor_f(lp, 4); lp += lane_xor_f(lp, 8);
                if (io.logp && c == 0 && row < io.M) io.logp[row] = lp - 0.5f * (float)p.A * 1.8378770664093453f;
            }
    }
}

// Layers 1 and 2 as an LDS-tiled GEMM: one workgroup of four wavefronts owns a 128 x 128 output tile (each wave 64 x 64 = 4 x 4 MFMA
// tiles, 16 v_mfma_f32_16x16x32_bf16 per k-step).  Per k-step the workgroup stages the 128 x 32 block of A and the 32 x 128 block of B
// (8 KB each, already in fragment order: [fragment][lane][8 bf16]) in LDS, double-buffered, every thread moving two 16-byte chunks of
// each; a wave then reads its 4 + 4 fragments back with conflict-free ds_read_b128 (lane-major 16-B records).  Against the one-wave
// kernel above that is 2 KB instead of 6 KB of L2 traffic per 8 MFMAs: the layer is no longer bound by the L2 -> CU path.
// MODE 0: layer 1 (A = normalised observations, K = K1, N = H1), MODE 1: layer 2 (A = h1, K = H1, N = H2).  N must be a multiple of 128.
// BM = 64 halves the tile height (each wave 32 x 64) for batches too small to fill the chip with 128 x 128 tiles.
// (Folding k_policy_prep into MODE 0 -- fp32 observations normalised on the way from the register stage to LDS -- was measured slower:
// 44.9 / 98.8 us against 41.2 / 83.4 us at 4096 / 16384 rows; eight scalar loads per chunk cost more than the 4 us kernel they replace.)
// GATED: as in k_policy_layer.
template <int MODE, int BM, bool GATED = false>
__global__ void __launch_bounds__(256) k_policy_gemm(PolicyDev p, PolicyIO io) {
    constexpr int BN = 128, MT = BM / 32, AF = BM / 16;      // MT: row fragments per wave, AF: row fragments per workgroup
    __shared__ bf16x8 sA[2][AF][64];
    __shared__ bf16x8 sB[2][8][64];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, c = l & 15, g = l >> 4, wr = w >> 1, wc = w & 1;
    const int K = (MODE == 0) ? p.K1 : p.H1, N = (MODE == 0) ? p.H1 : p.H2, KS = K / 32;
    const int row_blocks = (io.M + BM - 1) / BM;
    // consecutive workgroups walk down the rows of one column block: they read the same weight fragments back to back
    const int cb = (int)blockIdx.x / row_blocks, rb = (int)blockIdx.x % row_blocks;
    if (cb >= N / BN) return;
    const int row0 = rb * BM, nt0 = cb * (BN / 16);
    const uint16_t* wp = (MODE == 0) ? p.w1p : p.w2p;
    const uint16_t* ain = (MODE == 0) ? io.s16 : io.h1;
    // staging: this thread moves fragments w and w + 4 (lane l) of both operands
    constexpr int AU = AF / 4;                               // A chunks per thread (2 for BM = 128, 1 for BM = 64)
    const uint16_t* ag[AU]; const uint16_t* bg[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int f = w + 4 * u, row = row0 + 16 * f + c;
        if (u < AU) ag[u < AU ? u : 0] = ain + (size_t)(row < io.M ? row : 0) * K + 8 * g;
        bg[u] = wp + ((size_t)(nt0 + f) * KS * 64 + l) * 8;
    }
    // two register stages: the chunks of k-step ks + 3 are requested while k-step ks is multiplied and reach LDS two iterations later,
    // so a request has two full iterations (MFMAs + barrier) to come back -- with one workgroup per CU nothing else hides the L2 latency
    bf16x8 ra[2][AU], rbv[2][2];
#define DMP_GLOAD(st_, ks_)                                                                                \
    { _Pragma("unroll") for (int u = 0; u < 2; ++u) { if (u < AU) ra[st_][u < AU ? u : 0] = *reinterpret_cast<const bf16x8*>(ag[u < AU ? u : 0] + (size_t)(ks_) * 32); \
                                                       rbv[st_][u] = *reinterpret_cast<const bf16x8*>(bg[u] + (size_t)(ks_) * 512); } }
#define DMP_LSTORE(buf_, st_)                                                                              \
    { _Pragma("unroll") for (int u = 0; u < 2; ++u) { if (u < AU) sA[buf_][w + 4 * u][l] = ra[st_][u < AU ? u : 0]; sB[buf_][w + 4 * u][l] = rbv[st_][u]; } }
    f32x4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0f;
    DMP_GLOAD(0, 0)
    DMP_LSTORE(0, 0)
    DMP_GLOAD(1, 1)                    // KS >= 2 (K is a multiple of 64)
    if (2 < KS) DMP_GLOAD(0, 2)
    __syncthreads();
#define DMP_ITER(ks, par)                                                                                  \
    {                                                                                                      \
        /* k-step ks + 1 (stage par ^ 1, requested two iterations ago) goes to the other buffer, its registers take k-step ks + 3 */ \
        if ((ks) + 1 < KS) DMP_LSTORE((par) ^ 1, (par) ^ 1)                                                \
        if ((ks) + 3 < KS) DMP_GLOAD((par) ^ 1, (ks) + 3)                                                  \
        DMP_MULT(par)                                                                                      \
        __syncthreads();                                                                                   \
    }
#define DMP_MULT(buf)                                                                                      \
    {                                                                                                      \
        bf16x8 a[MT], b[4];                                                                                \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { if (i < MT) a[i < MT ? i : 0] = sA[buf][MT * wr + i][l]; b[i] = sB[buf][4 * wc + i][l]; } \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);       \
    }
    for (int ks = 0; ks < KS; ks += 2) { DMP_ITER(ks, 0) DMP_ITER(ks + 1, 1) }
#undef DMP_ITER
#undef DMP_MULT
#undef DMP_GLOAD
#undef DMP_LSTORE
    const float* bias = (MODE == 0) ? p.b1 : p.b2;
    uint16_t* out = (MODE == 0) ? io.h1 : io.h2;
    const float* const gsig = (MODE == 0) ? io.gsig0 : io.gsig1; const float* const gbeta = (MODE == 0) ? io.gbeta0 : io.gbeta1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = (nt0 + 4 * wc + j) * 16 + c; const float bc = bias[col];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 16 * MT * wr + 16 * i + 4 * g + r;
                if (GATED) { if (row < io.M) out[(size_t)row * N + col] = f32_to_bf16(fmaxf(fmaf(gsig[(size_t)row * N + col], acc[i][j][r] + bc, gbeta[(size_t)row * N + col]), 0.0f)); }
                else if (row < io.M) out[(size_t)row * N + col] = f32_to_bf16(fmaxf(acc[i][j][r] + bc, 0.0f));
            }
    }
}


// ---- One launch for the whole actor (round 5) ---------------------------------------------------------------------------------------------
// A workgroup of four wavefronts takes a tile of 32 batch rows through prep + the three layers; an MLP is row-independent, so nothing is
// synchronised beyond the workgroup.  The products are computed TRANSPOSED, out^T = W^T x in^T: the weight fragment is the A operand (16
// output features x 32 k), the activations the B operand (32 k x 16 batch rows), so a lane of the result holds FOUR CONSECUTIVE FEATURES of
// one batch row (rows 4 (l >> 4) + r of the C tile) -- after bias + ReLU + bf16 they are 8 contiguous bytes of the next layer's B fragment:
// one ds_write_b64 per tile, no transposition.  (The host's fragment packing serves both roles: lane <-> (feature l & 15, k 8 (l >> 4) + i).)
//
// Layer 1 is produced in four chunks of 256 features (each wave 64); behind every chunk all waves add its contribution to their 128 layer-2
// outputs (64 accumulator VGPRs per wave, alive across the chunks).  LDS then holds the observations (KS1 x 2 KB), TWO chunk buffers
// (2 x 16 KB: one barrier per chunk) and, overlaid on the first two once they are dead, h2 (32 KB): 48 KB at K1 = 256, so the kernel fits
// beside resident waves of the step kernel of another env group (20 KB of LDS each).
//
// What bounds it: every workgroup streams ALL 1.5 MB of weights through its CU's 64 B / clk path from L2 (~ 10 us at 2.4 GHz; 128 workgroups
// at 4096 rows = 19 TB/s across the eight L2s).  The stream is laid out by the host in consumption order per wave -- blocks of 8 fragments
// (8 KB): layer-1 blocks = 2 k-steps x the wave's 4 feature tiles, layer-2 blocks = 1 k-step x its 8 feature tiles -- and walked with a
// three-deep register ring (block t + 2 is requested before block t is multiplied), the whole schedule unrolled at compile time so that the
// ring slots are plain registers.  KS1 = K1 / 32 (8: humanoid, 12: dog3d); H1 = 1024, H2 = 512 (learning/nets/fc_2layers_1024units.py);
// other widths take the per-layer kernels above.
//
// GATED (dm_policy_create_gated, GC <= 256, GH = 64): behind the observations a prologue takes the tile's goal rows through c, e_0, e_1 (gate_hidden; sx and sc live in the
// chunk buffers, which are still empty, e_0 / e_1 in 8 KB of their own).  The gate projections ride the weight stream: behind the layer-1 blocks of every chunk 3 blocks =
// 4 feature tiles x {sigma k-steps 0 1, beta k-steps 0 1, scale biases, bias-projection biases}, behind the last chunk 6 blocks for the 8 layer-2 tiles; a tile's sigma and
// beta are formed in the epilogue that already holds its accumulators (gated_tile_store), 8 MFMAs per feature tile.  Block t + 2 is still requested when block t is entered,
// and a block is entered once the block before it is used up (a tile's six slots may straddle two blocks).  The plain instantiations are untouched by the switch.
//
// HEAD = 1 (dm_policy_eval_scalar, action_dim = 1): the scalar head (ScalarHead) in place of the Gaussian one.  A tile that row_mask switches off leaves before the first
// weight request; no Philox draw; layer 3 is ONE 16-column tile (N3T = 1) on the two waves that own it (waves 2 and 3 are done behind the barrier that completes h2), its column 0
// goes through scalar_head_store.  Layers 1 and 2, the stream and the ring are the code above, so y is bit for bit the mode action of an actor with A = 1.  HEAD = 0 is
// untouched by the switch.
template <int KS1, int N3T, bool GATED = false, int HEAD = 0>
__global__ void __launch_bounds__(256, 2) k_policy_fused(PolicyDev p, typename HeadIO<HEAD>::type io) {
    static_assert(HEAD == 0 || N3T == 1, "the scalar head multiplies one column tile of layer 3");
    constexpr int NGB1 = GATED ? 3 : 0, NGB2 = GATED ? 6 : 0;
    constexpr int R = 32, NQ = 4, NB1 = KS1 / 2, NB2 = 8, NBQ = NB1 + NGB1 + NB2, NBLK = NQ * NBQ + NGB2;
    constexpr int LDS_S16 = KS1 * 2 * 64, LDS_H1C = 8 * 2 * 64, LDS_H2 = 16 * 2 * 64;            // in 16-byte records
    constexpr int LDS_TOTAL = (LDS_S16 + 2 * LDS_H1C > LDS_H2) ? LDS_S16 + 2 * LDS_H1C : LDS_H2;
    __shared__ bf16x8 lds[LDS_TOTAL];
    __shared__ float lp_part[4][16];
    __shared__ float sbias[1024 + 512];              // b1 | b2: a global read in an epilogue would have to drain the weight requests in flight behind it (vmcnt is in order)
    bf16x8* const s16 = lds;                         // [ks][bt][lane]
    bf16x8* const h1c = lds + LDS_S16;               // [2][ksl][bt][lane]
    bf16x8* const h2 = lds;                          // [ks][bt][lane]: overlays s16 and h1c[0] (dead from the barrier of the last chunk on)
    const int t = threadIdx.x, w = t >> 6, l = t & 63, c = l & 15, g = l >> 4;
    const int row0 = (int)blockIdx.x * R;
#ifndef DM_EMU
#define DMF_STAMP(i_) { if (io.prof && t == 0) io.prof[(size_t)blockIdx.x * 8 + (i_)] = __builtin_amdgcn_s_memtime(); }
#else
#define DMF_STAMP(i_) {}
#endif
    DMF_STAMP(0)
    if constexpr (HEAD != 0) { if (scalar_head_tile_masked(io, row0, R, t)) return; }
    const uint16_t* const ws = p.wfs + ((size_t)w * NBLK * 8 * 64 + l) * 8;      // this wave's stream; fragment f of block b at ws + (b * 8 + f) * 512
    bf16x8 ring[3][8];
#define DMF_LOAD(slot_, blk_)                                                                                              \
    { DMP_SCHED_FENCE(); _Pragma("unroll") for (int f = 0; f < 8; ++f) ring[slot_][f] = *reinterpret_cast<const bf16x8*>(ws + ((size_t)(io.probe == 1 ? 0 : ((blk_) < NBLK ? (blk_) : NBLK - 1)) * 8 + f) * 512); DMP_SCHED_FENCE(); }   \
    /* (fenced: left alone, the machine scheduler sinks every request to just in front of its MFMA to save registers, and the stream runs at one L2 latency per fragment) */
    DMF_LOAD(0, 0)                                   // the first two blocks are requested before anything else: they fly while the observations are prepared
    DMF_LOAD(1, 1)
    // ---- prep: normalise, clip, bf16, into B-fragment order (learning/normalizer.py:95-98).  A thread owns input column t (and t + 256): consecutive lanes read
    // consecutive floats of a row, mean and 1 / std are read once per thread, and all row reads are independent and requested up front (one latency, not 32)
    constexpr int NCOL = (KS1 * 32 + 255) / 256;
    float px[NCOL][R], pmean[NCOL], pinv[NCOL];
    {
#pragma unroll
        for (int i = 0; i < 6; ++i) { const int k = t + 256 * i; sbias[k] = (k < 1024) ? p.b1[k] : p.b2[k - 1024]; }
        const int SS = p.S - io.G;
#pragma unroll
        for (int kk = 0; kk < NCOL; ++kk) {
            const int k = t + 256 * kk, kc = k < p.S ? k : p.S - 1;
            pmean[kk] = p.s_mean[kc]; pinv[kk] = p.s_inv_std[kc];
            const bool from_goal = kc >= SS;
            const float* const base = from_goal ? io.goals + (kc - SS) : io.states + kc;
            const size_t stride = from_goal ? (size_t)io.G : (size_t)SS;
#pragma unroll
            for (int m = 0; m < R; ++m) { int row = row0 + m; if (row >= io.M) row = io.M - 1; px[kk][m] = base[(size_t)row * stride]; }
        }
        DMP_SCHED_FENCE();
    }
    // the head's noise does not depend on the net: drawn now, while the weight and observation requests are in flight (4 Philox + Box-Muller per owned action tile and lane)
    constexpr int NT3W = (N3T + 1) / 2;
    float hz[NT3W][4]; bool explore;
    if constexpr (HEAD == 0) {
        const int row = row0 + 16 * (w & 1) + c;
        explore = io.sample && row < io.M;
        if (explore && io.exp_rate < 1.0f) explore = philox_coin((uint32_t)(io.env_off + row), io.step, io.seed_lo, io.seed_hi) < io.exp_rate;
#pragma unroll
        for (int it = 0; it < NT3W; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 16 * ((w >> 1) + 2 * it) + 4 * g + r;
                hz[it][r] = (explore && col < p.A) ? philox_normal((uint32_t)(io.env_off + row), io.step * (uint32_t)p.A + (uint32_t)col, io.seed_lo, io.seed_hi) : 0.0f;
            }
    }

    {
        uint16_t* const s16h = reinterpret_cast<uint16_t*>(s16);
#pragma unroll
        for (int kk = 0; kk < NCOL; ++kk) {
            const int k = t + 256 * kk;
            if (k < KS1 * 32) {
                const int rec0 = (k >> 5) * 128 + 16 * ((k & 31) >> 3), e = k & 7;          // record of batch row m: rec0 + 64 (m >> 4) + (m & 15)
#pragma unroll
                for (int m = 0; m < R; ++m) {
                    float v = fminf(fmaxf((px[kk][m] - pmean[kk]) * pinv[kk], -p.s_clip), p.s_clip);
                    if (k >= p.S) v = 0.0f;
                    s16h[(size_t)(rec0 + 64 * (m >> 4) + (m & 15)) * 8 + e] = f32_to_bf16(v);
                }
            }
        }
    }
    __syncthreads();
    bf16x8* se = nullptr;
    if constexpr (GATED) {
        __shared__ bf16x8 se_buf[2 * 4 * 2 * 64];
        se = se_buf;
        const GateDev gd = *io.gate;
        bf16x8* const sx = h1c + LDS_H1C;          // goal block re-based to k = 0 (<= 512 records); c goes to h1c[0] (<= 1024 records)
        {
            const uint16_t* const s16h = reinterpret_cast<const uint16_t*>(s16); uint16_t* const sxh = reinterpret_cast<uint16_t*>(sx);
            const int m = t & 31;
            for (int k = t >> 5; k < gd.KG; k += 8) {
                const int kc = p.S - gd.G + k;
                sxh[((size_t)((k >> 5) * 2 + (m >> 4)) * 64 + (m & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7)] =
                    k < gd.G ? s16h[((size_t)((kc >> 5) * 2 + (m >> 4)) * 64 + (m & 15) + 16 * ((kc & 31) >> 3)) * 8 + (kc & 7)] : (uint16_t)0;
            }
        }
        __syncthreads();
        gate_hidden(gd, sx, h1c, se, w, l, c, g);
    }
#define DMF_GF(X_, i_) ring[((X_) + (i_) / 8) % 3][(i_) % 8]
    /* gated tile tl_ (six slots from 6 tl_ on behind block X_) for both batch tiles; before it the blocks whose predecessor is used up are entered */
#define DMF_GATED_TILE(X_, tl_, E_, ACC_, MB_, DST0_, DST1_)                                                                                          \
    {                                                                                                                                                 \
        if ((tl_) % 4 == 0) DMF_LOAD(((X_) + 3 * ((tl_) / 4) + 2) % 3, (X_) + 3 * ((tl_) / 4) + 2)                                                    \
        if ((tl_) % 4 == 2) DMF_LOAD(((X_) + 3 * ((tl_) / 4) + 3) % 3, (X_) + 3 * ((tl_) / 4) + 3)                                                    \
        if ((tl_) % 4 == 3) DMF_LOAD(((X_) + 3 * ((tl_) / 4) + 4) % 3, (X_) + 3 * ((tl_) / 4) + 4)                                                    \
        gated_tile_store(DST0_, DMF_GF(X_, 6 * (tl_)), DMF_GF(X_, 6 * (tl_) + 1), DMF_GF(X_, 6 * (tl_) + 2), DMF_GF(X_, 6 * (tl_) + 3), DMF_GF(X_, 6 * (tl_) + 4),   \
                         DMF_GF(X_, 6 * (tl_) + 5), (E_)[(0 * 2 + 0) * 64 + l], (E_)[(1 * 2 + 0) * 64 + l], ACC_[0], MB_);                            \
        gated_tile_store(DST1_, DMF_GF(X_, 6 * (tl_)), DMF_GF(X_, 6 * (tl_) + 1), DMF_GF(X_, 6 * (tl_) + 2), DMF_GF(X_, 6 * (tl_) + 3), DMF_GF(X_, 6 * (tl_) + 4),   \
                         DMF_GF(X_, 6 * (tl_) + 5), (E_)[(0 * 2 + 1) * 64 + l], (E_)[(1 * 2 + 1) * 64 + l], ACC_[1], MB_);                            \
    }

    DMF_STAMP(1)
    f32x4 acc2[8][2];
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc2[n][b][r] = 0.0f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        f32x4 acc1[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc1[j][b][r] = 0.0f;
        // layer 1, features [256 q + 64 w, + 64): NB1 blocks of 2 k-steps x 4 feature tiles
#pragma unroll
        for (int b1 = 0; b1 < NB1; ++b1) {
            const int blk = q * NBQ + b1;
            DMF_LOAD((blk + 2) % 3, blk + 2)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int ks = 2 * b1 + kk;
                const bf16x8 x0 = s16[(ks * 2 + 0) * 64 + l], x1 = s16[(ks * 2 + 1) * 64 + l];
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc1[j][0] = mfma16(ring[blk % 3][kk * 4 + j], x0, acc1[j][0]); acc1[j][1] = mfma16(ring[blk % 3][kk * 4 + j], x1, acc1[j][1]); }
            }
        }
        // bias + ReLU + bf16 -> this chunk's buffer, already in the B-fragment order of layer 2 (local k = 64 w + 16 j + 4 g + r)
        if constexpr (GATED) {
            uint16_t* const dst = reinterpret_cast<uint16_t*>(h1c + (q & 1) * LDS_H1C);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f0 = 256 * q + 64 * w + 16 * j + 4 * g;
                const int ksl = 2 * w + (j >> 1), ll = c + 16 * (2 * (j & 1) + (g >> 1));
                DMF_GATED_TILE(q * NBQ + NB1, j, se, acc1[j], sbias + f0, dst + ((size_t)((ksl * 2 + 0) * 64 + ll)) * 8 + 4 * (g & 1), dst + ((size_t)((ksl * 2 + 1) * 64 + ll)) * 8 + 4 * (g & 1))
            }
        } else {
            uint16_t* const dst = reinterpret_cast<uint16_t*>(h1c + (q & 1) * LDS_H1C);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f0 = 256 * q + 64 * w + 16 * j + 4 * g;
                const int ksl = 2 * w + (j >> 1), ll = c + 16 * (2 * (j & 1) + (g >> 1));
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    store4(dst + ((size_t)((ksl * 2 + b) * 64 + ll)) * 8 + 4 * (g & 1), fmaxf(acc1[j][b][0] + sbias[f0], 0.0f), fmaxf(acc1[j][b][1] + sbias[f0 + 1], 0.0f),
                           fmaxf(acc1[j][b][2] + sbias[f0 + 2], 0.0f), fmaxf(acc1[j][b][3] + sbias[f0 + 3], 0.0f));
                }
            }
        }
        __syncthreads();
        if (q == 0) DMF_STAMP(2)
        // layer 2, outputs [128 w, + 128), k in [256 q, + 256): NB2 blocks of 1 k-step x 8 feature tiles
        {
            const bf16x8* const src = h1c + (q & 1) * LDS_H1C;
#pragma unroll
            for (int ksl = 0; ksl < NB2; ++ksl) {
                const int blk = q * NBQ + NB1 + NGB1 + ksl;
                DMF_LOAD((blk + 2) % 3, blk + 2)
                const bf16x8 x0 = src[(ksl * 2 + 0) * 64 + l], x1 = src[(ksl * 2 + 1) * 64 + l];
#pragma unroll
                for (int n = 0; n < 8; ++n) { acc2[n][0] = mfma16(ring[blk % 3][n], x0, acc2[n][0]); acc2[n][1] = mfma16(ring[blk % 3][n], x1, acc2[n][1]); }
            }
        }
    }
    DMF_STAMP(3)
    constexpr int KS3 = 16;
    bf16x8 wf[KS3];
    float hc_ls[NT3W][4], hc_b3[NT3W][4], hc_as[NT3W][4], hc_am[NT3W][4];
    if constexpr (GATED) {
        // layer-2 epilogue, gated: the ring is still at work (6 blocks of gate projections), so layer 3's first fragments are requested behind it
        uint16_t* const dst = reinterpret_cast<uint16_t*>(h2);
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int f0 = 128 * w + 16 * n + 4 * g;
            const int ks = 4 * w + (n >> 1), ll = c + 16 * (2 * (n & 1) + (g >> 1));
            DMF_GATED_TILE(NQ * NBQ, n, se + 512, acc2[n], sbias + 1024 + f0, dst + ((size_t)((ks * 2 + 0) * 64 + ll)) * 8 + 4 * (g & 1), dst + ((size_t)((ks * 2 + 1) * 64 + ll)) * 8 + 4 * (g & 1))
        }
    }
#undef DMF_GATED_TILE
#undef DMF_GF
#undef DMF_LOAD
    // the first action tile's 16 weight fragments of layer 3 are requested now (the ring is dead): they arrive during the epilogue and the barrier
    float hb3 = 0.0f;
    if constexpr (HEAD != 0) {
        // scalar head: tile 0 only, for the two waves that multiply it; of the constants b3[0] alone (a scalar load: not behind the vector requests)
        if (w < 2) {
            DMP_SCHED_FENCE();
#pragma unroll
            for (int ks = 0; ks < KS3; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(p.w3p + ((size_t)ks * 64 + l) * 8);
            DMP_SCHED_FENCE();
        }
        hb3 = p.b3[0];
    } else {
        const int ntc0 = (w >> 1) < N3T ? (w >> 1) : N3T - 1;
        DMP_SCHED_FENCE();
#pragma unroll
        for (int ks = 0; ks < KS3; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(p.w3p + (((size_t)ntc0 * KS3 + ks) * 64 + l) * 8);
        DMP_SCHED_FENCE();
    }
    // ... and so are the head's per-column constants of every tile this wave owns (branch-free, clamped: one latency for all of them)
    if constexpr (HEAD == 0) {
#pragma unroll
    for (int it = 0; it < NT3W; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * ((w >> 1) + 2 * it) + 4 * g + r, cc = col < p.A ? col : p.A - 1;
            hc_ls[it][r] = p.logstd[cc]; hc_b3[it][r] = p.b3[cc]; hc_as[it][r] = p.a_std[cc]; hc_am[it][r] = p.a_mean[cc];
        }
    }
    DMP_SCHED_FENCE();
    // layer-2 epilogue -> h2 (B-fragment order of layer 3: k = 128 w + 16 n + 4 g + r).  Every wave is past the barrier of the last chunk, so s16 and
    // h1c[0], which h2 overlays, are dead; h1c[1] (still being read by slower waves) lies behind them.
    if constexpr (!GATED) {
        uint16_t* const dst = reinterpret_cast<uint16_t*>(h2);
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int f0 = 128 * w + 16 * n + 4 * g;
            const int ks = 4 * w + (n >> 1), ll = c + 16 * (2 * (n & 1) + (g >> 1));
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                store4(dst + ((size_t)((ks * 2 + b) * 64 + ll)) * 8 + 4 * (g & 1), fmaxf(acc2[n][b][0] + sbias[1024 + f0], 0.0f), fmaxf(acc2[n][b][1] + sbias[1024 + f0 + 1], 0.0f),
                       fmaxf(acc2[n][b][2] + sbias[1024 + f0 + 2], 0.0f), fmaxf(acc2[n][b][3] + sbias[1024 + f0 + 3], 0.0f));
            }
        }
    }
    __syncthreads();
    DMF_STAMP(4)
    if constexpr (HEAD != 0) {
        // layer 3 + scalar head: waves 0 and 1 own batch tiles 0 and 1 of column tile 0; the lanes g = 0 hold column 0 (features 4 g + r) of batch row c
        if (w >= 2) return;
        const int row = row0 + 16 * w + c;
        f32x4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS3; ++ks) acc = mfma16(wf[ks], h2[(ks * 2 + w) * 64 + l], acc);
        if (g == 0 && row < io.M) scalar_head_store(io, row, acc[0] + hb3);
    } else {
        // layer 3 + Gaussian head: wave w owns batch tile w & 1 and the action tiles (w >> 1), (w >> 1) + 2, ...; K = 512
        const int bt = w & 1, row = row0 + 16 * bt + c;
        float lp = 0.0f;
#pragma unroll
        for (int nt = (w >> 1), it = 0; it < (N3T + 1) / 2; ++it, nt += 2) {
            f32x4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < KS3; ++ks) acc = mfma16(wf[ks], h2[(ks * 2 + bt) * 64 + l], acc);
            if (it + 1 < (N3T + 1) / 2) {              // the next tile's fragments, in flight while this tile's head is computed
                const int ntn = nt + 2 < N3T ? nt + 2 : N3T - 1;
#pragma unroll
                for (int ks = 0; ks < KS3; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(p.w3p + (((size_t)ntn * KS3 + ks) * 64 + l) * 8);
            }
            if (nt < N3T) {
                if (io.exp_flags && nt == 0 && g == 0 && row < io.M) io.exp_flags[row] = explore ? 1 : 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = 16 * nt + 4 * g + r;
                    if (col < p.A) {
                        const float ls = hc_ls[it][r];
                        const float z = hz[it][r];
                        const float na = acc[r] + hc_b3[it][r] + expf(ls) * z;
                        if (row < io.M) io.actions[(size_t)row * p.A + col] = na * hc_as[it][r] + hc_am[it][r];
                        lp += -0.5f * z * z - ls;
                    }
                }
            }
        }
        DMF_STAMP(5)
        // log-probability: sum over the four feature groups of a lane column, then over the two waves that share the batch tile
        lp += lane_xor_f(lp, 16); lp += lane_xor_f(lp, 32);
        if (g == 0) lp_part[w][c] = lp;
        __syncthreads();
        if (io.logp && w < 2 && g == 0 && row < io.M) io.logp[row] = lp_part[w][c] + lp_part[w + 2][c] - 0.5f * (float)p.A * 1.8378770664093453f;
        DMF_STAMP(6)
    }
#undef DMF_STAMP
}

// ---------------------------------------------------------------- the packed weights: their layout and the kernel that writes it
// (dm_policy_create(_gated) once with every source given, dm_policy_set_weights with whichever are; host side: policy_pack, dm_policy_host.h)
// ONE launch packs every array of a context from fp32 sources in device memory into the buffers the forward kernels read; nothing else writes them, so the
// layout is what this kernel does:
//  * fragment order (PK_FRAG) of W [K x N] (tf.layers.dense kernel layout: input index first), zero-padded to Kp x Np: [n-tile][k-step][lane][8] bf16 -- row r
//    of the array is lane l = r % 64 of fragment (nt, ks) = (r / 64 / KS, r / 64 % KS), KS = Kp / 32, and holds column n = 16 nt + (l & 15),
//    k = 32 ks + 8 (l >> 4) + i, i = 0 .. 7 (pack_row).  A fragment is 1 KB: the operand of one mfma16, 16 bytes per lane.
//  * fused stream (PK_FUSED; H1 = 1024, H2 = 512, gate_hidden = 64): 1 KB slots of one fragment each, 8 slots to a block, NBLK blocks per wave w = 0 .. 3 of
//    k_policy_fused in the order the wave consumes them.  Per layer-1 chunk q = 0 .. 3: NB1 = K1 / 64 blocks, block b slot 4 kk + j = layer-1 fragment (feature
//    tile 16 q + 4 w + j, k-step 2 b + kk); gated: 3 blocks = 24 slots = the gate tiles of layer 1's feature tiles 16 q + 4 w + j, j = 0 .. 3; then 8 blocks, block
//    ksl slot n = layer-2 fragment (feature tile 8 w + n, k-step 8 q + ksl).  Gated: behind the last chunk 6 blocks = 48 slots = the gate tiles of layer 2's
//    feature tiles 8 w + n, n = 0 .. 7.  A gate tile of feature tile ft is six slots in consumption order: the sigma fragments (gate{i}/dense_1, K = 64) of
//    k-steps 0 and 1, the beta fragments (gate{i}/dense) of k-steps 0 and 1, then lane l's four sigma biases and its four beta biases as fp32 bits (features
//    16 ft + 4 (l >> 4) + r: pack_bias_row).
//  * vectors (PK_VEC) are fp32 as given, zero behind the N source elements (b3 up to N3); s_inv_std is 1 / s_std (PK_RECIP).
//  * fp32 -> bf16: round to nearest even, every NaN -> 0x7fc0 (f32_to_bf16_nan).
// The kernel is DESTINATION-ordered: a job is one destination array, a workgroup is 256 consecutive destination units of one job (PackArgs::first maps blockIdx
// to the job), and a thread owns one unit -- a whole 16-byte fragment row [8 bf16] of a packed weight array or of the fused stream, or one fp32 element of a
// vector.  The thread decodes its row's index as above (for the fused stream: wave, block, slot first, so the stream is written straight from the fp32 sources
// and not copied from w1p / w2p), reads eight fp32 ELEMENTS (sources are only 4-byte aligned: torch views) and writes one vector store.  Source layout by
// PackArgs::out_in: [in x out] row-major (tf.layers.dense: the 16 lanes of a quarter-wave read 64 consecutive bytes per k) or [out x in]
// (torch.nn.Linear.weight: 32 consecutive bytes per lane, 128 per column over the four quarter-waves).  A fused-stream row whose source array is not given keeps
// its bytes (the host adds a job only for a source that is there); with every source given every byte of every array is written.
enum { PK_FRAG = 0, PK_FUSED = 1, PK_VEC = 2, PK_RECIP = 3, PK_MAX_JOBS = 28 };
struct PackJob {
    int kind;
    int K, N;              // PK_FRAG: the source is W [K x N] ([N x K] with out_in), rows / columns behind them are zero padding; PK_VEC / PK_RECIP: N source elements
    int KS;                // PK_FRAG: k-steps of the destination (padded K / 32)
    int rows;              // destination units: 16-byte rows (PK_FRAG, PK_FUSED) or fp32 elements (PK_VEC: zero behind N; PK_RECIP: 1 / x)
    const float* src; void* dst;
};
struct PackFused {         // sources of the fused stream (any may be null: those rows are kept); widths fixed by k_policy_fused: H1 = 1024, H2 = 512, GH = 64
    int gated, NB1, S;     // NB1 = K1 / 64 layer-1 blocks per chunk; w1 is [S x 1024]
    const float *w1, *w2;
    const float *ws[2], *wb[2], *bs[2], *bb[2];   // gate{i}/dense_1 and gate{i}/dense kernels [64 x H_i], their biases [H_i]
};
struct PackArgs { int njobs, out_in; int first[PK_MAX_JOBS + 1]; PackJob job[PK_MAX_JOBS]; PackFused fs; };

// the rounding of the packed weights: to nearest even, every NaN -> 0x7fc0 (the device f32_to_bf16 above has no NaN case)
DMP_DEV uint16_t f32_to_bf16_nan(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
struct alignas(16) u32x4_rec { uint32_t x, y, z, w; };
// the row of lane l in fragment (nt, ks) of W [K x N]: column n = 16 nt + (l & 15), k = 32 ks + 8 (l >> 4) + i
DMP_DEV u32x4_rec pack_row(const float* W, int K, int N, int out_in, int nt, int ks, int l) {
    const int n = 16 * nt + (l & 15), k0 = 32 * ks + 8 * (l >> 4);
    // branch-free: a padding element reads W[0] and is replaced by zero afterwards, so the eight loads of a lane are in flight together
    float f[8]; uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        const size_t at = out_in ? (size_t)n * K + k : (size_t)k * N + n;
        f[i] = W[(k < K && n < N) ? at : 0];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = (k0 + i < K && n < N) ? (uint32_t)f32_to_bf16_nan(f[i]) : 0u;
    u32x4_rec v; v.x = h[0] | (h[1] << 16); v.y = h[2] | (h[3] << 16); v.z = h[4] | (h[5] << 16); v.w = h[6] | (h[7] << 16);
    return v;
}
// slots 4 / 5 of a gate tile: the lane's four biases (features 16 ft + 4 (l >> 4) + r) as fp32 bits
DMP_DEV u32x4_rec pack_bias_row(const float* b, int ft, int l) {
    const float* s = b + 16 * ft + 4 * (l >> 4);
    u32x4_rec v; v.x = __builtin_bit_cast(uint32_t, s[0]); v.y = __builtin_bit_cast(uint32_t, s[1]); v.z = __builtin_bit_cast(uint32_t, s[2]); v.w = __builtin_bit_cast(uint32_t, s[3]);
    return v;
}

__global__ void __launch_bounds__(256) k_policy_pack(PackArgs a) {
    const int b = blockIdx.x;
    int j = 0;
    while (j + 1 < a.njobs && b >= a.first[j + 1]) ++j;
    const int kind = a.job[j].kind, rows = a.job[j].rows;
    const int r = (b - a.first[j]) * 256 + (int)threadIdx.x;
    if (r >= rows) return;
    if (kind == PK_VEC || kind == PK_RECIP) {
        const float* src = a.job[j].src;
        float v = 0.0f;
        if (r < a.job[j].N) v = (kind == PK_RECIP) ? 1.0f / src[r] : src[r];
        static_cast<float*>(a.job[j].dst)[r] = v;
        return;
    }
    u32x4_rec* dst = static_cast<u32x4_rec*>(a.job[j].dst) + r;
    const int f = r >> 6, l = r & 63;                     // fragment of the destination, lane row inside it
    if (kind == PK_FRAG) {
        const int KS = a.job[j].KS;
        *dst = pack_row(a.job[j].src, a.job[j].K, a.job[j].N, a.out_in, f / KS, f % KS, l);
        return;
    }
    // PK_FUSED: f = (w * NBLK + block) * 8 + slot; block = q * NBQ + bq inside the four chunks (NBQ blocks each), the layer-2 gate tiles behind them
    const PackFused& s = a.fs;
    const int NB1 = s.NB1, KS1 = 2 * NB1, NBQ = NB1 + (s.gated ? 11 : 8), NBLK = 4 * NBQ + (s.gated ? 6 : 0);
    const int w = f / (8 * NBLK), blk = (f >> 3) % NBLK, slot = f & 7;
    int layer = -1, ft = 0, gs = 0;                       // a gate slot: layer, feature tile, slot 0 .. 5 of the tile
    if (blk < 4 * NBQ) {
        const int q = blk / NBQ, bq = blk % NBQ;
        if (bq < NB1) {                                   // two k-steps x feature tiles 16 q + 4 w + j of layer 1
            if (s.w1) *dst = pack_row(s.w1, s.S, 1024, a.out_in, 16 * q + 4 * w + (slot & 3), 2 * bq + (slot >> 2), l);
            return;
        }
        if (!s.gated || bq >= NB1 + 3) {                  // k-step 8 q + ksl of layer 2 x feature tiles 8 w + n
            if (s.w2) *dst = pack_row(s.w2, 1024, 512, a.out_in, 8 * w + slot, 8 * q + bq - NB1 - (s.gated ? 3 : 0), l);
            return;
        }
        const int g = (bq - NB1) * 8 + slot;
        layer = 0; ft = 16 * q + 4 * w + g / 6; gs = g % 6;
    } else {
        const int g = (blk - 4 * NBQ) * 8 + slot;
        layer = 1; ft = 8 * w + g / 6; gs = g % 6;
    }
    const int H = layer ? 512 : 1024;
    if (gs < 2) { if (s.ws[layer]) *dst = pack_row(s.ws[layer], 64, H, a.out_in, ft, gs, l); }
    else if (gs < 4) { if (s.wb[layer]) *dst = pack_row(s.wb[layer], 64, H, a.out_in, ft, gs - 2, l); }
    else if (gs == 4) { if (s.bs[layer]) *dst = pack_bias_row(s.bs[layer], ft, l); }
    else if (s.bb[layer]) *dst = pack_bias_row(s.bb[layer], ft, l);
}

}  // namespace dmp
