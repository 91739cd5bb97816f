// PPO actor and critic minibatch updates on the device (include/dm_hip.h dm_train_*, deepmimic_amd/train.py): what PPOAgent._update_actor / _update_critic and
// MPISolver.update do (learning/ppo_agent.py:95-139, 286-309, learning/solvers/mpi_solver.py:33-54) for the plain three-layer nets, on the context that samples.
// Included at the end of dm_host.cpp (shares its runtime shim, dm_policy's kernels and the workgroup tree of dm_ppo_batch.h); in no step-kernel translation unit.
// Out of scope: Adam, one fused training kernel, step-size schedules.  The AMP discriminator update (dm_train_disc_grad) is the second half of this file; the gated nets
// of the AMP task agents are trained by dm_train_gated.h (dm_train_gated_*), which is included behind this file and launches its kernels.
//
// One *_grad call is, in stream order:
//     k_policy_prep, layers 1 and 2     the context's own per-layer kernels (forced: DM_POLICY_* is not read), leaving s16 / h1 / h2 in bf16 as the sampling net had them
//     k_train_head                      one wavefront per 16 rows owns all N3 columns: layer 3 with the MFMA chain of k_policy_layer<2,1,2>, z3 (fp32) and dz3 (bf16, padded
//                                       columns zero) into the workspace, per-row statistics folded over the workgroup's rows in row order into one fp64 partial block
//     k_train_fold                      one workgroup: the partial blocks in a fixed order (contiguous runs per thread, then the tree of dm_ppo_batch.h) -> stats
//     k_train_wgrad x 3, k_train_bgrad x 3, k_train_dgrad x 2        layer 3 first
// Every matrix-core operand is bf16 (RNE), accumulation fp32, gradients fp32.  Nothing is split over the contraction, so there is no partial to fold and no atomic: the
// k-steps of a tile are accumulated in ascending order by one wavefront, two calls on one input give the same bytes.
//
// k_train_wgrad   dW [K x N] = in^T dz: both operands are contracted over the ROW index of row-major arrays.  A wavefront owns a 32 x 32 tile of dW; per 32 batch rows it
//                 stages the 32 x 32 blocks of `in` and `dz` in LDS with 16-byte row reads and takes its fragments back column-wise (8 two-byte LDS reads per fragment;
//                 rows past M are staged as zeros).  The padding columns of s16 are computed and not stored.
// k_train_bgrad   db = the column sums of the same bf16 dz in fp32: per column four contiguous row quarters, each ascending, added in order.
// k_train_dgrad   dz_prev [M x H] = (dz W^T) . [h != 0]: A fragments are 16 bytes of a dz row, B fragments 8 consecutive floats of a master row converted on load (zeros
//                 past the true width of w3), the ReLU mask and the bf16 store in the epilogue.  A wavefront owns 32 rows x 32 columns.
// k_train_sgd<NMAT>   the momentum step, a grid-stride loop over P: the new momentum from exact fp64 products, rounded once; the master by one fmaf.  NMAT: the matrix
//                 ranges under the weight decay, 3 (a plain block) or GATED_MATRICES (a gated one, dm_train_gated.h).
// The 32 x 32 tiles share a toolkit of inline functions (tile_zero, tile_chain_packed, tile_store_masked); the host side has one forward (train_forward), one backward
// launcher (TrainBackward), one step (train_sgd) and one read (train_read), which dm_train_gated.h calls too.
// A non-finite input (observation past the normaliser's clip, action, advantage, old logp, target, master) reaches the gradients as a non-finite value: bf16_rne keeps a
// NaN a NaN, nothing clamps.  (A NaN OBSERVATION is not one: k_policy_prep turns it into -s_clip, as for the sampling net.)
#pragma once

namespace dmt {

using dmp::bf16x8; using dmp::f32x4; using dmp::mfma16;

constexpr int kMaxA = 128;        // action bounds ride in the kernel arguments

// round to nearest even; unlike dmp::f32_to_bf16 a NaN stays a NaN (quiet, sign kept)
DMP_DEV uint16_t bf16_rne(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

DMP_DEV float bf16_f32(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

// ---- the tile toolkit.  A wavefront's 32 x 32 tile is f32x4 acc[2][2]: acc[i][j][r] is row 16 i + 4 g + r, column 16 j + c of the tile (c = lane & 15, g = lane >> 4).
template <int N>
DMP_DEV void tile_zero(f32x4 (&acc)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] = 0.0f;
}
template <int N, int M>
DMP_DEV void tile_zero(f32x4 (&acc)[N][M]) {
#pragma unroll
    for (int i = 0; i < N; ++i) tile_zero(acc[i]);
}

// acc += in[m0 .., :] W[:, n0 ..] with W's PACKED bf16 fragments as the B operand (16 bytes per lane per k-step, what the layer kernels read): in [M x 32 KS] (a row past
// M reads row 0), wp the fragments of W [32 KS x N]; k-steps ascending
DMP_DEV void tile_chain_packed(f32x4 (&acc)[2][2], const uint16_t* in, const uint16_t* wp, int KS, int M, int m0, int n0, int l, int c, int g) {
    const uint16_t* arow[2]; const uint16_t* bcol[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + 16 * i + c;
        arow[i] = in + (size_t)(row < M ? row : 0) * (32 * KS) + 8 * g;
        bcol[i] = wp + ((size_t)(n0 / 16 + i) * KS * 64 + l) * 8;
    }
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = *reinterpret_cast<const bf16x8*>(arow[i] + (size_t)ks * 32);
            fb[i] = *reinterpret_cast<const bf16x8*>(bcol[i] + (size_t)ks * 512);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(fa[i], fb[j], acc[i][j]);
    }
}

// out = bf16(acc) . [h != 0] on the tile's rows below M: the ReLU mask from the saved activation h, h / out [M x ld]
DMP_DEV void tile_store_masked(const f32x4 (&acc)[2][2], const uint16_t* h, uint16_t* out, int ld, int M, int m0, int n0, int c, int g) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + 16 * i + 4 * g + r, col = n0 + 16 * j + c;
                if (row < M) {
                    const size_t at = (size_t)row * ld + col;
                    out[at] = (h[at] & 0x7fffu) ? bf16_rne(acc[i][j][r]) : (uint16_t)0;
                }
            }
}

// exp(x) with every rounding point written down (Cephes expf: k = rint(x log2 e), r = x - k ln 2 in two fmaf, a degree-5 polynomial in Horner form, ldexp), so that
// device, emulator and the numpy mirror (deepmimic_amd/train.py reference_exp) agree bit for bit; within 2 ulp of exp.  NaN -> NaN, +inf -> +inf, -inf -> 0.
DMP_DEV float exp_det(float x) {
    if (!(x == x)) return x;
    x = fminf(fmaxf(x, -104.0f), 89.0f);
    const float kf = rintf(x * 1.44269504088896341f);
    float r = fmaf(kf, -0.693359375f, x); r = fmaf(kf, 2.12194440e-4f, r);
    float p = fmaf(r, 1.9875691500e-4f, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f); p = fmaf(p, r, 4.1665795894e-2f); p = fmaf(p, r, 1.6666665459e-1f); p = fmaf(p, r, 5.0000001201e-1f);
    const float z = r * r;
    const float y = fmaf(p, z, r) + 1.0f;
    return ldexpf(y, (int)kf);
}

enum { HEAD_ACTOR = 0, HEAD_CRITIC = 1 };
enum { PART_WORDS = 8 };          // fp64 words per workgroup partial: actor {sum min(l0, l1), clipped rows, sum ratio, sum logp, sum violation^2}, critic {sum e^2, sum v}

struct HeadArgs {
    int M, kind, bounded;
    const float *actions, *old_logp, *adv, *targets;
    float clip_lo, clip_hi, eps, bwn, nf, c0;  // 1 - eps, 1 + eps, eps, bound_weight / n, n, (-0.5 A) ln 2 pi -- all float, formed on the host (no contraction)
    float* z3; uint16_t* dz3; double* part; float* out;      // out: logp_out / values_out or null
    float bmin[kMaxA], bmax[kMaxA];            // un-normalised action bounds (bounded != 0)
};

// what the actor head makes of one element: u = (x - mu) / sigma with x the normalised action
struct HeadElem { float mu, sg, u; };
DMP_DEV HeadElem head_elem(const dmp::PolicyDev& p, const HeadArgs& a, int row, int col, float mu) {
    HeadElem e; e.mu = mu; e.sg = exp_det(p.logstd[col]);
    const float x = (a.actions[(size_t)row * p.A + col] - p.a_mean[col]) / p.a_std[col];
    e.u = (x - mu) / e.sg;
    return e;
}

__global__ void __launch_bounds__(64) k_train_head(dmp::PolicyDev p, const uint16_t* h2, HeadArgs a) {
    __shared__ double rowv[16][5];
    __shared__ double lanev[64][4];
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int row0 = (int)blockIdx.x * 16, KS = p.H2 / 32, NB = p.N3 / 32, N3 = p.N3;
    const uint16_t* const ap = h2 + (size_t)(row0 + c < a.M ? row0 + c : 0) * p.H2 + 8 * g;
    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sls = 0.0f;
    // ---- layer 3 (the MFMA chain of k_policy_layer<2, 1, 2>: per 16-column tile the k-steps ascending from a zero accumulator), z3 = acc + b3 into the workspace
    for (int cb = 0; cb < NB; ++cb) {
        f32x4 acc[2];
        tile_zero(acc);
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(ap + (size_t)ks * 32);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = mfma16(af, *reinterpret_cast<const bf16x8*>(p.w3p + (((size_t)(2 * cb + j) * KS + ks) * 64 + l) * 8), acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = (2 * cb + j) * 16 + c;
            const bool live = col < p.A;
            const float b3 = live ? p.b3[col] : 0.0f;
            if (live && a.kind == HEAD_ACTOR) sls += p.logstd[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 4 * g + r;
                if (row >= a.M) continue;
                const float mu = live ? acc[j][r] + b3 : 0.0f;
                a.z3[(size_t)row * N3 + col] = mu;
                if (live && a.kind == HEAD_ACTOR) { const HeadElem e = head_elem(p, a, row, col, mu); q[r] = fmaf(e.u, e.u, q[r]); }
            }
        }
    }
    if (a.kind == HEAD_CRITIC) {
        // 0.5 MSE: dz3 = (v - tar) / n in column 0, zeros in the padding columns
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * g + r;
            if (row < a.M) {
                for (int col = c; col < N3; col += 16) if (col != 0) a.dz3[(size_t)row * N3 + col] = 0;
                if (c == 0) {
                    const float v = a.z3[(size_t)row * N3], e = v - a.targets[row];
                    a.dz3[(size_t)row * N3] = bf16_rne(e / a.nf);
                    if (a.out) a.out[row] = v;
                    rowv[4 * g + r][0] = (double)e * (double)e; rowv[4 * g + r][1] = (double)v;
                }
            } else if (c == 0) { rowv[4 * g + r][0] = 0.0; rowv[4 * g + r][1] = 0.0; }
        }
        __syncthreads();
        if (l < 2) { double s = 0.0; for (int m = 0; m < 16; ++m) s += rowv[m][l]; a.part[(size_t)blockIdx.x * PART_WORDS + l] = s; }
        return;
    }
    // ---- actor: logp is a row sum over the 16 lanes of a group (each lane: its columns ascending, then the xor tree), the constant once
    sls += dmp::lane_xor_f(sls, 1); sls += dmp::lane_xor_f(sls, 2); sls += dmp::lane_xor_f(sls, 4); sls += dmp::lane_xor_f(sls, 8);
    const float cst = a.c0 - sls;
    float gi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * g + r;
        float s = q[r];
        s += dmp::lane_xor_f(s, 1); s += dmp::lane_xor_f(s, 2); s += dmp::lane_xor_f(s, 4); s += dmp::lane_xor_f(s, 8);
        gi[r] = 0.0f;
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        if (row < a.M) {
            const float lp = fmaf(-0.5f, s, cst), adv = a.adv[row];
            const float ratio = exp_det(lp - a.old_logp[row]);
            const float l0 = adv * ratio, l1 = adv * fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
            const bool first = !(l0 > l1);                   // tf.minimum sends the gradient of a tie to its first argument; a NaN stays in the gradient
            gi[r] = first ? -(l0 / a.nf) : 0.0f;
            st[0] = (double)(first ? l0 : l1); st[1] = fabsf(ratio - 1.0f) > a.eps ? 1.0 : 0.0; st[2] = (double)ratio; st[3] = (double)lp;
            if (c == 0 && a.out) a.out[row] = lp;
        }
        if (c == 0) for (int k = 0; k < 4; ++k) rowv[4 * g + r][k] = st[k];
    }
    // ---- dz3 = g (x - mu) / sigma^2 + (bound_weight / n) (min(mu - lo, 0) + max(mu - hi, 0)), lo / hi in normalised action space
    double viol[4] = {0.0, 0.0, 0.0, 0.0};
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = (2 * cb + j) * 16 + c;
            const bool live = col < p.A;
            float lo = 0.0f, hi = 0.0f;
            if (live && a.bounded) { lo = (a.bmin[col] - p.a_mean[col]) / p.a_std[col]; hi = (a.bmax[col] - p.a_mean[col]) / p.a_std[col]; }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 4 * g + r;
                if (row >= a.M) continue;
                float dz = 0.0f;
                if (live) {
                    const HeadElem e = head_elem(p, a, row, col, a.z3[(size_t)row * N3 + col]);
                    dz = gi[r] * (e.u / e.sg);
                    if (a.bounded) {
                        const float vlo = fminf(e.mu - lo, 0.0f), vhi = fmaxf(e.mu - hi, 0.0f);
                        dz = fmaf(a.bwn, vlo + vhi, dz);
                        viol[r] += (double)vlo * (double)vlo; viol[r] += (double)vhi * (double)vhi;
                    }
                }
                a.dz3[(size_t)row * N3 + col] = live ? bf16_rne(dz) : (uint16_t)0;
            }
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) lanev[l][r] = viol[r];
    __syncthreads();
    if (c == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) { double s = 0.0; for (int k = 0; k < 16; ++k) s += lanev[16 * g + k][r]; rowv[4 * g + r][4] = s; }
    __syncthreads();
    if (l < 5) { double s = 0.0; for (int m = 0; m < 16; ++m) s += rowv[m][l]; a.part[(size_t)blockIdx.x * PART_WORDS + l] = s; }
}

// the partial blocks of k_train_head in a fixed order -> stats (actor: double[6], critic: double[2])
__global__ void __launch_bounds__(256) k_train_fold(const double* part, int groups, int kind, int n, double* stats) {
    __shared__ double red[dmb::kThreads];
    const int t = (int)threadIdx.x, per = (groups + dmb::kThreads - 1) / dmb::kThreads, g0 = t * per, g1 = (g0 + per < groups) ? g0 + per : groups;
    double tot[5];
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int g = g0; g < g1; ++g) s += part[(size_t)g * PART_WORDS + k];
        tot[k] = dmb::block_sum(s, red);
        if (kind == HEAD_CRITIC && k == 1) break;
    }
    if (t != 0) return;
    const double dn = (double)n;
    if (kind == HEAD_CRITIC) { stats[0] = 0.5 * tot[0] / dn; stats[1] = tot[1] / dn; return; }
    stats[0] = dn; stats[1] = -(tot[0] / dn); stats[2] = 0.5 * tot[4] / dn; stats[3] = tot[1] / dn; stats[4] = tot[2] / dn; stats[5] = tot[3] / dn;
}

struct WgradArgs { const uint16_t* in; int ldin, K; const uint16_t* dz; int lddz, N; int M; float* dW; };

// ACC: the tile is ADDED to what dW holds (one fp32 add per element by its one owner): the penalty's contribution on top of the least-squares gradient (dm_train_disc_grad)
template <bool ACC>
__global__ void __launch_bounds__(64) k_train_wgrad(WgradArgs a) {
    constexpr int PITCH = 40;                    // halves per staged row: 80 bytes, so a 16-byte record stays aligned
    __shared__ alignas(16) uint16_t sa[32 * PITCH];
    __shared__ alignas(16) uint16_t sb[32 * PITCH];
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int nbn = (a.N + 31) / 32, k0 = ((int)blockIdx.x / nbn) * 32, n0 = ((int)blockIdx.x % nbn) * 32;
    const int mr = l >> 1, hf = l & 1;           // staging: this lane moves the 16 columns 16 hf .. of block row mr
    f32x4 acc[2][2];
    tile_zero(acc);
    bf16x8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) dmp::set8(zero, e, 0);
    for (int m0 = 0; m0 < a.M; m0 += 32) {
        const int row = m0 + mr;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            bf16x8 ra = zero, rb = zero;
            if (row < a.M) {
                ra = *reinterpret_cast<const bf16x8*>(a.in + (size_t)row * a.ldin + k0 + 16 * hf + 8 * v);
                rb = *reinterpret_cast<const bf16x8*>(a.dz + (size_t)row * a.lddz + n0 + 16 * hf + 8 * v);
            }
            *reinterpret_cast<bf16x8*>(sa + mr * PITCH + 16 * hf + 8 * v) = ra;
            *reinterpret_cast<bf16x8*>(sb + mr * PITCH + 16 * hf + 8 * v) = rb;
        }
        __syncthreads();
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) { dmp::set8(fa[i], e, sa[(8 * g + e) * PITCH + 16 * i + c]); dmp::set8(fb[i], e, sb[(8 * g + e) * PITCH + 16 * i + c]); }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(fa[i], fb[j], acc[i][j]);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = k0 + 16 * i + 4 * g + r, col = n0 + 16 * j + c;
                if (row < a.K && col < a.N) {
                    float* const at = a.dW + (size_t)row * a.N + col;
                    if constexpr (ACC) *at = *at + acc[i][j][r]; else *at = acc[i][j][r];
                }
            }
}

// four wavefronts per 64 columns: wave s adds the s-th contiguous quarter of the rows, ascending (16 independent loads in flight, added in row order), then the quarters in order
// ACC: db = (db + the column sums), then with w the regulariser db = fmaf(reg, w, db) -- dw3 of dm_train_disc_grad (M = 0: the regulariser alone)
template <bool ACC>
__global__ void __launch_bounds__(256) k_train_bgrad(const uint16_t* dz, int lddz, int N, int M, float* db, const float* w, float reg) {
    __shared__ float part[4][64];
    const int t = (int)threadIdx.x, cl = t & 63, sl = t >> 6, col = (int)blockIdx.x * 64 + cl;
    const int q = (M + 3) / 4, m0 = sl * q, m1 = (m0 + q < M) ? m0 + q : M;
    float s = 0.0f;
    if (col < N) {
        int m = m0;
        for (; m + 16 <= m1; m += 16) {
            uint16_t v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = dz[(size_t)(m + u) * lddz + col];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += bf16_f32(v[u]);
        }
        for (; m < m1; ++m) s += bf16_f32(dz[(size_t)m * lddz + col]);
    }
    part[sl][cl] = s;
    __syncthreads();
    if (sl == 0 && col < N) {
        float v = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
        if constexpr (ACC) { v = db[col] + v; if (w) v = fmaf(reg, w[col], v); }
        db[col] = v;
    }
}

struct DgradArgs { const uint16_t* dz; int lddz; const float* W; int ldw; const uint16_t* h; int H; int M; uint16_t* out; };
// the layer-1 form (INPUT = true; dm_train_disc_grad): gx = g1 W1^T with W [S x ldw] the layer-1 master, rows S .. H - 1 (H = K1) read as zero; no mask; per row the fp32
// sum of squares of the tile's 32 columns -> sq [M x H / 32]; out = bf16(gx scale), the padding columns zero
struct DgradInArgs : DgradArgs { int S; float scale; float* sq; };
template <bool INPUT> struct DgradSel { typedef DgradArgs type; };
template <> struct DgradSel<true> { typedef DgradInArgs type; };

template <bool INPUT>
__global__ void __launch_bounds__(64) k_train_dgrad(typename DgradSel<INPUT>::type a) {
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int rbn = (a.M + 31) / 32, m0 = ((int)blockIdx.x % rbn) * 32, k0 = ((int)blockIdx.x / rbn) * 32;      // consecutive workgroups walk down the rows under one block of W
    f32x4 acc[2][2];
    tile_zero(acc);
    const uint16_t* arow[2]; const float* wrow[2]; bool wlive[2] = {true, true};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + 16 * i + c;
        arow[i] = a.dz + (size_t)(row < a.M ? row : 0) * a.lddz + 8 * g;
        if constexpr (INPUT) { wlive[i] = k0 + 16 * i + c < a.S; wrow[i] = a.W + (size_t)(wlive[i] ? k0 + 16 * i + c : 0) * a.ldw + 8 * g; }
        else wrow[i] = a.W + (size_t)(k0 + 16 * i + c) * a.ldw + 8 * g;
    }
    for (int nk = 0; nk < a.lddz; nk += 32) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = *reinterpret_cast<const bf16x8*>(arow[i] + nk);
#pragma unroll
            for (int e = 0; e < 8; ++e) dmp::set8(fb[i], e, nk + 8 * g + e < a.ldw && (!INPUT || wlive[i]) ? bf16_rne(wrow[i][nk + e]) : (uint16_t)0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(fa[i], fb[j], acc[i][j]);
    }
    if constexpr (INPUT) {
        // per row: the lane's two columns (v0 v0, then fmaf(v1, v1, .)), then the pairwise tree over the 16 lanes of the group
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + 16 * i + 4 * g + r;
                const float v0 = acc[i][0][r], v1 = acc[i][1][r];
                float q = v0 * v0; q = fmaf(v1, v1, q);
                q += dmp::lane_xor_f(q, 1); q += dmp::lane_xor_f(q, 2); q += dmp::lane_xor_f(q, 4); q += dmp::lane_xor_f(q, 8);
                if (row < a.M) {
                    if (c == 0) a.sq[(size_t)row * (a.H / 32) + k0 / 32] = q;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int col = k0 + 16 * j + c;
                        a.out[(size_t)row * a.H + col] = col < a.S ? bf16_rne(acc[i][j][r] * a.scale) : (uint16_t)0;
                    }
                }
            }
        return;
    }
    tile_store_masked(acc, a.h, a.out, a.H, a.M, m0, k0, c, g);
}

// NMAT: the matrix ranges [mat[k][0], mat[k][1]) of the block, the entries under the weight decay -- 3 for a plain net, GATED_MATRICES for a gated one, where
// _weight_decay_loss (learning/tf_agent.py) drops only the variables whose name contains "bias", and actor/gate{i}/dense/kernel -- the beta projection -- is not one
enum { GATED_ARRAYS = 20, GATED_MATRICES = 10 };
template <int NMAT> struct SgdArgs { float* w; float* v; const float* g; long long P, mat[NMAT][2]; float lr, mom, wd, gs; unsigned blocks; };

template <int NMAT>
__global__ void __launch_bounds__(256) k_train_sgd(SgdArgs<NMAT> a) {
    for (long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x; i < a.P; i += (long long)a.blocks * 256) {
        const float w = a.w[i];
        // g is carried in fp64, where every product of two floats is exact (a contraction changes nothing), and v is rounded ONCE: under cancellation between
        // momentum * v and g a chain of fp32 roundings would be off by many ulps of the small result
        double gg = (double)a.gs * (double)a.g[i];
        // (The three ranges of a plain block are one spelled-out chain: written as the loop, the same test costs the plain kernel two SGPRs and a VGPR.)
        bool matrix = false;
        if constexpr (NMAT == 3) matrix = (i >= a.mat[0][0] && i < a.mat[0][1]) || (i >= a.mat[1][0] && i < a.mat[1][1]) || (i >= a.mat[2][0] && i < a.mat[2][1]);
        else for (int k = 0; k < NMAT; ++k) matrix = matrix || (i >= a.mat[k][0] && i < a.mat[k][1]);
        if (matrix) gg += (double)a.wd * (double)w;          // _weight_decay_loss skips the biases
        const float vv = (float)((double)a.mom * (double)a.v[i] + gg);
        a.v[i] = vv;
        a.w[i] = fmaf(-a.lr, vv, w);
    }
}

// offsets (in floats) of w1, b1, w2, b2, w3, b3 in a parameter block and its length
struct Layout { long long o[6], P; };
inline Layout layout_of(const dmp::PolicyDev& d) {
    Layout L; const long long S = d.S, H1 = d.H1, H2 = d.H2, A = d.A;
    L.o[0] = 0; L.o[1] = S * H1; L.o[2] = L.o[1] + H1; L.o[3] = L.o[2] + H1 * H2; L.o[4] = L.o[3] + H2; L.o[5] = L.o[4] + H2 * A; L.P = L.o[5] + A;
    return L;
}
// the caller's workspace: [z3 fp32 n x N3][dz3 bf16 n x N3][dz2 bf16 n x H2][dz1 bf16 n x H1][ceil(n / 16) partial blocks of PART_WORDS doubles]; every piece starts on a multiple of 16 bytes
struct Work { float* z3; uint16_t *dz3, *dz2, *dz1; double* part; size_t bytes; };
inline Work carve(const dmp::PolicyDev& d, int n, void* ws) {
    Work w; char* at = (char*)ws;
    w.z3 = (float*)at; at += (size_t)n * d.N3 * 4;
    w.dz3 = (uint16_t*)at; at += (size_t)n * d.N3 * 2;
    w.dz2 = (uint16_t*)at; at += (size_t)n * d.H2 * 2;
    w.dz1 = (uint16_t*)at; at += (size_t)n * d.H1 * 2;
    w.part = (double*)at; at += (size_t)((n + 15) / 16) * PART_WORDS * sizeof(double);
    w.bytes = (size_t)(at - (char*)ws);
    return w;
}

// ---------------------------------------------------------------- the AMP discriminator update (dm_train_disc_grad): AMPAgent._step_disc, learning/amp_agent.py:134-207, 251-257
// loss = 0.5 (mean_e 0.5 (y - 1)^2 + mean_a 0.5 (y + 1)^2) + c_gp 0.5 mean_e |dy/dx|^2 + c_lr 0.5 |w3|^2 on the plain ReLU net with one output; expert rows first.
// relu'' = 0 almost everywhere, so the penalty's gradient is first-order algebra on the saved activations (m_k = [h_k != 0]):
//     g2 = bf16(w3)^T . m2        g1 = (g2 W2^T) . m1        gx = g1 W1^T        a = gx (c_gp / n_e)
//     dW1 += a^T g1       t1 = (a W1) . m1       dW2 += t1^T g2       dw3 += colsum((t1 W2) . m2)       dw3 = fmaf(c_lr, w3, dw3)
// One call is, in stream order: k_policy_prep x 2 (expert rows, then agent rows behind them), layers 1 and 2, k_train_disc_head (which also writes g2), the least-squares
// backward pass above over all rows, then on the expert rows k_train_dgrad<false> (g1), k_train_dgrad<true> (a, |gx|^2), k_train_fwdm x 2 (t1, t2),
// k_train_wgrad<true> x 2, k_train_bgrad<true>, and k_train_disc_wnorm, k_train_disc_fold for the statistics.  Each gradient element has one owner: the least-squares
// value is written first, the penalty's own contraction (from a zero accumulator, k-steps ascending) is added to it by one fp32 add, the regulariser last by one fmaf.
//
// k_train_fwdm    out [M x N] = (in W) . [h != 0], bf16: the contraction over the ROW index of W.  Its B operand is the context's PACKED bf16 weights (w1p / w2p) and not the
//                 masters: the packed arrays ARE W in the B-fragment order of this contraction (16 bytes per lane per k-step, what the layer kernels read), by the
//                 precondition of the *_grad calls they are the RNE bf16 of the masters, and a read of the masters would be eight floats from eight different rows per
//                 fragment plus a conversion.  A wavefront owns 32 rows x 32 columns, k-steps ascending from a zero accumulator.
enum { DISC_STATS = 8, DISC_WN_BLOCKS = 64 };

struct DiscHeadArgs { int M, ne; float nef, naf; int penalty; const float* w3; float* z3; uint16_t* dz3; uint16_t* g2; double* part; float* out; };

DMP_DEV uint16_t get8(const bf16x8& f, int i) {
#ifdef DM_EMU
    return f.v[i];
#else
    return (uint16_t)f[i];
#endif
}

// one wavefront per 16 rows: layer 3 on column tile 0 (the chain of the scalar head k_policy_layer<2, 1, 1, false, 1>), y = acc + b3, t = +1 (expert) / -1 (agent),
// dz3 = (0.5 (y - t)) / n_side in column 0; the partial block {sum_e e^2, sum_a e^2, #e[y > 0], #a[y < 0], sum_a sigmoid(y), sum_a |y|}; g2 of its expert rows
__global__ void __launch_bounds__(64) k_train_disc_head(dmp::PolicyDev p, const uint16_t* h2, DiscHeadArgs a) {
    __shared__ double rowv[16][6];
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int row0 = (int)blockIdx.x * 16, KS = p.H2 / 32, N3 = p.N3;
    const uint16_t* const ap = h2 + (size_t)(row0 + c < a.M ? row0 + c : 0) * p.H2 + 8 * g;
    f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
    for (int ks = 0; ks < KS; ++ks)
        acc = mfma16(*reinterpret_cast<const bf16x8*>(ap + (size_t)ks * 32), *reinterpret_cast<const bf16x8*>(p.w3p + ((size_t)ks * 64 + l) * 8), acc);
    const float b3 = p.b3[0];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * g + r;
        double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (row < a.M) {
            for (int col = c; col < N3; col += 16) if (col != 0) { a.z3[(size_t)row * N3 + col] = 0.0f; a.dz3[(size_t)row * N3 + col] = 0; }
            if (c == 0) {
                const bool expert = row < a.ne;
                const float y = acc[r] + b3, e = y - (expert ? 1.0f : -1.0f);
                a.z3[(size_t)row * N3] = y;
                a.dz3[(size_t)row * N3] = bf16_rne((0.5f * e) / (expert ? a.nef : a.naf));
                if (a.out) a.out[row] = y;
                st[expert ? 0 : 1] = (double)e * (double)e;
                if (expert) st[2] = y > 0.0f ? 1.0 : 0.0;
                else { st[3] = y < 0.0f ? 1.0 : 0.0; st[4] = (double)(1.0f / (1.0f + exp_det(-y))); st[5] = (double)fabsf(y); }
            }
        }
        if (c == 0) for (int k = 0; k < 6; ++k) rowv[4 * g + r][k] = st[k];
    }
    __syncthreads();
    if (l < 6) { double s = 0.0; for (int m = 0; m < 16; ++m) s += rowv[m][l]; a.part[(size_t)blockIdx.x * PART_WORDS + l] = s; }
    if (!a.penalty) return;
    for (int m = 0; m < 16; ++m) {
        const int row = row0 + m;
        if (row >= a.ne) break;
        for (int k = 8 * l; k < p.H2; k += 512) {
            const bf16x8 hv = *reinterpret_cast<const bf16x8*>(h2 + (size_t)row * p.H2 + k);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) dmp::set8(o, e, (get8(hv, e) & 0x7fffu) ? bf16_rne(a.w3[k + e]) : (uint16_t)0);
            *reinterpret_cast<bf16x8*>(a.g2 + (size_t)row * p.H2 + k) = o;
        }
    }
}

struct FwdmArgs { const uint16_t* in; const uint16_t* wp; int KS; const uint16_t* h; int N; int M; uint16_t* out; };      // in [M x 32 KS], wp: fragments of W [32 KS x N], h / out [M x N]

__global__ void __launch_bounds__(64) k_train_fwdm(FwdmArgs a) {
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int rbn = (a.M + 31) / 32, m0 = ((int)blockIdx.x % rbn) * 32, n0 = ((int)blockIdx.x / rbn) * 32;      // consecutive workgroups walk down the rows under one block of W
    f32x4 acc[2][2];
    tile_zero(acc);
    tile_chain_packed(acc, a.in, a.wp, a.KS, a.M, m0, n0, l, c, g);
    tile_store_masked(acc, a.h, a.out, a.N, a.M, m0, n0, c, g);
}

// the sums of squares of the masters in fp64: workgroup b takes the b-th contiguous chunk of the parameter block, thread t its elements t, t + 256, .. ascending, then the
// tree of dm_ppo_batch.h -> wn[2 b] (the three matrices), wn[2 b + 1] (w3 alone)
__global__ void __launch_bounds__(256) k_train_disc_wnorm(const float* params, Layout L, int blocks, double* wn) {
    __shared__ double red[dmb::kThreads];
    const long long chunk = (L.P + blocks - 1) / blocks, lo = (long long)blockIdx.x * chunk, hi = lo + chunk < L.P ? lo + chunk : L.P;
    double sm = 0.0, s3 = 0.0;
    for (long long i = lo + (long long)threadIdx.x; i < hi; i += 256) {
        const double x = (double)params[i], xx = x * x;
        if ((i >= L.o[0] && i < L.o[1]) || (i >= L.o[2] && i < L.o[3]) || (i >= L.o[4] && i < L.o[5])) sm += xx;
        if (i >= L.o[4] && i < L.o[5]) s3 += xx;
    }
    sm = dmb::block_sum(sm, red); s3 = dmb::block_sum(s3, red);
    if (threadIdx.x == 0) { wn[2 * (size_t)blockIdx.x] = sm; wn[2 * (size_t)blockIdx.x + 1] = s3; }
}

struct DiscFoldArgs { const double* part; int groups; const float* sq; long long nsq; const double* wn; int wblocks; int ne, na; double* stats; };

// one workgroup: every array by contiguous runs per thread, then the tree -> stats {least-squares loss, acc_expert, acc_agent, mean_a sigmoid(y), mean_a |y|,
// gradient penalty 0.5 mean_e |gx|^2, 0.5 |w3|^2, 0.5 sum_k |W_k|^2}
__global__ void __launch_bounds__(256) k_train_disc_fold(DiscFoldArgs a) {
    __shared__ double red[dmb::kThreads];
    const int t = (int)threadIdx.x;
    double tot[9];
    {
        const int per = (a.groups + dmb::kThreads - 1) / dmb::kThreads, g0 = t * per, g1 = (g0 + per < a.groups) ? g0 + per : a.groups;
        for (int k = 0; k < 6; ++k) {
            double s = 0.0;
            for (int g = g0; g < g1; ++g) s += a.part[(size_t)g * PART_WORDS + k];
            tot[k] = dmb::block_sum(s, red);
        }
    }
    {
        const long long per = (a.nsq + dmb::kThreads - 1) / dmb::kThreads, i0 = t * per, i1 = (i0 + per < a.nsq) ? i0 + per : a.nsq;
        double s = 0.0;
        for (long long i = i0; i < i1; ++i) s += (double)a.sq[i];
        tot[6] = dmb::block_sum(s, red);
    }
    for (int k = 0; k < 2; ++k) {
        double s = 0.0;
        if (t < a.wblocks) s = a.wn[2 * t + k];
        tot[7 + k] = dmb::block_sum(s, red);
    }
    if (t != 0) return;
    const double de = (double)a.ne, da = (double)a.na;
    a.stats[0] = 0.5 * (0.5 * tot[0] / de + 0.5 * tot[1] / da);
    a.stats[1] = tot[2] / de; a.stats[2] = tot[3] / da; a.stats[3] = tot[4] / da; a.stats[4] = tot[5] / da;
    a.stats[5] = 0.5 * tot[6] / de; a.stats[6] = 0.5 * tot[8]; a.stats[7] = 0.5 * tot[7];
}

// the discriminator call's workspace: the pieces of `carve` for n = n_e + n_a rows, then [g2 bf16 n_e x H2][g1 bf16 n_e x H1][a bf16 n_e x K1][t1 bf16 n_e x H1]
// [t2 bf16 n_e x H2][sq fp32 n_e x K1 / 32, padded to 16 bytes][wn 64 x 2 doubles]
struct DiscWork { Work w; uint16_t *g2, *g1, *a, *t1, *t2; float* sq; double* wn; size_t bytes; };
inline DiscWork carve_disc(const dmp::PolicyDev& d, int ne, int na, void* ws) {
    DiscWork k; k.w = carve(d, ne + na, ws);
    char* at = (char*)ws + k.w.bytes;
    k.g2 = (uint16_t*)at; at += (size_t)ne * d.H2 * 2;
    k.g1 = (uint16_t*)at; at += (size_t)ne * d.H1 * 2;
    k.a = (uint16_t*)at; at += (size_t)ne * d.K1 * 2;
    k.t1 = (uint16_t*)at; at += (size_t)ne * d.H1 * 2;
    k.t2 = (uint16_t*)at; at += (size_t)ne * d.H2 * 2;
    k.sq = (float*)at; at += ((size_t)ne * (d.K1 / 32) * 4 + 15) / 16 * 16;
    k.wn = (double*)at; at += (size_t)DISC_WN_BLOCKS * 2 * sizeof(double);
    k.bytes = (size_t)(at - (char*)ws);
    return k;
}

}  // namespace dmt

static int train_net_ok(const char* fn, const dm_policy* p) {
    if (!p) return fail(std::string(fn) + ": null net");
    if (p->gated) return fail(std::string(fn) + ": a gated context (dm_policy_create_gated) is not trained here: the plain three-layer nets only (a gated net: dm_train_gated_*)");
    return 0;
}

// the refusals every *_grad call takes from here, the discriminator's included.  train_rows_ok: the row count the kernels' int indices hold; train_ws_ok: the workspace
// against `need`, the bytes of the call's carve, which `sizer` states, and the alignment of the workspace and the statistics
static int train_rows_ok(const char* fn, const dmp::PolicyDev& d, long long n) {
    if (n * std::max(std::max(d.K1, d.H1), d.H2) > 0x7fffffffLL) return fail(std::string(fn) + ": too many rows for one call");
    return 0;
}
static int train_ws_ok(const char* fn, const double* stats, const void* ws, int64_t ws_bytes, size_t need, const char* sizer) {
    if (ws_bytes < (int64_t)need) return fail(std::string(fn) + ": workspace too small (" + sizer + ")");
    if ((((uintptr_t)ws) & 15) != 0 || (((uintptr_t)stats) & 7) != 0) return fail(std::string(fn) + ": the workspace must be 16-byte and stats 8-byte aligned");
    return 0;
}

// what the actor and critic *_grad calls (plain and gated) refuse alike in their common arguments
static int train_args_ok(const dm_policy* p, const char* fn, const float* params, const float* states, const float* goals, int goal_dim, int n, const float* grads,
                         const double* stats, const void* ws, int64_t ws_bytes, size_t need, const char* sizer) {
    if (n < 1) return fail(std::string(fn) + ": n must be >= 1");
    if (!params || !states || !grads || !stats || !ws) return fail(std::string(fn) + ": null argument");
    if (check_goal(p, fn, "net", goals, goal_dim)) return -1;
    return train_rows_ok(fn, p->pd, n) || train_ws_ok(fn, stats, ws, ws_bytes, need, sizer) ? -1 : 0;
}

// The forward pass of every *_grad call: k_policy_prep on n rows of `states` (null: the caller has filled s16 -- dm_train_disc_grad's two batches), a gated context's
// k_policy_gate, then layers 1 and 2 on the context's own per-layer kernels -- the forced route, DM_POLICY_* is not read -- leaving s16 / h1 / h2 in bf16 as the sampling
// net had them and, gated, sigma_i / beta_i in fp32 (gbuf)
static void train_forward(dm_policy* p, const float* states, const float* goals, int goal_dim, int n, rt_stream stream) {
    const dmp::PolicyDev& d = p->pd;
    dmp::PolicyIO io; memset(&io, 0, sizeof(io));
    io.states = states; io.M = n; io.goals = goal_dim ? goals : nullptr; io.G = goal_dim; io.exp_rate = 1.0f;
    io.s16 = p->s16; io.h1 = p->h1; io.h2 = p->h2;
    if (p->gated) { io.gsig0 = p->gbuf[0]; io.gbeta0 = p->gbuf[1]; io.gsig1 = p->gbuf[2]; io.gbeta1 = p->gbuf[3]; io.gate = p->gd_dev; }
    if (states) RT_LAUNCH(dmp::k_policy_prep, n, stream, d, io);
    if (!p->gated) return launch_layers<false>(policy_path_layered(d), n, stream, d, io);
    RT_LAUNCH4(dmp::k_policy_gate, (n + 31) / 32, stream, d, io, p->gd);
    launch_layers<true>(policy_path_layered(d), n, stream, d, io);
}

// k_train_head and k_train_fold of an actor or critic call, on the h2 the forward left
static void train_head(const dm_policy* p, int n, dmt::HeadArgs& ha, const dmt::Work& w, double* stats, rt_stream stream) {
    const int groups = (n + 15) / 16;
    ha.M = n; ha.nf = (float)n; ha.z3 = w.z3; ha.dz3 = w.dz3; ha.part = w.part;
    RT_LAUNCH(dmt::k_train_head, groups, stream, p->pd, (const uint16_t*)p->h2, ha);
    RT_LAUNCH4(dmt::k_train_fold, 1, stream, (const double*)w.part, groups, ha.kind, n, stats);
}

// The backward launches of a *_grad call over n rows: masters read from `params` and gradients written into `grads` at offsets (in floats) of the call's layout
struct TrainBackward {
    rt_stream stream; int n; const float* params; float* grads;
    // dW [K x N] = in^T dz at offset ow, and db = the column sums of dz at offset ob
    void wgrad_bgrad(const uint16_t* in, int ldin, int K, const uint16_t* dz, int lddz, int N, long long ow, long long ob) const {
        dmt::WgradArgs wa; wa.in = in; wa.ldin = ldin; wa.K = K; wa.dz = dz; wa.lddz = lddz; wa.N = N; wa.M = n; wa.dW = grads + ow;
        RT_LAUNCH(dmt::k_train_wgrad<false>, ((K + 31) / 32) * ((N + 31) / 32), stream, wa);
        RT_LAUNCH4(dmt::k_train_bgrad<false>, (N + 63) / 64, stream, dz, lddz, N, n, grads + ob, (const float*)nullptr, 0.0f);
    }
    // out [n x H] = bf16((dz W^T) . [h != 0]) with W [H x ldw] the master at offset ow
    void dgrad(const uint16_t* dz, int lddz, long long ow, int ldw, const uint16_t* h, int H, uint16_t* out) const {
        dmt::DgradArgs da; da.dz = dz; da.lddz = lddz; da.W = params + ow; da.ldw = ldw; da.h = h; da.H = H; da.M = n; da.out = out;
        RT_LAUNCH(dmt::k_train_dgrad<false>, ((n + 31) / 32) * (H / 32), stream, da);
    }
    // the plain three-layer net from the dz3 in the workspace, layer 3 first
    void plain_backward(const dm_policy* p, const dmt::Work& w, const dmt::Layout& L) const {
        const dmp::PolicyDev& d = p->pd;
        const uint16_t* in[3] = {p->s16, p->h1, p->h2}; const int ldin[3] = {d.K1, d.H1, d.H2}, K[3] = {d.S, d.H1, d.H2};
        uint16_t* dz[3] = {w.dz1, w.dz2, w.dz3}; const int lddz[3] = {d.H1, d.H2, d.N3}, N[3] = {d.H1, d.H2, d.A};
        for (int layer = 2; layer >= 0; --layer) {
            wgrad_bgrad(in[layer], ldin[layer], K[layer], dz[layer], lddz[layer], N[layer], L.o[2 * layer], L.o[2 * layer + 1]);
            if (layer > 0) dgrad(dz[layer], lddz[layer], L.o[2 * layer], N[layer], in[layer], K[layer], dz[layer - 1]);
        }
    }
};

// what the two *_grad calls share behind their own checks: the forward pass, the head, the fold and the backward pass
static int train_grad(dm_policy* p, const char* fn, const float* params, const float* states, const float* goals, int goal_dim, int n, dmt::HeadArgs& ha, float* grads,
                      double* stats, void* ws, int64_t ws_bytes, void* hip_stream) {
    const dmt::Work w = dmt::carve(p->pd, n, ws);
    if (train_args_ok(p, fn, params, states, goals, goal_dim, n, grads, stats, ws, ws_bytes, w.bytes, "dm_train_workspace_bytes")) return -1;
    DevGuard guard(p->device_id);
    rt_stream stream = (rt_stream)hip_stream;
    if (policy_grow(p, n, stream)) return -1;
    train_forward(p, states, goals, goal_dim, n, stream);
    train_head(p, n, ha, w, stats, stream);
    TrainBackward{stream, n, params, grads}.plain_backward(p, w, dmt::layout_of(p->pd));
    return launch_status(0);
}

// the head's own checks and its kernel arguments, for the plain and the gated call alike (the caller has checked the net)
static int train_actor_head(const char* fn, const dm_policy* net, int n, const float* actions_dev, const float* old_logp_dev, const float* adv_dev, const dm_train_actor_cfg* cfg,
                            float* logp_out, dmt::HeadArgs& ha) {
    if (!actions_dev || !old_logp_dev || !adv_dev || !cfg) return fail(std::string(fn) + ": null argument");
    if (!(cfg->ratio_clip > 0.0)) return fail(std::string(fn) + ": ratio_clip must be > 0");
    if (!(cfg->bound_weight >= 0.0)) return fail(std::string(fn) + ": bound_weight must be >= 0");
    if ((cfg->a_bound_min == nullptr) != (cfg->a_bound_max == nullptr)) return fail(std::string(fn) + ": a_bound_min and a_bound_max come together (both NULL: no bound loss)");
    const dmp::PolicyDev& d = net->pd;
    if (!d.logstd || !d.a_mean || !d.a_std) return fail(std::string(fn) + ": the context holds no logstd / a_mean / a_std");
    if (d.A > dmt::kMaxA) return fail(std::string(fn) + ": action_dim above 128 is not compiled (the action bounds ride in the kernel arguments)");
    memset(&ha, 0, sizeof(ha));
    ha.kind = dmt::HEAD_ACTOR; ha.actions = actions_dev; ha.old_logp = old_logp_dev; ha.adv = adv_dev; ha.out = logp_out;
    ha.eps = (float)cfg->ratio_clip; ha.clip_lo = 1.0f - ha.eps; ha.clip_hi = 1.0f + ha.eps;
    ha.bounded = cfg->a_bound_min ? 1 : 0;
    ha.c0 = (-0.5f * (float)d.A) * 1.8378770664093453f;
    if (n >= 1) ha.bwn = (float)cfg->bound_weight / (float)n;
    if (ha.bounded) for (int j = 0; j < d.A; ++j) { ha.bmin[j] = cfg->a_bound_min[j]; ha.bmax[j] = cfg->a_bound_max[j]; }
    return 0;
}

static int train_value_head(const char* fn, const dm_policy* net, const float* targets_dev, float* values_out, dmt::HeadArgs& ha) {
    if (net->pd.A != 1) return fail(std::string(fn) + ": the context has action_dim " + std::to_string(net->pd.A) + ", the value head needs a net with one output");
    if (!targets_dev) return fail(std::string(fn) + ": null argument");
    memset(&ha, 0, sizeof(ha));
    ha.kind = dmt::HEAD_CRITIC; ha.targets = targets_dev; ha.out = values_out;
    return 0;
}

// what the plain and the gated step refuse alike in their arrays and scalars
static int train_step_ok(const char* fn, const float* params_dev, const float* momentum_dev, const float* grads_dev, int64_t P, double stepsize, double momentum,
                         double weight_decay, double grad_scale) {
    if (!params_dev || !momentum_dev || !grads_dev) return fail(std::string(fn) + ": null argument");
    if (P < 1) return fail(std::string(fn) + ": P must be >= 1");
    if (!(stepsize >= 0.0 && std::isfinite(stepsize))) return fail(std::string(fn) + ": stepsize must be finite and >= 0");
    if (!(momentum >= 0.0 && std::isfinite(momentum))) return fail(std::string(fn) + ": momentum must be finite and >= 0");
    if (!(weight_decay >= 0.0 && std::isfinite(weight_decay))) return fail(std::string(fn) + ": weight_decay must be finite and >= 0");
    if (!std::isfinite(grad_scale)) return fail(std::string(fn) + ": grad_scale must be finite");
    return 0;
}

// The masters of a block into its context -- dm_policy_set_weights with DM_DEVICE_PTRS on views of params at the offsets o of the block's 2 NMAT arrays, the gate's
// included: "packed weights = RNE bf16 of the masters" stays true for every array.  What every optimiser step ends with (train_sgd below, dm_optim.h).
template <int NMAT>
static int train_refresh(dm_policy* net, const long long* o, const float* params, rt_stream stream) {
    const dmp::PolicyDev& d = net->pd;
    dm_policy_params pp; memset(&pp, 0, sizeof(pp));
    pp.state_dim = d.S; pp.hidden1 = d.H1; pp.hidden2 = d.H2; pp.action_dim = d.A;
    dm_policy_gate_params gp; memset(&gp, 0, sizeof(gp));
    if (net->gated) { gp.goal_dim = net->gd.G; gp.gate_common = net->gd.GC; gp.gate_hidden = net->gd.GH; }
    const float** const arr[dmt::GATED_ARRAYS] = {&pp.w1, &pp.b1, &pp.w2, &pp.b2, &pp.w3, &pp.b3, &gp.gc_w, &gp.gc_b, &gp.g0_w, &gp.g0_b, &gp.g0_bias_w, &gp.g0_bias_b, &gp.g0_scale_w, &gp.g0_scale_b,
                                                  &gp.g1_w, &gp.g1_b, &gp.g1_bias_w, &gp.g1_bias_b, &gp.g1_scale_w, &gp.g1_scale_b};
    for (int k = 0; k < 2 * NMAT; ++k) *arr[k] = params + o[k];
    return policy_pack(net, pp, net->gated ? &gp : nullptr, DM_DEVICE_PTRS, stream);
}

// What the plain and the gated step share behind their checks.  o: the offsets of the block's 2 NMAT arrays (a layout's o: array 2 k a matrix, under the weight decay,
// 2 k + 1 its bias vector); null with no context: no matrix, the step alone.  k_train_sgd<NMAT>, then train_refresh
template <int NMAT>
static int train_sgd(dm_policy* net, const long long* o, float* params, float* momentum_dev, const float* grads, int64_t P, double stepsize, double momentum,
                     double weight_decay, double grad_scale, void* hip_stream) {
    dmt::SgdArgs<NMAT> a; memset(&a, 0, sizeof(a));
    if (o) for (int k = 0; k < NMAT; ++k) { a.mat[k][0] = o[2 * k]; a.mat[k][1] = o[2 * k + 1]; }
    a.w = params; a.v = momentum_dev; a.g = grads; a.P = P; a.lr = (float)stepsize; a.mom = (float)momentum; a.wd = (float)weight_decay; a.gs = (float)grad_scale;
    a.blocks = (unsigned)std::min<int64_t>((P + 255) / 256, 4096);
    rt_stream stream = (rt_stream)hip_stream;
    if (!net) {                                   // no context: on the calling thread's current device
        RT_LAUNCH4(dmt::k_train_sgd<NMAT>, a.blocks, stream, a);
        return launch_status(0);
    }
    DevGuard guard(net->device_id);
    RT_LAUNCH4(dmt::k_train_sgd<NMAT>, a.blocks, stream, a);
    if (launch_status(0)) return -1;
    return train_refresh<NMAT>(net, o, params, stream);
}

// what dm_train_read_activations and dm_train_gated_read share behind the check of the net: array `which` of `count` = {source, bytes per row}; `names`: what `which` may be
struct TrainReadRow { const void* src; size_t row_bytes; };
static int train_read(const char* fn, dm_policy* net, const TrainReadRow* table, int count, const char* names, int which, int n, void* host_out, size_t capacity) {
    if (!host_out) return fail(std::string(fn) + ": null argument");
    if (which < 0 || which >= count) return fail(std::string(fn) + ": which must be " + names);
    if (n < 1 || n > net->cap) return fail(std::string(fn) + ": n must be in [1, rows the context holds]");
    const size_t bytes = (size_t)n * table[which].row_bytes;
    if (capacity < bytes) return fail(std::string(fn) + ": the host buffer is smaller than the array (" + std::to_string(bytes) + " bytes)");
    DevGuard guard(net->device_id);
#ifndef DM_EMU
    if (hipDeviceSynchronize() != hipSuccess) return fail("device synchronize failed");
#endif
    return rt_d2h(host_out, table[which].src, bytes, 0) == 0 ? 0 : fail("device to host copy failed");
}

extern "C" {

int64_t dm_train_param_count(const dm_policy* net) {
    if (train_net_ok("dm_train_param_count", net)) return -1;
    return (int64_t)dmt::layout_of(net->pd).P;
}

int64_t dm_train_workspace_bytes(const dm_policy* net, int n) {
    if (train_net_ok("dm_train_workspace_bytes", net)) return -1;
    if (n < 1) { fail("dm_train_workspace_bytes: n must be >= 1"); return -1; }
    return (int64_t)dmt::carve(net->pd, n, nullptr).bytes;
}

int dm_train_actor_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* actions_dev,
                        const float* old_logp_dev, const float* adv_dev, const dm_train_actor_cfg* cfg, float* grads_dev, double* stats_dev, float* logp_out,
                        void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_actor_grad";
    if (train_net_ok(fn, net)) return -1;
    dmt::HeadArgs ha;
    if (train_actor_head(fn, net, n, actions_dev, old_logp_dev, adv_dev, cfg, logp_out, ha)) return -1;
    return train_grad(net, fn, params_dev, states_dev, goals_dev, goal_dim, n, ha, grads_dev, stats_dev, workspace, workspace_bytes, hip_stream);
}

int dm_train_value_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* targets_dev,
                        float* grads_dev, double* stats_dev, float* values_out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_value_grad";
    if (train_net_ok(fn, net)) return -1;
    dmt::HeadArgs ha;
    if (train_value_head(fn, net, targets_dev, values_out, ha)) return -1;
    return train_grad(net, fn, params_dev, states_dev, goals_dev, goal_dim, n, ha, grads_dev, stats_dev, workspace, workspace_bytes, hip_stream);
}

// what the two discriminator entry points refuse alike
static int train_disc_ok(const char* fn, const dm_policy* net, int n_expert, int n_agent) {
    if (train_net_ok(fn, net)) return -1;
    if (net->pd.A != 1) return fail(std::string(fn) + ": the context has action_dim " + std::to_string(net->pd.A) + ", the discriminator is a net with one output");
    if (n_expert < 1 || n_agent < 1) return fail(std::string(fn) + ": n_expert and n_agent must be >= 1");
    return train_rows_ok(fn, net->pd, (long long)n_expert + (long long)n_agent);
}

int64_t dm_train_disc_workspace_bytes(const dm_policy* net, int n_expert, int n_agent) {
    if (train_disc_ok("dm_train_disc_workspace_bytes", net, n_expert, n_agent)) return -1;
    return (int64_t)dmt::carve_disc(net->pd, n_expert, n_agent, nullptr).bytes;
}

int dm_train_disc_grad(dm_policy* net, const float* params_dev, const float* expert_obs_dev, int n_expert, const float* agent_obs_dev, int n_agent,
                       const dm_train_disc_cfg* cfg, float* grads_dev, double* stats_dev, float* logits_out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_disc_grad";
    if (train_disc_ok(fn, net, n_expert, n_agent)) return -1;
    if (!params_dev || !expert_obs_dev || !agent_obs_dev || !cfg || !grads_dev || !stats_dev || !workspace) return fail(std::string(fn) + ": null argument");
    if (!(cfg->grad_penalty >= 0.0 && std::isfinite(cfg->grad_penalty))) return fail(std::string(fn) + ": grad_penalty must be finite and >= 0");
    if (!(cfg->logit_reg >= 0.0 && std::isfinite(cfg->logit_reg))) return fail(std::string(fn) + ": logit_reg must be finite and >= 0");
    dm_policy* p = net;
    const dmp::PolicyDev& d = p->pd;
    const int ne = n_expert, na = n_agent, n = ne + na;
    const dmt::DiscWork k = dmt::carve_disc(d, ne, na, workspace);
    if (train_ws_ok(fn, stats_dev, workspace, workspace_bytes, k.bytes, "dm_train_disc_workspace_bytes")) return -1;
    DevGuard guard(p->device_id);
    rt_stream stream = (rt_stream)hip_stream;
    if (policy_grow(p, n, stream)) return -1;
    const bool penalty = cfg->grad_penalty > 0.0;
    const float c_lr = (float)cfg->logit_reg;
    // ---- forward: the two batches into one s16 (expert rows first), then the layers over all rows
    dmp::PolicyIO io; memset(&io, 0, sizeof(io));
    io.exp_rate = 1.0f; io.h1 = p->h1; io.h2 = p->h2;
    io.states = expert_obs_dev; io.M = ne; io.s16 = p->s16;
    RT_LAUNCH(dmp::k_policy_prep, ne, stream, d, io);
    io.states = agent_obs_dev; io.M = na; io.s16 = p->s16 + (size_t)ne * d.K1;
    RT_LAUNCH(dmp::k_policy_prep, na, stream, d, io);
    train_forward(p, nullptr, nullptr, 0, n, stream);
    const dmt::Layout L = dmt::layout_of(d);
    const int groups = (n + 15) / 16;
    dmt::DiscHeadArgs ha; memset(&ha, 0, sizeof(ha));
    ha.M = n; ha.ne = ne; ha.nef = (float)ne; ha.naf = (float)na; ha.penalty = penalty ? 1 : 0; ha.w3 = params_dev + L.o[4];
    ha.z3 = k.w.z3; ha.dz3 = k.w.dz3; ha.g2 = k.g2; ha.part = k.w.part; ha.out = logits_out;
    RT_LAUNCH(dmt::k_train_disc_head, groups, stream, d, (const uint16_t*)p->h2, ha);
    // ---- the least-squares backward pass over all rows
    TrainBackward{stream, n, params_dev, grads_dev}.plain_backward(p, k.w, L);
    // ---- the penalty, expert rows only
    const int rb = (ne + 31) / 32;
    if (penalty) {
        TrainBackward{stream, ne, params_dev, grads_dev}.dgrad(k.g2, d.H2, L.o[2], d.H2, p->h1, d.H1, k.g1);
        dmt::DgradInArgs d1; d1.dz = k.g1; d1.lddz = d.H1; d1.W = params_dev + L.o[0]; d1.ldw = d.H1; d1.h = nullptr; d1.H = d.K1; d1.M = ne; d1.out = k.a;
        d1.S = d.S; d1.scale = (float)cfg->grad_penalty / (float)ne; d1.sq = k.sq;
        RT_LAUNCH(dmt::k_train_dgrad<true>, rb * (d.K1 / 32), stream, d1);
        dmt::FwdmArgs f1; f1.in = k.a; f1.wp = d.w1p; f1.KS = d.K1 / 32; f1.h = p->h1; f1.N = d.H1; f1.M = ne; f1.out = k.t1;
        RT_LAUNCH(dmt::k_train_fwdm, rb * (d.H1 / 32), stream, f1);
        dmt::FwdmArgs f2; f2.in = k.t1; f2.wp = d.w2p; f2.KS = d.H1 / 32; f2.h = p->h2; f2.N = d.H2; f2.M = ne; f2.out = k.t2;
        RT_LAUNCH(dmt::k_train_fwdm, rb * (d.H2 / 32), stream, f2);
        dmt::WgradArgs w1; w1.in = k.a; w1.ldin = d.K1; w1.K = d.S; w1.dz = k.g1; w1.lddz = d.H1; w1.N = d.H1; w1.M = ne; w1.dW = grads_dev + L.o[0];
        RT_LAUNCH(dmt::k_train_wgrad<true>, ((d.S + 31) / 32) * (d.H1 / 32), stream, w1);
        dmt::WgradArgs w2; w2.in = k.t1; w2.ldin = d.H1; w2.K = d.H1; w2.dz = k.g2; w2.lddz = d.H2; w2.N = d.H2; w2.M = ne; w2.dW = grads_dev + L.o[2];
        RT_LAUNCH(dmt::k_train_wgrad<true>, (d.H1 / 32) * (d.H2 / 32), stream, w2);
    }
    if (penalty || c_lr > 0.0f)
        RT_LAUNCH4(dmt::k_train_bgrad<true>, (d.H2 + 63) / 64, stream, (const uint16_t*)k.t2, d.H2, d.H2, penalty ? ne : 0, grads_dev + L.o[4], c_lr > 0.0f ? params_dev + L.o[4] : (const float*)nullptr, c_lr);
    // ---- the statistics
    const int wblocks = (int)std::min<long long>((L.P + 16383) / 16384, dmt::DISC_WN_BLOCKS);
    RT_LAUNCH4(dmt::k_train_disc_wnorm, wblocks, stream, params_dev, L, wblocks, k.wn);
    dmt::DiscFoldArgs fa; fa.part = k.w.part; fa.groups = groups; fa.sq = k.sq; fa.nsq = penalty ? (long long)ne * (d.K1 / 32) : 0; fa.wn = k.wn; fa.wblocks = wblocks;
    fa.ne = ne; fa.na = na; fa.stats = stats_dev;
    RT_LAUNCH4(dmt::k_train_disc_fold, 1, stream, fa);
    return launch_status(0);
}

int dm_train_sgd_step(dm_policy* net, float* params_dev, float* momentum_dev, const float* grads_dev, int64_t P, double stepsize, double momentum, double weight_decay,
                      double grad_scale, void* hip_stream) {
    const char* fn = "dm_train_sgd_step";
    if (net && train_net_ok(fn, net)) return -1;
    if (train_step_ok(fn, params_dev, momentum_dev, grads_dev, P, stepsize, momentum, weight_decay, grad_scale)) return -1;
    dmt::Layout L; memset(&L, 0, sizeof(L));
    if (net) {
        L = dmt::layout_of(net->pd);
        if (P != L.P) return fail(std::string(fn) + ": P is " + std::to_string((long long)P) + ", the net has " + std::to_string(L.P) + " parameters (dm_train_param_count)");
    } else if (weight_decay != 0.0) return fail(std::string(fn) + ": weight_decay needs the net (which entries are matrices is its layout)");
    return train_sgd<3>(net, net ? L.o : nullptr, params_dev, momentum_dev, grads_dev, P, stepsize, momentum, weight_decay, grad_scale, hip_stream);
}

int dm_train_read_activations(dm_policy* net, int which, int n, void* host_out, size_t capacity) {
    const char* fn = "dm_train_read_activations";
    if (train_net_ok(fn, net)) return -1;
    const dmp::PolicyDev& d = net->pd;
    const TrainReadRow table[3] = {{net->s16, (size_t)d.K1 * 2}, {net->h1, (size_t)d.H1 * 2}, {net->h2, (size_t)d.H2 * 2}};
    return train_read(fn, net, table, 3, "0 (s16), 1 (h1) or 2 (h2)", which, n, host_out, capacity);
}

}  // extern "C"
