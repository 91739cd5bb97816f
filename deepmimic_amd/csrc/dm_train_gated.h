// The PPO actor and critic minibatch updates for the GATED nets of the AMP task agents (include/dm_hip.h dm_train_gated_*, deepmimic_amd/train.py GatedActorTrainer /
// GatedCriticTrainer): fc_2layers_gated_1024units as "ActorNet" and "CriticNet" of ct_agent_humanoid_amp_tasks*.txt, trained on the context that samples.  Included at the
// end of dm_host.cpp behind dm_train.h, whose head, fold, wgrad / bgrad / dgrad and step kernels, tile toolkit, checks, forward (train_forward), backward launcher
// (TrainBackward), step (train_sgd<GATED_MATRICES>) and read (train_read) it uses unchanged; in no step-kernel translation unit.
//
// Notation (dm_policy.h GateDev; i = 0: layer 1, width H1, i = 1: layer 2, width H2): c = relu(Wc xg + bc), e_i = relu(We_i c + be_i), beta_i = Wb_i e_i + bb_i,
// sigma_i = 2 sigmoid(Ws_i e_i + bs_i), u_i = W_i h_(i-1) + b_i, p_i = fmaf(sigma_i, u_i, beta_i), h_i = bf16(relu(p_i)).
// One *_grad call is, in stream order:
//     k_policy_prep, k_policy_gate, the GATED layers 1 and 2      the context's own per-layer route (forced), leaving s16 / h1 / h2 in bf16 and sigma_i / beta_i in fp32 (gbuf)
//     k_train_gate_hidden          xg, c, e_0, e_1 once more through dmp::gate_hidden (the forward keeps them in LDS only) -> row-major bf16 in the workspace
//     k_train_head, k_train_fold   unchanged; then wgrad / bgrad / dgrad of layer 3: dp_1 = bf16((dz3 W3^T) . [h2 != 0])
//     per hidden layer, 2 then 1:  k_train_gate_split (du_i, da_i from dp_i), wgrad / bgrad from du_i, and for layer 2 k_train_dgrad from du_1 -> dp_0
//     per gate i:                  wgrad / bgrad on e_i from dp_i (Wb_i, bb_i) and from da_i (Ws_i, bs_i), k_train_dgrad2 -> dze_i, wgrad / bgrad on c from dze_i (We_i, be_i)
//     k_train_dgrad2 -> dzc, wgrad / bgrad on xg from dzc (Wc, bc)
// Every gradient element has one owner and one contraction from a zero accumulator, k-steps ascending: no partial, no atomic, two calls on one input give the same bytes.
#pragma once

namespace dmt {

// the element of row m (of the workgroup's 32), feature k in the B-fragment order [k-step][batch tile][lane][8] of dm_policy.h gate_store: 8 consecutive k share a record
DMP_DEV size_t gate_record(int k, int m) { return (size_t)((k >> 5) * 2 + (m >> 4)) * 64 + (m & 15) + 16 * ((k & 31) >> 3); }

// one such LDS array of `width` features -> rows row0 .. of a row-major [M x width] bf16 array: a 16-byte record per store
DMP_DEV void gate_rows_out(const bf16x8* src, int width, int row0, int M, uint16_t* out, int t) {
    for (int idx = t; idx < 4 * width; idx += 256) {
        const int m = idx & 31, k0 = (idx >> 5) * 8;
        if (row0 + m < M) *reinterpret_cast<bf16x8*>(out + (size_t)(row0 + m) * width + k0) = src[gate_record(k0, m)];
    }
}

// The gate's hidden activations of 32 rows as k_policy_gate forms them -- its staging of the goal block, then dmp::gate_hidden: the same function, hence the same bits --
// written out: xg [M x KG] (padding columns zero), c [M x GC], e_0, e_1 [M x GH].  Four wavefronts, every wave the same number of MFMA trips (gate_hidden).
__global__ void __launch_bounds__(256) k_train_gate_hidden(dmp::PolicyDev p, const uint16_t* s16, int M, dmp::GateDev gd, uint16_t* xg, uint16_t* c_out, uint16_t* e0, uint16_t* e1) {
    __shared__ bf16x8 sx[4 * 2 * 64], sc[8 * 2 * 64], se[2][4 * 2 * 64];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, c = l & 15, g = l >> 4;
    const int row0 = (int)blockIdx.x * 32;
    {
        uint16_t* const sxh = reinterpret_cast<uint16_t*>(sx);
        const int m = t & 31, row = row0 + m < M ? row0 + m : M - 1;
        const uint16_t* const src = s16 + (size_t)row * p.K1 + (p.S - gd.G);
        for (int k = t >> 5; k < gd.KG; k += 8) sxh[gate_record(k, m) * 8 + (k & 7)] = k < gd.G ? src[k] : (uint16_t)0;
    }
    __syncthreads();
    dmp::gate_hidden(gd, sx, sc, se[0], w, l, c, g);
    gate_rows_out(sx, gd.KG, row0, M, xg, t);
    gate_rows_out(sc, gd.GC, row0, M, c_out, t);
    gate_rows_out(se[0], gd.GH, row0, M, e0, t);
    gate_rows_out(se[1], gd.GH, row0, M, e1, t);
}

// in [M x 32 KS], wp: the packed fragments of W [32 KS x N], bias [N], sig fp32 and dp bf16 [M x N] -> du, da bf16 [M x N]
struct SplitArgs { const uint16_t* in; const uint16_t* wp; int KS; const float* bias; const float* sig; const uint16_t* dp; int N, M; uint16_t *du, *da; };

// The gate split of one hidden layer: p = fmaf(sigma, u, beta) sends dp to u (du = dp sigma), to beta (dp itself) and to sigma's pre-activation z (da = dp u dsigma/dz,
// dsigma/dz = sigma (1 - sigma / 2) for sigma = 2 sigmoid(z)).  u is not stored by the forward: acc is recomputed by tile_chain_packed, the chain of k_train_fwdm (the packed B fragments,
// k-steps ascending from a zero accumulator: the chain of k_policy_layer / k_policy_gemm), so u = acc + b has the bits the forward had.  Per element in fp32, one rounding
// per written operation; the ReLU mask is already inside dp; sigma = 0 and sigma = 2 give da = 0 (times dp u); a NaN propagates.  A wavefront owns 32 rows x 32 columns.
__global__ void __launch_bounds__(64) k_train_gate_split(SplitArgs a) {
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int rbn = (a.M + 31) / 32, m0 = ((int)blockIdx.x % rbn) * 32, n0 = ((int)blockIdx.x / rbn) * 32;      // consecutive workgroups walk down the rows under one block of W
    f32x4 acc[2][2];
    tile_zero(acc);
    tile_chain_packed(acc, a.in, a.wp, a.KS, a.M, m0, n0, l, c, g);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + 16 * j + c; const float b = a.bias[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + 16 * i + 4 * g + r;
                if (row >= a.M) continue;
                const size_t at = (size_t)row * a.N + col;
                const float sg = a.sig[at], dp = bf16_f32(a.dp[at]), u = acc[i][j][r] + b;
                const float ds = sg * fmaf(-0.5f, sg, 1.0f);
                a.du[at] = bf16_rne(dp * sg);
                a.da[at] = bf16_rne((dp * u) * ds);
            }
    }
}

// dz[p] [M x ld] bf16, W[p] [H x ld] fp32 masters (p = 0, 1), h / out [M x H]
struct Dgrad2Args { const uint16_t* dz[2]; const float* W[2]; int ld; const uint16_t* h; int H, M; uint16_t* out; };

// The two-pair form of k_train_dgrad<false>: out = bf16((dz_0 W_0^T + dz_1 W_1^T) . [h != 0]) with ONE accumulator started at zero, the k-steps of pair 0 ascending, then
// those of pair 1; B operands the RNE bf16 of the masters, converted on load.  A wavefront owns 32 rows x 32 columns.  (The gate's hidden units feed two projections each:
// e_i the beta and the sigma projection, c the two e_i.)
__global__ void __launch_bounds__(64) k_train_dgrad2(Dgrad2Args a) {
    const int l = (int)threadIdx.x, c = l & 15, g = l >> 4;
    const int rbn = (a.M + 31) / 32, m0 = ((int)blockIdx.x % rbn) * 32, k0 = ((int)blockIdx.x / rbn) * 32;
    f32x4 acc[2][2];
    tile_zero(acc);
    for (int p = 0; p < 2; ++p) {
        const uint16_t* arow[2]; const float* wrow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = m0 + 16 * i + c;
            arow[i] = a.dz[p] + (size_t)(row < a.M ? row : 0) * a.ld + 8 * g;
            wrow[i] = a.W[p] + (size_t)(k0 + 16 * i + c) * a.ld + 8 * g;
        }
        // the operands of four k-steps are requested in one batch (one memory latency per four: with 2 n / 32 workgroups of one wave the kernel's time is all latency),
        // then multiplied in k order
        const int KS = a.ld / 32;
        for (int ks0 = 0; ks0 < KS; ks0 += 4) {
            bf16x8 fa[4][2]; float wf[4][2][8];
            DMP_SCHED_FENCE();                               // (fenced: left alone, the scheduler sinks every request to just in front of its MFMA to save registers)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int nk = 32 * (ks0 + u < KS ? ks0 + u : KS - 1);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[u][i] = *reinterpret_cast<const bf16x8*>(arow[i] + nk);
#pragma unroll
                    for (int e = 0; e < 8; ++e) wf[u][i][e] = wrow[i][nk + e];
                }
            }
            DMP_SCHED_FENCE();
#pragma unroll
            for (int u = 0; u < 4; ++u) if (ks0 + u < KS) {
                bf16x8 fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) dmp::set8(fb[i], e, bf16_rne(wf[u][i][e]));
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(fa[u][i], fb[j], acc[i][j]);
            }
        }
    }
    tile_store_masked(acc, a.h, a.out, a.H, a.M, m0, k0, c, g);
}

// offsets (in floats) of the GATED_ARRAYS = 20 arrays of a gated parameter block -- the six of Layout, then the gate's in the order of dm_policy_gate_params -- and its length;
// array 2 k is a matrix, 2 k + 1 its bias vector
struct GatedLayout { long long o[GATED_ARRAYS], P; };
inline GatedLayout gated_layout_of(const dmp::PolicyDev& d, const dmp::GateDev& q) {
    const long long S = d.S, H1 = d.H1, H2 = d.H2, A = d.A, G = q.G, GC = q.GC, GH = q.GH;
    const long long count[GATED_ARRAYS] = {S * H1, H1, H1 * H2, H2, H2 * A, A, G * GC, GC, GC * GH, GH, GH * H1, H1, GH * H1, H1, GC * GH, GH, GH * H2, H2, GH * H2, H2};
    GatedLayout L; long long at = 0;
    for (int k = 0; k < GATED_ARRAYS; ++k) { L.o[k] = at; at += count[k]; }
    L.P = at;
    return L;
}

// the caller's workspace: the five pieces of `carve` (its dz2 / dz1 slots hold dp_1 / dp_0), then, all bf16 and each starting on a multiple of 16 bytes,
// [du_1 n x H2][du_0 n x H1][da_1 n x H2][da_0 n x H1][xg n x KG][c n x GC][e_0 n x GH][e_1 n x GH][dze_0 n x GH][dze_1 n x GH][dzc n x GC]
struct GatedWork { Work w; uint16_t *du[2], *da[2], *xg, *c, *e[2], *dze[2], *dzc; size_t bytes; };
inline GatedWork carve_gated(const dmp::PolicyDev& d, const dmp::GateDev& q, int n, void* ws) {
    GatedWork k; k.w = carve(d, n, ws);
    char* at = (char*)ws + k.w.bytes;
    auto piece = [&](int width) { uint16_t* p = (uint16_t*)at; at += ((size_t)n * width * 2 + 15) / 16 * 16; return p; };
    k.du[1] = piece(d.H2); k.du[0] = piece(d.H1); k.da[1] = piece(d.H2); k.da[0] = piece(d.H1);
    k.xg = piece(q.KG); k.c = piece(q.GC); k.e[0] = piece(q.GH); k.e[1] = piece(q.GH); k.dze[0] = piece(q.GH); k.dze[1] = piece(q.GH); k.dzc = piece(q.GC);
    k.bytes = (size_t)(at - (char*)ws);
    return k;
}

}  // namespace dmt

static int train_gated_ok(const char* fn, const dm_policy* p) {
    if (!p) return fail(std::string(fn) + ": null net");
    if (!p->gated) return fail(std::string(fn) + ": a plain context (dm_policy_create) is not trained here: the gated nets only (a plain net: dm_train_*)");
    return 0;
}

// what the two gated *_grad calls share behind their own checks
static int train_gated_grad(dm_policy* p, const char* fn, const float* params, const float* states, const float* goals, int goal_dim, int n, dmt::HeadArgs& ha, float* grads,
                            double* stats, void* ws, int64_t ws_bytes, void* hip_stream) {
    const dmp::PolicyDev& d = p->pd; const dmp::GateDev& q = p->gd;
    const dmt::GatedWork k = dmt::carve_gated(d, q, n, ws);
    if (train_args_ok(p, fn, params, states, goals, goal_dim, n, grads, stats, ws, ws_bytes, k.bytes, "dm_train_gated_workspace_bytes")) return -1;
    DevGuard guard(p->device_id);
    rt_stream stream = (rt_stream)hip_stream;
    if (policy_grow(p, n, stream)) return -1;
    train_forward(p, states, goals, goal_dim, n, stream);
    const int rb = (n + 31) / 32;
    RT_LAUNCH4(dmt::k_train_gate_hidden, rb, stream, d, (const uint16_t*)p->s16, n, q, k.xg, k.c, k.e[0], k.e[1]);
    train_head(p, n, ha, k.w, stats, stream);
    // ---- backward; o[a]: the offset of array `a` of the block (GatedLayout: a matrix and, behind it, its bias vector)
    const dmt::GatedLayout L = dmt::gated_layout_of(d, q);
    const long long* const o = L.o;
    const TrainBackward bw{stream, n, params, grads};
    auto split = [&](const uint16_t* in, const uint16_t* wp, int K, const float* bias, const float* sig, int N, int i) {
        dmt::SplitArgs sa; sa.in = in; sa.wp = wp; sa.KS = K / 32; sa.bias = bias; sa.sig = sig; sa.dp = i ? k.w.dz2 : k.w.dz1; sa.N = N; sa.M = n; sa.du = k.du[i]; sa.da = k.da[i];
        RT_LAUNCH(dmt::k_train_gate_split, rb * (N / 32), stream, sa);
    };
    auto dgrad2 = [&](const uint16_t* dz0, int arr0, const uint16_t* dz1, int arr1, int ld, const uint16_t* h, int H, uint16_t* out) {
        dmt::Dgrad2Args da; da.dz[0] = dz0; da.dz[1] = dz1; da.W[0] = params + o[arr0]; da.W[1] = params + o[arr1]; da.ld = ld; da.h = h; da.H = H; da.M = n; da.out = out;
        RT_LAUNCH(dmt::k_train_dgrad2, rb * (H / 32), stream, da);
    };
    bw.wgrad_bgrad(p->h2, d.H2, d.H2, k.w.dz3, d.N3, d.A, o[4], o[5]);
    bw.dgrad(k.w.dz3, d.N3, o[4], d.A, p->h2, d.H2, k.w.dz2);                         // dp_1
    split(p->h1, d.w2p, d.H1, d.b2, p->gbuf[2], d.H2, 1);
    bw.wgrad_bgrad(p->h1, d.H1, d.H1, k.du[1], d.H2, d.H2, o[2], o[3]);
    bw.dgrad(k.du[1], d.H2, o[2], d.H2, p->h1, d.H1, k.w.dz1);                        // dp_0
    split(p->s16, d.w1p, d.K1, d.b1, p->gbuf[0], d.H1, 0);
    bw.wgrad_bgrad(p->s16, d.K1, d.S, k.du[0], d.H1, d.H1, o[0], o[1]);
    for (int i = 0; i < 2; ++i) {
        const int H = i ? d.H2 : d.H1, base = 8 + 6 * i;                              // We_i, be_i, Wb_i, bb_i, Ws_i, bs_i
        const uint16_t* const dp = i ? k.w.dz2 : k.w.dz1;
        bw.wgrad_bgrad(k.e[i], q.GH, q.GH, dp, H, H, o[base + 2], o[base + 3]);
        bw.wgrad_bgrad(k.e[i], q.GH, q.GH, k.da[i], H, H, o[base + 4], o[base + 5]);
        dgrad2(dp, base + 2, k.da[i], base + 4, H, k.e[i], q.GH, k.dze[i]);
        bw.wgrad_bgrad(k.c, q.GC, q.GC, k.dze[i], q.GH, q.GH, o[base], o[base + 1]);
    }
    dgrad2(k.dze[0], 8, k.dze[1], 14, q.GH, k.c, q.GC, k.dzc);
    bw.wgrad_bgrad(k.xg, q.KG, q.G, k.dzc, q.GC, q.GC, o[6], o[7]);
    return launch_status(0);
}

extern "C" {

int64_t dm_train_gated_param_count(const dm_policy* net) {
    if (train_gated_ok("dm_train_gated_param_count", net)) return -1;
    return (int64_t)dmt::gated_layout_of(net->pd, net->gd).P;
}

int64_t dm_train_gated_workspace_bytes(const dm_policy* net, int n) {
    if (train_gated_ok("dm_train_gated_workspace_bytes", net)) return -1;
    if (n < 1) { fail("dm_train_gated_workspace_bytes: n must be >= 1"); return -1; }
    return (int64_t)dmt::carve_gated(net->pd, net->gd, n, nullptr).bytes;
}

int dm_train_gated_actor_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* actions_dev,
                              const float* old_logp_dev, const float* adv_dev, const dm_train_actor_cfg* cfg, float* grads_dev, double* stats_dev, float* logp_out,
                              void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_gated_actor_grad";
    if (train_gated_ok(fn, net)) return -1;
    dmt::HeadArgs ha;
    if (train_actor_head(fn, net, n, actions_dev, old_logp_dev, adv_dev, cfg, logp_out, ha)) return -1;
    return train_gated_grad(net, fn, params_dev, states_dev, goals_dev, goal_dim, n, ha, grads_dev, stats_dev, workspace, workspace_bytes, hip_stream);
}

int dm_train_gated_value_grad(dm_policy* net, const float* params_dev, const float* states_dev, const float* goals_dev, int goal_dim, int n, const float* targets_dev,
                              float* grads_dev, double* stats_dev, float* values_out, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_gated_value_grad";
    if (train_gated_ok(fn, net)) return -1;
    dmt::HeadArgs ha;
    if (train_value_head(fn, net, targets_dev, values_out, ha)) return -1;
    return train_gated_grad(net, fn, params_dev, states_dev, goals_dev, goal_dim, n, ha, grads_dev, stats_dev, workspace, workspace_bytes, hip_stream);
}

int dm_train_gated_sgd_step(dm_policy* net, float* params_dev, float* momentum_dev, const float* grads_dev, int64_t P, double stepsize, double momentum, double weight_decay,
                            double grad_scale, void* hip_stream) {
    const char* fn = "dm_train_gated_sgd_step";
    if (train_gated_ok(fn, net)) return -1;
    if (train_step_ok(fn, params_dev, momentum_dev, grads_dev, P, stepsize, momentum, weight_decay, grad_scale)) return -1;
    const dmt::GatedLayout L = dmt::gated_layout_of(net->pd, net->gd);
    if (P != L.P) return fail(std::string(fn) + ": P is " + std::to_string((long long)P) + ", the net has " + std::to_string(L.P) + " parameters (dm_train_gated_param_count)");
    return train_sgd<dmt::GATED_MATRICES>(net, L.o, params_dev, momentum_dev, grads_dev, P, stepsize, momentum, weight_decay, grad_scale, hip_stream);
}

int dm_train_gated_read(dm_policy* net, int which, int n, void* host_out, size_t capacity) {
    const char* fn = "dm_train_gated_read";
    if (train_gated_ok(fn, net)) return -1;
    const dmp::PolicyDev& d = net->pd;
    const TrainReadRow table[7] = {{net->s16, (size_t)d.K1 * 2}, {net->h1, (size_t)d.H1 * 2}, {net->h2, (size_t)d.H2 * 2}, {net->gbuf[0], (size_t)d.H1 * 4}, {net->gbuf[1], (size_t)d.H1 * 4},
                                   {net->gbuf[2], (size_t)d.H2 * 4}, {net->gbuf[3], (size_t)d.H2 * 4}};
    return train_read(fn, net, table, 7, "0 (s16), 1 (h1), 2 (h2) or 3 .. 6 (sigma_0, beta_0, sigma_1, beta_1)", which, n, host_out, capacity);
}

}  // extern "C"
