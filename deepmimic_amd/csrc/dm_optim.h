// The optimiser step of the device trainers with Adam, global-norm gradient clipping and a non-finite guard (dm_train_opt_step): what ends a minibatch of a learner that
// has left the reference's batch size -- tf.train.MomentumOptimizer (k_train_sgd's statement) or Adam on the fp32 masters, the gradient scaled as
// torch.nn.utils.clip_grad_norm_ scales it, and a step that does not happen when a gradient element is not finite -- with every decision in device scalars: nothing is
// read on the host.  Included at the end of dm_host.cpp behind dm_train_gated.h (its layouts, train_refresh; dm_ppo_batch.h: the tree).  The contract is in
// include/dm_hip.h, the same arithmetic in numpy in deepmimic_amd/train.py (reference_grad_norm, reference_opt_begin, reference_adam_step).
//
// One call is at most three launches and the refresh, ordered by the stream alone (no workgroup waits on another one, no atomics):
//     k_opt_sq     only with clipping or the guard.  Workgroup b owns the kChunk elements from b kChunk; thread t takes b kChunk + t + 256 k, k = 0 .. kPer - 1, in that
//                  order (coalesced across the threads, kPer independent loads in flight per thread): the fp64 sum of its squares and the number of its non-finite
//                  elements; the 256 threads by the tree of dmb::block_sum; one partial {sum, count} per group, both doubles (a count is exact in one).
//     k_opt_begin  one workgroup: the partials by dmb::fold_groups (contiguous runs per thread, the tree), norm = |grad_scale| sqrt(sum), scale = min(1, max_grad_norm /
//                  (norm + 1e-6)) (a NaN stays one, as np.minimum keeps it), skip = guard && count > 0; unless skip t += 1 and the running powers of beta1 and beta2
//                  take one more factor; the state, and the control record of the step: {skip, s = float(grad_scale scale), alpha_t = stepsize / (1 - beta1^t),
//                  ic2 = 1 / (1 - beta2^t)}.  Without k_opt_sq: sum = count = 0, scale = 1.
//     k_opt_step   a grid-stride loop over P shaped like k_train_sgd: returns without a store when skip is set; else MOMENTUM -- k_train_sgd's statement with s in place
//                  of gs -- or ADAM.  No product is contracted into a sum (not every product here is one of two floats): every written operation rounds once in fp64,
//                  m', v' and w' are each rounded once to fp32.
// Traffic: 4 bytes per element for the norm, 16 (MOMENTUM) or 28 (ADAM) for the step: memory-bound and, at the sizes of the reference's nets, launch-bound.
#pragma once

namespace dmo {

constexpr int kThreads = dmb::kThreads;
constexpr int kPer = 4;                          // elements per thread of k_opt_sq
constexpr int kChunk = kThreads * kPer;          // elements per workgroup = per partial
constexpr int kCtrlBytes = 32;                   // the control record at the head of the workspace, then [sum G doubles][count G doubles]
constexpr long long kMaxP = 1LL << 40;           // (the group count stays an int)
enum { ST_T = 0, ST_POW1 = 1, ST_POW2 = 2, ST_SKIPPED = 3, ST_NORM = 4, ST_SCALE = 5, ST_NONFINITE = 6, ST_WORDS = 8 };

struct Ctrl { int skip; float s; double alpha, ic2; };
static_assert(sizeof(Ctrl) <= kCtrlBytes, "the control record");
struct Work { Ctrl* ctrl; double* sum; double* cnt; };
inline int groups_of(long long P) { return (int)((P + kChunk - 1) / kChunk); }
inline Work carve(void* ws, int groups) {
    Work w; w.ctrl = (Ctrl*)ws; w.sum = (double*)((char*)ws + kCtrlBytes); w.cnt = w.sum + groups;
    return w;
}

struct SqArgs { const float* g; long long P; Work w; };

__global__ void __launch_bounds__(256) k_opt_sq(SqArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[kThreads];
    const long long i0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x;
    float x[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) { const long long i = i0 + (long long)k * kThreads; x[k] = i < a.P ? a.g[i] : 0.0f; }
    double s = 0.0, bad = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const double d = (double)x[k];
        s += d * d;
        if (!(fabsf(x[k]) <= 3.402823466e+38f)) bad += 1.0;          // NaN or +-inf
    }
    const double sum = dmb::block_sum(s, red);
    const double cnt = dmb::block_sum(bad, red);
    if (threadIdx.x == 0) { a.w.sum[blockIdx.x] = sum; a.w.cnt[blockIdx.x] = cnt; }
}

struct BeginArgs {
    Work w; int groups;
    int measured, clip, guard, adam;             // measured: k_opt_sq ran
    double max_norm, grad_scale, B1, B2, stepsize;
    double* state;
};

__global__ void __launch_bounds__(256) k_opt_begin(BeginArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[kThreads];
    double sum = 0.0, cnt = 0.0;
    if (a.measured) { sum = dmb::fold_groups(a.w.sum, a.groups, red); cnt = dmb::fold_groups(a.w.cnt, a.groups, red); }
    if (threadIdx.x != 0) return;
    const double norm = fabs(a.grad_scale) * sqrt(sum);
    double scale = 1.0;
    if (a.clip) { const double q = a.max_norm / (norm + 1e-6); scale = (q < 1.0 || q != q) ? q : 1.0; }
    const bool skip = a.guard && cnt > 0.0;
    double t = a.state[ST_T];
    double p1 = t == 0.0 ? 1.0 : a.state[ST_POW1], p2 = t == 0.0 ? 1.0 : a.state[ST_POW2];
    if (skip) a.state[ST_SKIPPED] += 1.0;
    else {
        t += 1.0; p1 *= a.B1; p2 *= a.B2;
        a.state[ST_T] = t; a.state[ST_POW1] = p1; a.state[ST_POW2] = p2;
    }
    a.state[ST_NORM] = norm; a.state[ST_SCALE] = scale; a.state[ST_NONFINITE] = cnt;
    Ctrl c;
    c.skip = skip ? 1 : 0;
    c.s = (float)(a.grad_scale * scale);
    c.alpha = a.adam ? a.stepsize / (1.0 - p1) : 0.0;
    c.ic2 = a.adam ? 1.0 / (1.0 - p2) : 0.0;
    *a.w.ctrl = c;
}

// mat: the matrix ranges of the block as in SgdArgs.  MOMENTUM reads lr, mom; ADAM B1, B2 and their complements C1 = 1 - B1, C2 = 1 - B2 (fp64, exact), eps
template <int NMAT> struct StepArgs {
    float* w; float* m; float* v; const float* g; const Ctrl* ctrl;
    long long P, mat[NMAT][2];
    float lr, mom, wd; double B1, C1, B2, C2, eps; unsigned blocks;
};

template <int KIND, int NMAT>
__global__ void __launch_bounds__(256) k_opt_step(StepArgs<NMAT> a) {
#pragma clang fp contract(off)
    const Ctrl c = *a.ctrl;
    if (c.skip) return;
    for (long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x; i < a.P; i += (long long)a.blocks * 256) {
        const float w = a.w[i];
        double gg = (double)c.s * (double)a.g[i];
        bool matrix = false;
        if constexpr (NMAT == 3) matrix = (i >= a.mat[0][0] && i < a.mat[0][1]) || (i >= a.mat[1][0] && i < a.mat[1][1]) || (i >= a.mat[2][0] && i < a.mat[2][1]);
        else for (int k = 0; k < NMAT; ++k) matrix = matrix || (i >= a.mat[k][0] && i < a.mat[k][1]);
        if (matrix) gg += (double)a.wd * (double)w;          // L2 on the matrices, added to the gradient; the biases are exempt
        if constexpr (KIND == DM_OPT_MOMENTUM) {
            const float vv = (float)((double)a.mom * (double)a.m[i] + gg);
            a.m[i] = vv;
            a.w[i] = fmaf(-a.lr, vv, w);
        } else {
            const float m1 = (float)(a.B1 * (double)a.m[i] + a.C1 * gg);
            const float v1 = (float)(a.B2 * (double)a.v[i] + a.C2 * gg * gg);
            a.m[i] = m1; a.v[i] = v1;
            a.w[i] = (float)((double)w - c.alpha * (double)m1 / (sqrt((double)v1 * c.ic2) + a.eps));
        }
    }
}

}  // namespace dmo

// k_opt_sq (with clipping or the guard), k_opt_begin, k_opt_step<KIND, NMAT>, then with a net train_refresh<NMAT>.  o: as in train_sgd
template <int NMAT>
static int train_opt(dm_policy* net, const long long* o, const dm_train_opt_cfg& cfg, float* params, float* m, float* v, const float* grads, int64_t P, double* state,
                     void* ws, rt_stream stream) {
    const bool clip = cfg.max_grad_norm > 0.0 && std::isfinite(cfg.max_grad_norm), guard = cfg.skip_nonfinite != 0, adam = cfg.kind == DM_OPT_ADAM;
    const int groups = dmo::groups_of(P);
    const dmo::Work w = dmo::carve(ws, groups);
    if (clip || guard) {
        dmo::SqArgs sa; sa.g = grads; sa.P = P; sa.w = w;
        RT_LAUNCH4(dmo::k_opt_sq, groups, stream, sa);
    }
    const double B1 = (double)(float)cfg.beta1, B2 = (double)(float)cfg.beta2;
    dmo::BeginArgs ba; memset(&ba, 0, sizeof(ba));
    ba.w = w; ba.groups = groups; ba.measured = (clip || guard) ? 1 : 0; ba.clip = clip ? 1 : 0; ba.guard = guard ? 1 : 0; ba.adam = adam ? 1 : 0;
    ba.max_norm = cfg.max_grad_norm; ba.grad_scale = cfg.grad_scale; ba.B1 = B1; ba.B2 = B2; ba.stepsize = cfg.stepsize; ba.state = state;
    RT_LAUNCH4(dmo::k_opt_begin, 1, stream, ba);
    dmo::StepArgs<NMAT> a; memset(&a, 0, sizeof(a));
    if (o) for (int k = 0; k < NMAT; ++k) { a.mat[k][0] = o[2 * k]; a.mat[k][1] = o[2 * k + 1]; }
    a.w = params; a.m = m; a.v = v; a.g = grads; a.ctrl = w.ctrl; a.P = P;
    a.lr = (float)cfg.stepsize; a.mom = (float)cfg.beta1; a.wd = (float)cfg.weight_decay;
    a.B1 = B1; a.C1 = 1.0 - B1; a.B2 = B2; a.C2 = 1.0 - B2; a.eps = (double)(float)cfg.eps;
    a.blocks = (unsigned)std::min<int64_t>((P + 255) / 256, 4096);
    if (adam) RT_LAUNCH4((dmo::k_opt_step<DM_OPT_ADAM, NMAT>), a.blocks, stream, a);
    else RT_LAUNCH4((dmo::k_opt_step<DM_OPT_MOMENTUM, NMAT>), a.blocks, stream, a);
    if (launch_status(0)) return -1;
    return net ? train_refresh<NMAT>(net, o, params, stream) : 0;
}

extern "C" {

int64_t dm_train_opt_workspace_bytes(int64_t P) {
    if (P < 1 || P > dmo::kMaxP) { fail("dm_train_opt_workspace_bytes: P must be in [1, 2^40]"); return -1; }
    return (int64_t)dmo::kCtrlBytes + (int64_t)dmo::groups_of(P) * 16;
}

int dm_train_opt_step(dm_policy* net, const dm_train_opt_cfg* cfg, float* params_dev, float* m_dev, float* v_dev, const float* grads_dev, int64_t P, double* state_dev,
                      void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const char* fn = "dm_train_opt_step";
    if (!cfg || !params_dev || !m_dev || !grads_dev || !state_dev || !workspace) return fail(std::string(fn) + ": null argument (only net, and v_dev of MOMENTUM, may be NULL)");
    if (cfg->kind != DM_OPT_MOMENTUM && cfg->kind != DM_OPT_ADAM) return fail(std::string(fn) + ": kind must be DM_OPT_MOMENTUM or DM_OPT_ADAM");
    if (cfg->kind == DM_OPT_ADAM) {
        if (!v_dev) return fail(std::string(fn) + ": ADAM needs v_dev");
        // (the float the kernels use: a beta that rounds to 1 would divide by zero in the first step)
        if (!((float)cfg->beta1 >= 0.0f && (float)cfg->beta1 < 1.0f && (float)cfg->beta2 >= 0.0f && (float)cfg->beta2 < 1.0f)) return fail(std::string(fn) + ": beta1 and beta2 must be in [0, 1)");
        if (!((float)cfg->eps > 0.0f && std::isfinite((float)cfg->eps))) return fail(std::string(fn) + ": eps must be finite and > 0 (as a float)");
    } else if (!(cfg->beta1 >= 0.0 && std::isfinite(cfg->beta1))) return fail(std::string(fn) + ": momentum must be finite and >= 0");
    if (!(cfg->stepsize >= 0.0 && std::isfinite(cfg->stepsize))) return fail(std::string(fn) + ": stepsize must be finite and >= 0");
    if (!(cfg->weight_decay >= 0.0 && std::isfinite(cfg->weight_decay))) return fail(std::string(fn) + ": weight_decay must be finite and >= 0");
    if (!std::isfinite(cfg->grad_scale)) return fail(std::string(fn) + ": grad_scale must be finite");
    if (cfg->max_grad_norm != cfg->max_grad_norm) return fail(std::string(fn) + ": max_grad_norm must not be NaN (<= 0 or +inf: no clipping)");
    if (P < 1 || P > dmo::kMaxP) return fail(std::string(fn) + ": P must be in [1, 2^40]");
    dmt::GatedLayout L; memset(&L, 0, sizeof(L));
    if (net) {
        const char* counter = net->gated ? "dm_train_gated_param_count" : "dm_train_param_count";
        if (net->gated) L = dmt::gated_layout_of(net->pd, net->gd);
        else { const dmt::Layout l = dmt::layout_of(net->pd); for (int k = 0; k < 6; ++k) L.o[k] = l.o[k]; L.P = l.P; }
        if (P != L.P) return fail(std::string(fn) + ": P is " + std::to_string((long long)P) + ", the net has " + std::to_string(L.P) + " parameters (" + counter + ")");
    } else if (cfg->weight_decay != 0.0) return fail(std::string(fn) + ": weight_decay needs the net (which entries are matrices is its layout)");
    if ((((uintptr_t)state_dev) & 7) != 0) return fail(std::string(fn) + ": state must be 8-byte aligned");
    if (workspace_bytes < dm_train_opt_workspace_bytes(P)) return fail(std::string(fn) + ": workspace too small (dm_train_opt_workspace_bytes)");
    if ((((uintptr_t)workspace) & 15) != 0) return fail(std::string(fn) + ": the workspace must be 16-byte aligned");
    rt_stream stream = (rt_stream)hip_stream;
    if (!net) return train_opt<3>(nullptr, nullptr, *cfg, params_dev, m_dev, v_dev, grads_dev, P, state_dev, workspace, stream);      // on the calling thread's current device
    DevGuard guard(net->device_id);
    if (net->gated) return train_opt<dmt::GATED_MATRICES>(net, L.o, *cfg, params_dev, m_dev, v_dev, grads_dev, P, state_dev, workspace, stream);
    return train_opt<3>(net, L.o, *cfg, params_dev, m_dev, v_dev, grads_dev, P, state_dev, workspace, stream);
}

}  // extern "C"
