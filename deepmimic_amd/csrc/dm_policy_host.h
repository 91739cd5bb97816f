// Host side of the on-device policy (dm_policy.h): allocates a context's packed arrays, has k_policy_pack fill them from the fp32 weights of the
// reference's actor -- the same launch for a new context and for new weights into a live one (policy_pack); the layout is defined there, in dm_policy.h --
// and launches the layer kernels.  Included at the end of dm_host.cpp (shares its runtime shim).
#include "dm_policy.h"

struct dm_policy {
    dmp::PolicyDev pd; int device_id = 0; int cap = 0;
    int last_path = DM_POLICY_PATH_NONE, last_rows = 0;      // dm_policy_info: the kernels of the last dm_policy_forward(_ex)
    int scalar_path = DM_POLICY_PATH_NONE, scalar_rows = 0, scalar_kind = 0, scalar_masked = 0;      // dm_policy_scalar_info: the last dm_policy_eval_scalar
    uint16_t *h1 = nullptr, *h2 = nullptr, *s16 = nullptr;
    bool gated = false; dmp::GateDev gd; const dmp::GateDev* gd_dev = nullptr;   // dm_policy_create_gated: the gate's packed weights (gd_dev: the copy the fused kernel reads)
    float* gbuf[4] = {nullptr, nullptr, nullptr, nullptr};   // sigma_0, beta_0 [cap x H1], sigma_1, beta_1 [cap x H2] fp32, grown with h1 / h2
    std::vector<void*> allocs;
    void free_gbuf() { for (float*& b : gbuf) { if (b) rt_free(b); b = nullptr; } }
    ~dm_policy() { for (void* p : allocs) rt_free(p); if (h1) rt_free(h1); if (h2) rt_free(h2); if (s16) rt_free(s16); free_gbuf(); }
    void* alloc(size_t bytes) { void* d = nullptr; if (rt_malloc(&d, bytes)) return nullptr; allocs.push_back(d); return d; }      // freed with the context
};

// the launches of a path id, plain or GATED: one copy of the kernel choice for both
template <bool GATED>
static void launch_fused(int path, unsigned grid, rt_stream stream, const dmp::PolicyDev& d, const dmp::PolicyIO& io) {
    switch (path) {
    case DM_POLICY_PATH_FUSED_8_2: RT_LAUNCH4((dmp::k_policy_fused<8, 2, GATED>), grid, stream, d, io); break;
    case DM_POLICY_PATH_FUSED_8_4: RT_LAUNCH4((dmp::k_policy_fused<8, 4, GATED>), grid, stream, d, io); break;
    case DM_POLICY_PATH_FUSED_12_2: RT_LAUNCH4((dmp::k_policy_fused<12, 2, GATED>), grid, stream, d, io); break;
    default: RT_LAUNCH4((dmp::k_policy_fused<12, 4, GATED>), grid, stream, d, io); break;
    }
}
// the scalar head's one-launch kernels: action_dim = 1, so N3 = 32 and the id is one of the two K1 choices
template <bool GATED>
static void launch_fused_scalar(int path, unsigned grid, rt_stream stream, const dmp::PolicyDev& d, const dmp::ScalarIO& io) {
    if (path == DM_POLICY_PATH_FUSED_8_2) RT_LAUNCH4((dmp::k_policy_fused<8, 1, GATED, 1>), grid, stream, d, io);
    else RT_LAUNCH4((dmp::k_policy_fused<12, 1, GATED, 1>), grid, stream, d, io);
}
// layers 1 and 2; tiles sized so that every launch has at least ~1 wave per SIMD at 4096 rows: 64 x 64 (layer 1), 32 x 64 (layer 2)
template <bool GATED>
static void launch_layers(int path, int n, rt_stream stream, const dmp::PolicyDev& d, const dmp::PolicyIO& io) {
    switch (DM_POLICY_PATH_LAYER1(path)) {
    case DM_POLICY_LAYER_TILE128: RT_LAUNCH4((dmp::k_policy_gemm<0, 128, GATED>), ((n + 127) / 128) * (d.H1 / 128), stream, d, io); break;
    case DM_POLICY_LAYER_TILE64: RT_LAUNCH4((dmp::k_policy_gemm<0, 64, GATED>), ((n + 63) / 64) * (d.H1 / 128), stream, d, io); break;
    default: RT_LAUNCH((dmp::k_policy_layer<0, 4, 4, GATED>), ((n + 63) / 64) * (d.H1 / 64), stream, d, io); break;
    }
    switch (DM_POLICY_PATH_LAYER2(path)) {
    case DM_POLICY_LAYER_TILE128: RT_LAUNCH4((dmp::k_policy_gemm<1, 128, GATED>), ((n + 127) / 128) * (d.H2 / 128), stream, d, io); break;
    case DM_POLICY_LAYER_TILE64: RT_LAUNCH4((dmp::k_policy_gemm<1, 64, GATED>), ((n + 63) / 64) * (d.H2 / 128), stream, d, io); break;
    default: RT_LAUNCH((dmp::k_policy_layer<1, 2, 4, GATED>), ((n + 31) / 32) * (d.H2 / 64), stream, d, io); break;
    }
}

// The per-layer route for the widths: the LDS-tiled four-wave GEMM of height `tile` when the width allows it (a multiple of 128) and `tiled`, the one-wave kernel otherwise.
// With its defaults it is the route the trainers force (dm_train.h train_forward), whatever DM_POLICY_* says.
static int policy_path_layered(const dmp::PolicyDev& d, bool tiled = true, int tile = DM_POLICY_LAYER_TILE64) {
    const int l1 = (tiled && d.H1 % 128 == 0) ? tile : DM_POLICY_LAYER_ONE_WAVE, l2 = (tiled && d.H2 % 128 == 0) ? tile : DM_POLICY_LAYER_ONE_WAVE;
    return DM_POLICY_PATH_LAYERED(l1, l2);
}

// The ONE place that decides which kernels a forward call runs (ids: include/dm_hip.h dm_policy_path): dm_policy_forward_ex launches from the id
// this returns and dm_policy_info reports it, so the report cannot drift from the launch.
// One launch for the whole actor (k_policy_fused) where it is compiled for the widths; DM_POLICY_LAYERED=1 keeps the per-layer kernels (A/B, tests).
// Per layer: the LDS-tiled four-wave GEMM when the width allows it (a multiple of 128), the one-wave kernel otherwise or under DM_POLICY_ONE_WAVE.
// 64-row tiles by default (measured: 45 / 82 us at 4096 / 16384 rows against 56 / 85 us with 128-row tiles: more workgroups per CU hide more
// of the L2 latency than the bigger tile saves in traffic); DM_POLICY_TILE=128 selects the tall tile
static int policy_path(const dmp::PolicyDev& d) {
    if (d.wfs && getenv("DM_POLICY_LAYERED") == nullptr) {
        if (d.K1 == 256) return d.N3 == 32 ? DM_POLICY_PATH_FUSED_8_2 : DM_POLICY_PATH_FUSED_8_4;
        return d.N3 == 32 ? DM_POLICY_PATH_FUSED_12_2 : DM_POLICY_PATH_FUSED_12_4;
    }
    const bool tiled = (getenv("DM_POLICY_ONE_WAVE") == nullptr);
    int tile = DM_POLICY_LAYER_TILE64;
    if (const char* tl = getenv("DM_POLICY_TILE")) if (atoi(tl) == 128) tile = DM_POLICY_LAYER_TILE128;
    return policy_path_layered(d, tiled, tile);
}

extern "C" {

int dm_policy_info(dm_policy* p, int32_t* out) {
    if (!p || !out) return fail("null argument");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = p->pd.K1; out[1] = p->pd.N3; out[2] = p->pd.wfs ? 1 : 0; out[3] = p->last_path; out[4] = p->last_rows;
    out[5] = p->gated ? 1 : 0; out[6] = p->gated ? p->gd.G : 0; out[7] = (p->gated && p->pd.wfs) ? 1 : 0;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- fp32 weights into a context's packed arrays (k_policy_pack, dm_policy.h)
// The jobs of one k_policy_pack launch: one per destination array whose source is given, in the buffers policy_create allocated (their sizes: packed_array)
struct PackPlan {
    dmp::PackArgs a; unsigned blocks = 0;
    PackPlan() { memset(&a, 0, sizeof(a)); }
    void add(int kind, const float* src, const void* dst, int K, int N, int KS, size_t rows) {
        if (a.njobs >= dmp::PK_MAX_JOBS) return;
        dmp::PackJob& j = a.job[a.njobs];
        j.kind = kind; j.K = K; j.N = N; j.KS = KS; j.rows = (int)rows; j.src = src; j.dst = const_cast<void*>(dst);
        a.first[a.njobs++] = (int)blocks; blocks += (unsigned)((rows + 255) / 256); a.first[a.njobs] = (int)blocks;
    }
    // W [K x N] into fragments padded to Kp x Np
    void frag(const float* W, const uint16_t* dst, int K, int N, int Kp, int Np) { if (W) add(dmp::PK_FRAG, W, dst, K, N, Kp / 32, (size_t)Kp * Np / 8); }
    void vec(const float* src, const float* dst, int n, int np) { if (src) add(dmp::PK_VEC, src, dst, 0, n, 0, (size_t)np); }
};

// bytes of the fused stream a context holds: per wave 4 chunks of K1 / 64 + 8 blocks, with a gate 3 more per chunk and 6 behind the last (k_policy_pack, PK_FUSED)
static size_t fused_stream_bytes(const dm_policy* p) {
    const int NB1 = p->pd.K1 / 64, NBLK = p->gated ? 4 * (NB1 + 3 + 8) + 6 : 4 * (NB1 + 8);
    return (size_t)4 * NBLK * 8 * 512 * 2;
}

template <typename T> static const void* packed_member(const T*& member, void* fresh) { if (fresh) member = static_cast<const T*>(fresh); return member; }
// the packed device array `which` (include/dm_hip.h dm_policy_packed) and its size; null: the context holds no such array (*bytes is set only for an id the
// context's kind has).  `fresh`: policy_create's new allocation of that size, which becomes the array.  The ONE statement of the sizes.
static const void* packed_array(dm_policy* p, int which, size_t* bytes, void* fresh = nullptr) {
    dmp::PolicyDev& d = p->pd; dmp::GateDev& q = p->gd;
    const size_t f = sizeof(float);
    switch (which) {
    case DM_POLICY_PACKED_W1P: *bytes = (size_t)d.K1 * d.H1 * 2; return packed_member(d.w1p, fresh);
    case DM_POLICY_PACKED_W2P: *bytes = (size_t)d.H1 * d.H2 * 2; return packed_member(d.w2p, fresh);
    case DM_POLICY_PACKED_W3P: *bytes = (size_t)d.H2 * d.N3 * 2; return packed_member(d.w3p, fresh);
    case DM_POLICY_PACKED_B1: *bytes = f * d.H1; return packed_member(d.b1, fresh);
    case DM_POLICY_PACKED_B2: *bytes = f * d.H2; return packed_member(d.b2, fresh);
    case DM_POLICY_PACKED_B3: *bytes = f * d.N3; return packed_member(d.b3, fresh);
    case DM_POLICY_PACKED_S_MEAN: *bytes = f * d.S; return packed_member(d.s_mean, fresh);
    case DM_POLICY_PACKED_S_INV_STD: *bytes = f * d.S; return packed_member(d.s_inv_std, fresh);
    case DM_POLICY_PACKED_A_MEAN: *bytes = f * d.A; return packed_member(d.a_mean, fresh);
    case DM_POLICY_PACKED_A_STD: *bytes = f * d.A; return packed_member(d.a_std, fresh);
    case DM_POLICY_PACKED_LOGSTD: *bytes = f * d.A; return packed_member(d.logstd, fresh);
    case DM_POLICY_PACKED_WFS: *bytes = fused_stream_bytes(p); return packed_member(d.wfs, fresh);
    default: break;
    }
    if (!p->gated || which < DM_POLICY_PACKED_GATE_WCP || which > DM_POLICY_PACKED_GATE_BS1) return nullptr;
    if (which == DM_POLICY_PACKED_GATE_WCP) { *bytes = (size_t)q.KG * q.GC * 2; return packed_member(q.wcp, fresh); }
    if (which == DM_POLICY_PACKED_GATE_BC) { *bytes = f * q.GC; return packed_member(q.bc, fresh); }
    const int i = (which - DM_POLICY_PACKED_GATE_WEP0) / 6, H = i ? d.H2 : d.H1;      // six ids per gated layer, in the order of dm_policy_gate_params
    switch ((which - DM_POLICY_PACKED_GATE_WEP0) % 6) {
    case 0: *bytes = (size_t)q.GC * q.GH * 2; return packed_member(q.wep[i], fresh);
    case 1: *bytes = f * q.GH; return packed_member(q.be[i], fresh);
    case 2: *bytes = (size_t)q.GH * H * 2; return packed_member(q.wbp[i], fresh);
    case 3: *bytes = f * H; return packed_member(q.bb[i], fresh);
    case 4: *bytes = (size_t)q.GH * H * 2; return packed_member(q.wsp[i], fresh);
    default: *bytes = f * H; return packed_member(q.bs[i], fresh);
    }
}

// What dm_policy_create(_gated) and dm_policy_set_weights share behind their checks: every array of `pp` / `gp` that is given (widths: the context's) goes through
// ONE k_policy_pack launch into the context's packed arrays; a null array keeps what the context holds.  Host pointers (no DM_DEVICE_PTRS) are staged through one
// device temporary and the call returns when the launch is complete; device pointers: asynchronous on `stream`.  With every array given -- policy_create --
// every byte of every packed array is written, padding included.
static int policy_pack(dm_policy* p, const dm_policy_params& pp, const dm_policy_gate_params* gp, int flags, rt_stream stream) {
    const dmp::PolicyDev& d = p->pd; const dmp::GateDev& q = p->gd;
    dm_policy_params w = pp; dm_policy_gate_params g; memset(&g, 0, sizeof(g)); if (gp) g = *gp;
    // every array of the two structs with its element count, in one table: the host mode stages through it, nothing else walks the fields
    struct Arr { const float** ptr; size_t count; };
    const size_t S = d.S, H1 = d.H1, H2 = d.H2, A = d.A, G = q.G, GC = q.GC, GH = q.GH;
    const Arr arrs[] = {{&w.w1, S * H1}, {&w.b1, H1}, {&w.w2, H1 * H2}, {&w.b2, H2}, {&w.w3, H2 * A}, {&w.b3, A}, {&w.s_mean, S}, {&w.s_std, S}, {&w.a_mean, A}, {&w.a_std, A}, {&w.logstd, A},
                        {&g.gc_w, G * GC}, {&g.gc_b, GC}, {&g.g0_w, GC * GH}, {&g.g0_b, GH}, {&g.g0_bias_w, GH * H1}, {&g.g0_bias_b, H1}, {&g.g0_scale_w, GH * H1}, {&g.g0_scale_b, H1},
                        {&g.g1_w, GC * GH}, {&g.g1_b, GH}, {&g.g1_bias_w, GH * H2}, {&g.g1_bias_b, H2}, {&g.g1_scale_w, GH * H2}, {&g.g1_scale_b, H2}};
    int rc = 0;
    // host arrays: one scoped device temporary holds them all, the same kernel reads it
    std::vector<float> host;
    if (!(flags & DM_DEVICE_PTRS)) for (const Arr& r : arrs) if (*r.ptr) host.insert(host.end(), *r.ptr, *r.ptr + r.count);
    DevTmp stage(rc, stream, sizeof(float) * host.size(), host.empty() ? nullptr : host.data());
    if (rc) return rc;
    if (stage.p) { const float* at = (const float*)stage.p; for (const Arr& r : arrs) if (*r.ptr) { *r.ptr = at; at += r.count; } }

    PackPlan plan; plan.a.out_in = (flags & DM_WEIGHTS_OUT_IN) ? 1 : 0;
    plan.frag(w.w1, d.w1p, d.S, d.H1, d.K1, d.H1); plan.frag(w.w2, d.w2p, d.H1, d.H2, d.H1, d.H2); plan.frag(w.w3, d.w3p, d.H2, d.A, d.H2, d.N3);
    plan.vec(w.b1, d.b1, d.H1, d.H1); plan.vec(w.b2, d.b2, d.H2, d.H2); plan.vec(w.b3, d.b3, d.A, d.N3);
    plan.vec(w.s_mean, d.s_mean, d.S, d.S); if (w.s_std) plan.add(dmp::PK_RECIP, w.s_std, d.s_inv_std, 0, d.S, 0, (size_t)d.S);
    plan.vec(w.a_mean, d.a_mean, d.A, d.A); plan.vec(w.a_std, d.a_std, d.A, d.A); plan.vec(w.logstd, d.logstd, d.A, d.A);
    const float* sw[2] = {g.g0_scale_w, g.g1_scale_w}; const float* sb[2] = {g.g0_scale_b, g.g1_scale_b};
    const float* bw[2] = {g.g0_bias_w, g.g1_bias_w}; const float* bb[2] = {g.g0_bias_b, g.g1_bias_b};
    if (p->gated) {
        const float* ew[2] = {g.g0_w, g.g1_w}; const float* eb[2] = {g.g0_b, g.g1_b};
        plan.frag(g.gc_w, q.wcp, q.G, q.GC, q.KG, q.GC); plan.vec(g.gc_b, q.bc, q.GC, q.GC);
        for (int i = 0; i < 2; ++i) {
            const int H = i ? d.H2 : d.H1;
            plan.frag(ew[i], q.wep[i], q.GC, q.GH, q.GC, q.GH); plan.vec(eb[i], q.be[i], q.GH, q.GH);
            plan.frag(bw[i], q.wbp[i], q.GH, H, q.GH, H); plan.vec(bb[i], q.bb[i], H, H);
            plan.frag(sw[i], q.wsp[i], q.GH, H, q.GH, H); plan.vec(sb[i], q.bs[i], H, H);
        }
    }
    // the fused stream straight from the fp32 sources; a row whose source is not given keeps its bytes
    dmp::PackFused& fs = plan.a.fs;
    fs.gated = p->gated ? 1 : 0; fs.NB1 = d.K1 / 64; fs.S = d.S; fs.w1 = w.w1; fs.w2 = w.w2;
    for (int i = 0; i < 2; ++i) { fs.ws[i] = sw[i]; fs.wb[i] = bw[i]; fs.bs[i] = sb[i]; fs.bb[i] = bb[i]; }
    const bool fused_src = w.w1 || w.w2 || (p->gated && (sw[0] || sw[1] || bw[0] || bw[1] || sb[0] || sb[1] || bb[0] || bb[1]));
    if (d.wfs && fused_src) plan.add(dmp::PK_FUSED, nullptr, d.wfs, 0, 0, 0, fused_stream_bytes(p) / 16);   // (its sources: PackFused)
    if (plan.blocks == 0) return 0;                        // nothing given: nothing to do
    RT_LAUNCH4(dmp::k_policy_pack, plan.blocks, stream, plan.a);
    if (launch_status(0)) return -1;
    if (stage.p && rt_sync(stream) != 0) return fail("stream synchronize failed");      // the temporary is freed with this scope
    return 0;
}

// gp == nullptr: the plain actor.  With a gate the fused stream is the gated one (gate_hidden = 64 only, else the per-layer kernels).  Validation, the padded widths
// and the allocation are here; what goes into the arrays is policy_pack's.
static int policy_create(int device_id, const dm_policy_params* pp, const dm_policy_gate_params* gp, dm_policy** out) {
    if (!pp || !out) return fail("null argument");
    if (pp->state_dim < 1 || pp->action_dim < 1 || pp->hidden1 < 64 || pp->hidden2 < 64) return fail("dm_policy_create: bad layer widths");
    if (pp->hidden1 % 64 || pp->hidden2 % 64) return fail("dm_policy_create: hidden widths must be multiples of 64 (reference: 1024, 512)");
    if (!pp->w1 || !pp->b1 || !pp->w2 || !pp->b2 || !pp->w3 || !pp->b3) return fail("dm_policy_create: null weights");
    if (gp) {
        if (gp->goal_dim < 1 || gp->goal_dim >= pp->state_dim) return fail("dm_policy_create_gated: goal_dim must be in [1, state_dim): the gate reads the last goal_dim input columns");
        if (gp->goal_dim > 128) return fail("dm_policy_create_gated: goal_dim above 128 is not compiled (k_policy_gate holds the goal block in LDS)");
        if (gp->gate_common < 32 || gp->gate_common % 32 || gp->gate_common > 256 || gp->gate_hidden < 32 || gp->gate_hidden % 32 || gp->gate_hidden > 128)
            return fail("dm_policy_create_gated: gate widths must be multiples of 32, gate_common <= 256 and gate_hidden <= 128 (reference: 128, 64)");
        if (!gp->gc_w || !gp->gc_b || !gp->g0_w || !gp->g0_b || !gp->g0_bias_w || !gp->g0_bias_b || !gp->g0_scale_w || !gp->g0_scale_b ||
            !gp->g1_w || !gp->g1_b || !gp->g1_bias_w || !gp->g1_bias_b || !gp->g1_scale_w || !gp->g1_scale_b) return fail("dm_policy_create_gated: null gate weights");
    }
    if (valid_device(gp ? "dm_policy_create_gated" : "dm_policy_create", device_id)) return -1;
    DevGuard guard(device_id);
    dm_policy* p = new dm_policy(); p->device_id = device_id;
    dmp::PolicyDev& d = p->pd; memset(&d, 0, sizeof(d));
    d.S = pp->state_dim; d.H1 = pp->hidden1; d.H2 = pp->hidden2; d.A = pp->action_dim;
    d.K1 = (d.S + 63) / 64 * 64; d.N3 = (d.A + 31) / 32 * 32;
    // one-launch actor: compiled for the reference's widths (1024, 512), K1 = 256 / 384 and up to 64 action slots; a K1 of 320 or below 256 is padded up
    const bool fusable = d.H1 == 1024 && d.H2 == 512 && d.K1 <= 384 && d.N3 <= 64 && (!gp || gp->gate_hidden == 64);
    if (fusable) d.K1 = d.K1 <= 256 ? 256 : 384;
    d.s_clip = (pp->s_clip > 0) ? (float)pp->s_clip : std::numeric_limits<float>::infinity();
    dmp::GateDev& q = p->gd; memset(&q, 0, sizeof(q));
    if (gp) { p->gated = true; q.G = gp->goal_dim; q.KG = (q.G + 31) / 32 * 32; q.GC = gp->gate_common; q.GH = gp->gate_hidden; }
    // every packed array the context holds, at the size packed_array states for it (the fused stream only where its kernel is compiled)
    for (int which = 0; which <= DM_POLICY_PACKED_GATE_BS1; ++which) {
        size_t bytes = 0;
        packed_array(p, which, &bytes);
        if (bytes == 0 || (which == DM_POLICY_PACKED_WFS && !fusable)) continue;
        if (!packed_array(p, which, &bytes, p->alloc(bytes))) { delete p; return fail("device allocation failed"); }
    }
    if (gp) {                                             // the fused kernel reads the gate's first layers through a device copy of the pointers
        void* g = p->alloc(sizeof(q));
        if (!g || rt_h2d(g, &q, sizeof(q), 0)) { delete p; return fail("device allocation failed"); }
        p->gd_dev = (const dmp::GateDev*)g;
    }
    // an optional array that is not given: its default, packed like a given one (s_inv_std = 1)
    dm_policy_params w = *pp;
    const std::vector<float> zeros((size_t)std::max(d.S, d.A), 0.0f), ones(zeros.size(), 1.0f);
    for (const float** a : {&w.s_mean, &w.a_mean, &w.logstd}) if (!*a) *a = zeros.data();
    for (const float** a : {&w.s_std, &w.a_std}) if (!*a) *a = ones.data();
    if (policy_pack(p, w, gp, 0, 0)) { delete p; return -1; }
    *out = p;
    return 0;
}

static int policy_run(dm_policy* p, dmp::ScalarIO& io, bool scalar, void* hip_stream);

// the goal arguments of dm_policy_forward_ex / dm_policy_eval_scalar; `fn`, `net`: the caller's name and its word for the context, for the message
static int check_goal(const dm_policy* p, const char* fn, const char* net, const float* goals_dev, int goal_dim) {
    if (goal_dim < 0 || goal_dim >= p->pd.S || (goal_dim > 0 && !goals_dev)) return fail(std::string(fn) + ": goal_dim must be in [0, state_dim) with a goal block when positive (state_dim counts the goal columns)");
    if (p->gated && goal_dim != 0 && goal_dim != p->gd.G) return fail(std::string(fn) + ": a gated " + net + " takes its goal as a block of the gate's goal_dim columns, or goal_dim = 0 with the goal in the last columns of states_dev");
    return 0;
}

extern "C" {

int dm_policy_create(int device_id, const dm_policy_params* pp, dm_policy** out) { return policy_create(device_id, pp, nullptr, out); }

int dm_policy_create_gated(int device_id, const dm_policy_params* pp, const dm_policy_gate_params* gp, dm_policy** out) {
    if (!gp) return fail("null argument");
    return policy_create(device_id, pp, gp, out);
}

int dm_policy_destroy(dm_policy* p) { if (!p) return 0; DevGuard guard(p->device_id); delete p; return 0; }

int dm_policy_forward_ex(dm_policy* p, const float* states_dev, const float* goals_dev, int goal_dim, int n, float* actions_dev, float* logp_dev,
                         int32_t* exp_flags_dev, double exp_rate, int sample, uint64_t seed, uint32_t step, int env_id_offset, void* hip_stream);

int dm_policy_forward(dm_policy* p, const float* states_dev, int n, float* actions_dev, float* logp_dev, int sample,
                      uint64_t seed, uint32_t step, int env_id_offset, void* hip_stream) {
    return dm_policy_forward_ex(p, states_dev, nullptr, 0, n, actions_dev, logp_dev, nullptr, 1.0, sample, seed, step, env_id_offset, hip_stream);
}

int dm_policy_forward_ex(dm_policy* p, const float* states_dev, const float* goals_dev, int goal_dim, int n, float* actions_dev, float* logp_dev,
                         int32_t* exp_flags_dev, double exp_rate, int sample, uint64_t seed, uint32_t step, int env_id_offset, void* hip_stream) {
    if (!p || !states_dev || !actions_dev) return fail("null argument");
    if (check_goal(p, "dm_policy_forward_ex", "actor", goals_dev, goal_dim)) return -1;
    if (!(exp_rate >= 0.0 && exp_rate <= 1.0)) return fail("dm_policy_forward_ex: exp_rate must be in [0, 1]");
    if (n <= 0) return 0;
    dmp::ScalarIO io; memset(&io, 0, sizeof(io));
    io.states = states_dev; io.actions = actions_dev; io.logp = logp_dev; io.M = n; io.sample = sample ? 1 : 0;
    io.seed_lo = (uint32_t)seed; io.seed_hi = (uint32_t)(seed >> 32); io.step = step; io.env_off = env_id_offset;
    io.goals = goal_dim ? goals_dev : nullptr; io.G = goal_dim; io.exp_rate = (float)exp_rate; io.exp_flags = exp_flags_dev;
    return policy_run(p, io, false, hip_stream);
}

}  // extern "C"

// the activation buffers of a context grown to n rows (what policy_run and the training calls of dm_train.h share): n x (K1 + H1 + H2) bf16, with a gate its four fp32 scratch
// arrays; a growth waits for `stream` first, so work queued on it has left the old buffers
static int policy_grow(dm_policy* p, int n, rt_stream stream) {
    if (n > p->cap) {                       // hidden activations: n x (H1 + H2) bf16, grown on demand
        rt_sync(stream);
        if (p->h1) rt_free(p->h1); if (p->h2) rt_free(p->h2); if (p->s16) rt_free(p->s16); p->h1 = p->h2 = p->s16 = nullptr; p->cap = 0;
        p->free_gbuf();
        void *a = nullptr, *b = nullptr, *c = nullptr;
        if (rt_malloc(&a, (size_t)n * p->pd.H1 * 2) || rt_malloc(&b, (size_t)n * p->pd.H2 * 2) || rt_malloc(&c, (size_t)n * p->pd.K1 * 2)) { if (a) rt_free(a); if (b) rt_free(b); if (c) rt_free(c); return fail("device allocation failed"); }
        if (p->gated) for (int i = 0; i < 4; ++i) {
            void* g = nullptr;
            if (rt_malloc(&g, (size_t)n * (i < 2 ? p->pd.H1 : p->pd.H2) * sizeof(float))) { p->free_gbuf(); rt_free(a); rt_free(b); rt_free(c); return fail("device allocation failed"); }
            p->gbuf[i] = (float*)g;
        }
        p->h1 = (uint16_t*)a; p->h2 = (uint16_t*)b; p->s16 = (uint16_t*)c; p->cap = n;
    }
    return 0;
}

// What dm_policy_forward_ex and dm_policy_eval_scalar share: the activation buffers grown to io.M rows, the kernel choice (policy_path) and the launches.  `io` carries the
// call's own members (inputs, outputs, noise or head); scalar: the HEAD = 1 instantiation of the kernel that holds layer 3, everything in front of it as for the actor.
static int policy_run(dm_policy* p, dmp::ScalarIO& io, bool scalar, void* hip_stream) {
    const int n = io.M;
    DevGuard guard(p->device_id);
    rt_stream stream = (rt_stream)hip_stream;
    if (policy_grow(p, n, stream)) return -1;
    io.s16 = p->s16; io.h1 = p->h1; io.h2 = p->h2;
    if (!scalar) if (const char* pr = getenv("DM_POLICY_PROBE")) io.probe = atoi(pr);
    io.gsig0 = p->gbuf[0]; io.gbeta0 = p->gbuf[1]; io.gsig1 = p->gbuf[2]; io.gbeta1 = p->gbuf[3]; io.gate = p->gd_dev;
    const dmp::PolicyDev& d = p->pd;
    const int path = policy_path(d);
    const dmp::PolicyIO& pio = io;          // what every kernel but the HEAD = 1 ones takes
    if (scalar) { p->scalar_path = path; p->scalar_rows = n; p->scalar_kind = io.sh.kind; p->scalar_masked = io.sh.row_mask ? 1 : 0; }
    else { p->last_path = path; p->last_rows = n; }
    if (path < DM_POLICY_PATH_LAYERED_BASE) {
        const unsigned grid = (unsigned)((n + 31) / 32);
        if (scalar) {
            if (p->gated) launch_fused_scalar<true>(path, grid, stream, d, io); else launch_fused_scalar<false>(path, grid, stream, d, io);
            return launch_status(0);
        }
#ifndef DM_EMU
        static unsigned long long* prof_buf = nullptr; static int prof_calls = 0;
        if (io.probe == 2) { if (!prof_buf && hipMalloc((void**)&prof_buf, (size_t)8192 * 8 * 8) != hipSuccess) prof_buf = nullptr; io.prof = grid <= 8192 ? prof_buf : nullptr; }
#endif
        if (p->gated) launch_fused<true>(path, grid, stream, d, pio); else launch_fused<false>(path, grid, stream, d, pio);
        if (launch_status(0)) return -1;
#ifndef DM_EMU
        if (io.prof && ++prof_calls == 100) {          // DM_POLICY_PROBE=2: phase times of the 100th launch (100 MHz constant clock -> ns), mean over the workgroups
            (void)hipStreamSynchronize(stream);
            std::vector<unsigned long long> h((size_t)grid * 8); (void)hipMemcpy(h.data(), prof_buf, h.size() * 8, hipMemcpyDeviceToHost);
            double acc[6] = {0, 0, 0, 0, 0, 0}; unsigned long long t0 = ~0ull, t1 = 0;
            for (unsigned b = 0; b < grid; ++b) { for (int i = 0; i < 6; ++i) acc[i] += (double)(h[b * 8 + i + 1] - h[b * 8 + i]); t0 = std::min(t0, h[b * 8]); t1 = std::max(t1, h[b * 8 + 6]); }
            fprintf(stderr, "k_policy_fused phases (s_memtime ticks, mean of %u workgroups): weights + observations requested, noise drawn, observations to LDS %.0f | chunk 0 layer 1 %.0f | rest of the chunks %.0f | layer-2 epilogue + barrier %.0f | layer 3 + head %.0f | logp %.0f || first start -> last end %.0f\n",
                    grid, acc[0] / grid, acc[1] / grid, acc[2] / grid, acc[3] / grid, acc[4] / grid, acc[5] / grid, (double)(t1 - t0));
        }
#endif
        return 0;
    }
    // tiles sized so that every launch has at least ~1 wave per SIMD at 4096 rows: 64 x 64 (layer 1), 32 x 64 (layer 2), 16 x 32 (layer 3)
    RT_LAUNCH(dmp::k_policy_prep, n, stream, d, pio);
    if (p->gated) {
        // the launch is (path id, gated): the same kernel choice per layer, its GATED instantiation, behind k_policy_gate (32 rows per workgroup)
        RT_LAUNCH4(dmp::k_policy_gate, (n + 31) / 32, stream, d, pio, p->gd);
        launch_layers<true>(path, n, stream, d, pio);
    } else launch_layers<false>(path, n, stream, d, pio);
    if (scalar) { RT_LAUNCH((dmp::k_policy_layer<2, 1, 1, false, 1>), (n + 15) / 16, stream, d, io); }   // the scalar head: column tile 0 alone
    else { RT_LAUNCH((dmp::k_policy_layer<2, 1, 2>), (n + 15) / 16, stream, d, pio); }   // one workgroup per 16 rows owns all N3 columns (logp is a row sum)
    return launch_status(0);
}

extern "C" {

int dm_policy_eval_scalar(dm_policy* p, const float* states_dev, const float* goals_dev, int goal_dim, int n, const dm_scalar_head* head, float* out_dev,
                          float* raw_out_dev, void* hip_stream) {
    if (!p || !states_dev || !head || !out_dev) return fail("null argument");
    if (p->pd.A != 1) return fail("dm_policy_eval_scalar: the context has action_dim " + std::to_string(p->pd.A) + ", a scalar head needs a net with one output (create it with action_dim = 1)");
    if (check_goal(p, "dm_policy_eval_scalar", "net", goals_dev, goal_dim)) return -1;
    if (head->kind != DM_SCALAR_HEAD_VALUE && head->kind != DM_SCALAR_HEAD_STYLE) return fail("dm_policy_eval_scalar: head kind must be DM_SCALAR_HEAD_VALUE or DM_SCALAR_HEAD_STYLE");
    if (head->kind == DM_SCALAR_HEAD_VALUE && !(head->lo <= head->hi)) return fail("dm_policy_eval_scalar: value head needs lo <= hi (infinite bounds: no clipping)");
    if (head->kind == DM_SCALAR_HEAD_STYLE && head->task_reward_dev && !(head->lerp >= 0.0f && head->lerp <= 1.0f)) return fail("dm_policy_eval_scalar: lerp must be in [0, 1]");
    if (n <= 0) return 0;
    dmp::ScalarIO io; memset(&io, 0, sizeof(io));
    io.states = states_dev; io.actions = out_dev; io.M = n; io.goals = goal_dim ? goals_dev : nullptr; io.G = goal_dim; io.exp_rate = 1.0f;
    dmp::ScalarHead& h = io.sh;
    h.kind = head->kind == DM_SCALAR_HEAD_STYLE ? dmp::HEAD_STYLE : dmp::HEAD_VALUE;
    h.lo = head->lo; h.hi = head->hi; h.val_fail = head->val_fail; h.val_succ = head->val_succ; h.scale = head->scale; h.lerp = head->lerp; h.fill = head->fill;
    h.terminate = head->terminate_dev; h.task_r = head->task_reward_dev; h.row_mask = head->row_mask_dev; h.raw = raw_out_dev;
    return policy_run(p, io, true, hip_stream);
}

int dm_policy_scalar_info(dm_policy* p, int32_t* out) {
    if (!p || !out) return fail("null argument");
    out[0] = p->scalar_path; out[1] = p->scalar_rows; out[2] = p->scalar_kind; out[3] = p->scalar_masked;
    return 0;
}

}  // extern "C"

static int width_mismatch(const char* what, int got, int have) {
    return fail(std::string("dm_policy_set_weights: ") + what + " is " + std::to_string(got) + ", the context has " + std::to_string(have));
}

extern "C" {

int dm_policy_set_weights(dm_policy* p, const dm_policy_params* pp, const dm_policy_gate_params* gp, int flags, void* hip_stream) {
    if (!p || !pp) return fail("null argument");
    if (flags & ~(DM_DEVICE_PTRS | DM_WEIGHTS_OUT_IN)) return fail("dm_policy_set_weights: flags takes DM_DEVICE_PTRS and DM_WEIGHTS_OUT_IN only");
    const dmp::PolicyDev& d = p->pd; const dmp::GateDev& q = p->gd;
    if (pp->state_dim != d.S) return width_mismatch("state_dim", pp->state_dim, d.S);
    if (pp->hidden1 != d.H1) return width_mismatch("hidden1", pp->hidden1, d.H1);
    if (pp->hidden2 != d.H2) return width_mismatch("hidden2", pp->hidden2, d.H2);
    if (pp->action_dim != d.A) return width_mismatch("action_dim", pp->action_dim, d.A);
    if (gp && !p->gated) return fail("dm_policy_set_weights: gate parameters for a context without a gate (dm_policy_create)");
    if (!gp && p->gated) return fail("dm_policy_set_weights: a gated context (dm_policy_create_gated) needs its dm_policy_gate_params (null arrays in it keep the gate)");
    if (gp) {
        if (gp->goal_dim != q.G) return width_mismatch("goal_dim", gp->goal_dim, q.G);
        if (gp->gate_common != q.GC) return width_mismatch("gate_common", gp->gate_common, q.GC);
        if (gp->gate_hidden != q.GH) return width_mismatch("gate_hidden", gp->gate_hidden, q.GH);
    }
    DevGuard guard(p->device_id);
    return policy_pack(p, *pp, gp, flags, (rt_stream)hip_stream);
}

int dm_policy_read_packed(dm_policy* p, int which, void* host_out, size_t capacity, size_t* bytes) {
    if (!p) return fail("null argument");
    size_t n = 0;
    const void* dev = packed_array(p, which, &n);
    if (!dev) {
        if (which == DM_POLICY_PACKED_WFS) return fail("dm_policy_read_packed: this context holds no fused weight stream (widths k_policy_fused is not compiled for: the per-layer kernels)");
        if (which >= DM_POLICY_PACKED_GATE_WCP && which <= DM_POLICY_PACKED_GATE_BS1) return fail("dm_policy_read_packed: a gate array of a context without a gate");
        return fail("dm_policy_read_packed: unknown array id");
    }
    if (bytes) *bytes = n;
    if (!host_out) return 0;                               // size query
    if (capacity < n) return fail("dm_policy_read_packed: the host buffer is smaller than the array (" + std::to_string(n) + " bytes)");
    DevGuard guard(p->device_id);
#ifndef DM_EMU
    if (hipDeviceSynchronize() != hipSuccess) return fail("device synchronize failed");      // a refresh pending on any stream of the device is complete
#endif
    return rt_d2h(host_out, dev, n, 0) == 0 ? 0 : fail("device to host copy failed");
}

}  // extern "C"
