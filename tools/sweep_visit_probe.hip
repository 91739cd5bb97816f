// What does one row visit of the two-per-wave kernel's Gauss-Seidel sweep cost, and which of its instructions pay?  (DuoSim::substep_post, DM_DUO_PGS_ROW in
// deepmimic_amd/csrc/dm_device_duo.h: the text of the visit below is that macro's, on synthetic t, A, lo, hi.)  One wavefront runs the sweep of a 32-row pair, 32 visits x 10
// iterations, between two s_memtime stamps (tick = shader cycle), REPS times.
//   variant a  as shipped: per-visit friction-refresh test (s_bitcmp + s_cbranch), select mask from a 32-bit shift copied into an SGPR pair
//           b  without the per-visit test
//           c  select mask by one 64-bit shift of an opaque 0x0000000100000001
//           d  b + c
//           e  the five VALU of the dependent chain only (no test, no select, no block tests): the floor
//           f  the refresh test once per block of four (one s_and + branch; the tested body only in the blocks that hold a refresh row), 32-bit select masks
//   setting lone    one wave on its SIMD (grid 64)
//           loaded  two waves on the SIMD: the probed one at s_setprio 3, its mate streams v_fma at s_setprio 0 until the probed wave is done (grid 2048; 20 KB of LDS per
//                   workgroup keep a CU at 8 workgroups, the waves pair up by the SIMD they find themselves on)
// Every wait is bounded (a wave whose mate never shows up gives up and is not counted), nothing here can hang.
//   hipcc --offload-arch=gfx950 -O3 -o sweep_visit_probe tools/sweep_visit_probe.hip && ./sweep_visit_probe      (prints one JSON object: cycles per visit, median over waves)
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only -o sweep_visit_probe.s tools/sweep_visit_probe.hip     (the listing: compare a visit with the kernel's)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define OPAQUE_S(x) asm volatile("" : "+s"(x))
#define OPAQUE_V(x) asm volatile("" : "+v"(x))

constexpr int kIters = 10, kRows = 32, kReps = 6, kSlots = 8 * 8 * 2 * 16 * 4, kSpinMax = 200000, kMateMax = 20000;

// lane SRC of the own half (dm_device_duo.h half_bcast_c)
template <int SRC> __device__ __forceinline__ float half_bcast_c(float v) {
    const int x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + (SRC & 15), 0xf, 0xf, true);      // row_newbcast
    if (SRC < 16) return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x142, 0xa, 0xf, false));          // row_bcast:15 into rows 1, 3
    return __int_as_float(__builtin_amdgcn_permlane16_swap(x, x, false, false)[1]);
}
// lanes R and R + 32 take `newv` (dm_device_duo.h half_sel_c): two 32-bit halves ...
template <int R> __device__ __forceinline__ float half_sel32(float oldv, float newv, uint32_t one) {
    const uint32_t m32 = one << R;
    const uint64_t mk = ((uint64_t)m32 << 32) | m32;
    float out;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(out) : "v"(oldv), "v"(newv), "s"(mk));
    return out;
}
// ... or one 64-bit shift of 0x0000000100000001 (R < 32: the two bits never meet)
template <int R> __device__ __forceinline__ float half_sel64(float oldv, float newv, uint64_t one2) {
    const uint64_t mk = one2 << R;
    float out;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(out) : "v"(oldv), "v"(newv), "s"(mk));
    return out;
}

template <int V> struct Var {
    static constexpr bool ROW_TEST = V == 0 || V == 2, SEL64 = V == 2 || V == 3, FLOOR = V == 4, BLK_TEST = V == 5;
};

template <int V> __device__ __forceinline__ long long chain(float& t, float& lam, float& lo, float& hi, const float (&a)[kRows], int Rv_, uint32_t fmask_, int lv_, int rn_fric, int nrm_lane, float fric, int half) {
    using VV = Var<V>;
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < kIters; ++it) {
        uint32_t one = 1u; uint64_t one2 = 0x0000000100000001ull;
        int rnf = rn_fric, Rv = Rv_, lv = lv_; uint32_t fmask = fmask_;
        OPAQUE_S(Rv); OPAQUE_S(fmask); OPAQUE_V(lv); OPAQUE_S(one); OPAQUE_S(one2); OPAQUE_V(rnf);
#define ROW(r, TEST)                                                                                                   \
        {                                                                                                              \
            if (TEST) if (__builtin_expect((fmask >> (r)) & 1u, 0)) { const float ln = __shfl(lam, half * 32 + nrm_lane, 64); if (rnf == (r)) { hi = fric * ln; lo = -hi; } } \
            const float nl = __builtin_amdgcn_fmed3f(lo, t, hi);                                                       \
            const float delta = half_bcast_c<(r)>(nl - lam);                                                           \
            t -= a[r] * delta;                                                                                         \
            if (!VV::FLOOR) lam = VV::SEL64 ? half_sel64<(r)>(lam, nl, one2) : half_sel32<(r)>(lam, nl, one);          \
        }
#define ROW4(b4, TEST) ROW((b4) * 4, TEST) ROW((b4) * 4 + 1, TEST) ROW((b4) * 4 + 2, TEST) ROW((b4) * 4 + 3, TEST)
#define BLK(b4)                                                                                                        \
        if (VV::FLOOR) { ROW4(b4, false) }                                                                             \
        else if ((b4) * 4 < Rv) {                                                                                      \
            if (VV::BLK_TEST) { if (__builtin_expect((fmask & (0xFu << 4 * (b4))) != 0, 0)) { ROW4(b4, true) } else { ROW4(b4, false) } }   \
            else { ROW4(b4, VV::ROW_TEST) }                                                                            \
        }
        BLK(0) BLK(1) BLK(2) BLK(3) BLK(4) BLK(5) BLK(6) BLK(7)
#undef BLK
#undef ROW4
#undef ROW
    }
    return __builtin_amdgcn_s_memtime() - t0;
}

// role by arrival on the SIMD: 0 = the probed wave, 1 = its mate (loaded setting only), others leave
template <int V, bool LOADED>
__global__ void __launch_bounds__(64) k_visit(const float* in, float* sink, long long* cyc, unsigned* ticket, unsigned* done, int Rv, uint32_t fmask, int rn0, int rn1, float fric) {
    __shared__ float pad[LOADED ? 5120 : 64];
    const int l = threadIdx.x, half = l >> 5, hl = l & 31;
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned slot = ((((xcc & 7) * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 15)) * 4 + ((hw >> 4) & 3);
    unsigned role = 0;
    if (l == 0) role = atomicAdd(&ticket[slot], 1u);
    role = __builtin_amdgcn_readfirstlane(role);
    if (l == 0) cyc[(size_t)blockIdx.x * (kReps + 1)] = -1;
    pad[l] = (float)role;
    if (role >= (LOADED ? 2u : 1u)) return;
    if (LOADED && role == 1) {
        // the mate: an independent v_fma stream at priority 0 until the probed wave of this SIMD is done
        float x0 = in[l], x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3;
        for (int i = 0; i < kMateMax; ++i) {
#pragma unroll
            for (int k = 0; k < 64; ++k) { x0 = fmaf(x0, 1.0000001f, 1e-9f); x1 = fmaf(x1, 1.0000001f, 1e-9f); x2 = fmaf(x2, 1.0000001f, 1e-9f); x3 = fmaf(x3, 1.0000001f, 1e-9f); }
            if (__hip_atomic_load(&done[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
        }
        if (x0 + x1 + x2 + x3 == 12345.f) sink[l] = pad[(l + 1) & 15];
        return;
    }
    if (LOADED) {       // wait for the mate's ticket (bounded)
        int spins = 0;
        while (__hip_atomic_load(&ticket[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2u && ++spins < kSpinMax) __builtin_amdgcn_s_sleep(8);
        if (spins >= kSpinMax) { if (l == 0) __hip_atomic_store(&done[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    }
    // a pair like the kernel's: lanes >= RN of a half are friction rows, bounded by their normal row's impulse; rows refresh at RN of either half
    const int RN = half ? rn1 : rn0, NL = 4;
    const bool is_fric = hl >= RN;
    const int nrm_lane = is_fric ? NL + ((hl - RN) >> 1) : 0, rn_fric = is_fric ? RN : -1;
    float a[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) a[r] = (r == hl) ? 0.f : in[64 + l * kRows + r];
    float t = in[l], lam = 0, lo = 0, hi = is_fric ? 0.f : 1e30f;
    OPAQUE_S(fric);
    __builtin_amdgcn_s_setprio(3);
    for (int rep = 0; rep < kReps; ++rep) {
        const long long c = chain<V>(t, lam, lo, hi, a, Rv, fmask, hl, rn_fric, nrm_lane, fric, half);
        if (l == 0) cyc[(size_t)blockIdx.x * (kReps + 1) + 1 + rep] = c;
    }
    __builtin_amdgcn_s_setprio(0);
    if (l == 0) { cyc[(size_t)blockIdx.x * (kReps + 1)] = role; if (LOADED) __hip_atomic_store(&done[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    sink[(size_t)blockIdx.x * 64 + l] = t + lam + lo + hi;
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? -1 : v[v.size() / 2]; }

template <int V, bool LOADED> static void run(const float* in, float* sink, long long* cyc, unsigned* ticket, unsigned* done, double* out, int* waves) {
    const int G = LOADED ? 2048 : 64;
    std::vector<long long> h((size_t)G * (kReps + 1));
    for (int pass = 0; pass < 2; ++pass) {      // the first pass warms the instruction cache and the clocks
        hipMemset(ticket, 0, kSlots * 4); hipMemset(done, 0, kSlots * 4);
        hipLaunchKernelGGL((k_visit<V, LOADED>), dim3(G), dim3(64), 0, 0, in, sink, cyc, ticket, done, 32, (1u << 13) | (1u << 22), 13, 22, 0.9f);
        hipDeviceSynchronize();
    }
    if (hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "copy failed\n"); exit(1); }
    std::vector<double> per_wave;
    for (int b = 0; b < G; ++b) {
        if (h[(size_t)b * (kReps + 1)] != 0) continue;      // a mate, a wave without a mate, or one that left
        std::vector<double> r;
        for (int k = 1; k < kReps; ++k) r.push_back((double)h[(size_t)b * (kReps + 1) + 1 + k] / (kIters * kRows));     // (the first repetition is dropped)
        per_wave.push_back(median(r));
    }
    *out = median(per_wave); *waves = (int)per_wave.size();
}

int main() {
    float *in, *sink; long long* cyc; unsigned *ticket, *done;
    const size_t nin = 64 + 64 * kRows;
    std::vector<float> hin(nin);
    uint32_t s = 12345u;
    for (size_t i = 0; i < nin; ++i) { s = s * 1664525u + 1013904223u; hin[i] = ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * (i < 64 ? 1.0f : 0.05f); }
    hipMalloc(&in, nin * 4); hipMalloc(&sink, 2048 * 64 * 4); hipMalloc(&cyc, 2048 * (kReps + 1) * 8); hipMalloc(&ticket, kSlots * 4); hipMalloc(&done, kSlots * 4);
    hipMemcpy(in, hin.data(), nin * 4, hipMemcpyHostToDevice);
    const char* names[6] = {"a_shipped", "b_no_row_test", "c_sel64", "d_no_row_test_sel64", "e_chain_valu_only", "f_block_test"};
    double lone[3][6], loaded[3][6]; int wl[6], wd[6];
    for (int rep = 0; rep < 3; ++rep) {
        run<0, false>(in, sink, cyc, ticket, done, &lone[rep][0], &wl[0]); run<1, false>(in, sink, cyc, ticket, done, &lone[rep][1], &wl[1]);
        run<2, false>(in, sink, cyc, ticket, done, &lone[rep][2], &wl[2]); run<3, false>(in, sink, cyc, ticket, done, &lone[rep][3], &wl[3]);
        run<4, false>(in, sink, cyc, ticket, done, &lone[rep][4], &wl[4]); run<5, false>(in, sink, cyc, ticket, done, &lone[rep][5], &wl[5]);
        run<0, true>(in, sink, cyc, ticket, done, &loaded[rep][0], &wd[0]); run<1, true>(in, sink, cyc, ticket, done, &loaded[rep][1], &wd[1]);
        run<2, true>(in, sink, cyc, ticket, done, &loaded[rep][2], &wd[2]); run<3, true>(in, sink, cyc, ticket, done, &loaded[rep][3], &wd[3]);
        run<4, true>(in, sink, cyc, ticket, done, &loaded[rep][4], &wd[4]); run<5, true>(in, sink, cyc, ticket, done, &loaded[rep][5], &wd[5]);
    }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "device error\n"); return 1; }
    printf("{\"what\": \"cycles per row visit (s_memtime ticks), 32 visits x 10 iterations, median over waves of the per-wave median of %d repetitions; three runs each\", \"unit\": \"shader cycles per visit\"", kReps - 1);
    for (int set = 0; set < 2; ++set) {
        printf(", \"%s\": {", set ? "two_waves_per_simd_mate_fma_prio0_probed_prio3" : "one_wave_per_simd");
        for (int v = 0; v < 6; ++v) {
            const double(*x)[6] = set ? loaded : lone;
            printf("%s\"%s\": {\"runs\": [%.2f, %.2f, %.2f], \"waves\": %d}", v ? ", " : "", names[v], x[0][v], x[1][v], x[2][v], set ? wd[v] : wl[v]);
        }
        printf("}");
    }
    printf("}\n");
    return 0;
}
