// A probe for the wave-level primitives at the top of dm_device.h / dm_device_duo.h -- the cross-lane, select, row-file, matrix-core and hardware-approximation helpers
// that have one body for gfx950 (DPP, v_permlane*, inline asm, MFMA, M0-indexed register vectors) and another, a plain statement, under DM_EMU.  One launch evaluates ONE
// primitive, chosen by `op` (include/dm_hip.h DM_WOP_*, which also says what each op reads and writes), in every workgroup of the grid; a workgroup is one wavefront and
// works on its own block of the input.  tests/test_wave_primitives.py is the caller, nothing of the product is.
// Included by dm_kernels.cpp in the reset / query / probe object only (DM_MISC_FAMILY, both precisions): dm_device.h, dm_device_duo.h and the step-family objects do not
// know of it.  The emulator build compiles the same text with the generic bodies, so one test file holds both bodies to the same references.
//
// Layout: lane l of workgroup w reads in[(w * 64 + l) * DM_WAVE_PROBE_IN ..] and writes out[(w * 64 + l) * DM_WAVE_PROBE_OUT ..], doubles both.  The kernel narrows what an
// op reads to Real and widens what it writes (both exact for values of Real) and calls the dmk:: primitive itself -- nothing of a primitive's arithmetic is restated here.
// Wave-uniform arguments (a source lane, a row-file index) are read from the row of lane 0 (lane 1 for the second list), so they are runtime values in SGPRs; template
// arguments are swept by static_for, one output column per argument.  Every operand comes from memory, `z` and `one` are made opaque as the call sites make them, and the
// Gram operands pass DM_OPAQUE_V as theirs do: nothing is folded away.  Lanes and columns an op does not write keep the caller's fill.
//
// NOT covered: DuoSim::subtree_mfma (the v_mfma_f64_16x16x4_f64 subtree sums) is a member of the two-per-wave simulator that works on its LDS record; it cannot be called
// without restating it, and stays with the end-to-end parity and duo_*_bits tests.
//
// WHAT THIS PINS: the primitives' source text as the misc object compiles it.  The copies inlined into the step objects are built from the same text inside much larger
// functions (and, for some families, under other -mllvm flags); data movement, selects and the MFMA layouts do not depend on that, the contraction of a * b + c around
// dm_rcp / dm_rsqrt may.
#pragma once
#include "../../include/dm_hip.h"

namespace dmw {
using namespace dmk;

// the lane masks of the lane_sel op, DM_WAVE_PROBE_MASK_CHUNKS chunks of 64 (chunk = `arg`, column = position): every mask a kernel instantiates lane_sel with, then edges
constexpr uint64_t wp_mask(int chunk, int c) {
    switch (chunk) {
    case 0: return TopoDog3d::T.anc[c];                                        // tree_load_col
    case 1: return TopoDog3d::T.desc[c];                                       // tree_fwd
    case 2: return TopoDog3d::T.levmask[c];                                    // tree_elim (0 past the last level)
    case 3: return c < 34 ? TopoHumanoid3d::T.anc[c] : 0ull;
    case 4: return c < 34 ? TopoHumanoid3d::T.desc[c] : 0ull;
    case 5: return c < 34 ? TopoHumanoid3d::T.levmask[c] : 0ull;
    case 6: return (1ull << c) - 1ull;                                         // tree_solve: lanes below dof c
    case 7:                                                                    // DuoSim: chol_solve's `keep` (j = 3..33), back_substitute's `below` (k = 4..33), both halves alike
        if (c < 31) { const uint64_t keep = (~((1ull << (c + 1)) - 1ull)) & 0xffffffffull; return (keep << 32) | keep; }
        if (c < 61) { const uint64_t below = (1ull << (c - 30)) - 1ull; return (below << 32) | below; }
        return c == 61 ? ~0ull : (c == 62 ? 0xffffffff00000000ull : 0x00000000ffffffffull);
    default:                                                                   // edges, then arbitrary words
        return c == 0 ? 0ull : c == 1 ? ~0ull : c == 2 ? 1ull : c == 3 ? (1ull << 31) : c == 4 ? (1ull << 32) : c == 5 ? (1ull << 63) : (uint64_t)c * 0x9E3779B97F4A7C15ull;
    }
}

template <typename Real> struct WaveProbe {
    typedef typename VecT<Real>::v2 R2;
    const int l, half, hl;
    const double* x;        // this lane's input row
    const double* x0;       // the row of lane 0 of this workgroup: wave-uniform arguments (x0 + IN: lane 1's)
    double* y;

    DM_DEV WaveProbe(const double* in, double* out)
        : l((int)threadIdx.x), half((int)threadIdx.x >> 5), hl((int)threadIdx.x & 31), x(in + ((size_t)blockIdx.x * 64 + threadIdx.x) * DM_WAVE_PROBE_IN),
          x0(in + (size_t)blockIdx.x * 64 * DM_WAVE_PROBE_IN), y(out + ((size_t)blockIdx.x * 64 + threadIdx.x) * DM_WAVE_PROBE_OUT) {}

    template <int NP2> DM_DEV void load_y(R2 (&y2)[NP2]) const {
#pragma unroll
        for (int p = 0; p < NP2; ++p) { y2[p][0] = (Real)x[2 * p]; y2[p][1] = (Real)x[2 * p + 1]; }
#pragma unroll
        for (int p = 0; p < NP2; ++p) DM_OPAQUE_V(y2[p]);
    }
    template <int N> DM_DEV void store(const Real (&g)[N], int at = 0) const {
#pragma unroll
        for (int i = 0; i < N; ++i) y[at + i] = (double)g[i];
    }
    template <int NP2> DM_DEV void gram32() const { R2 y2[NP2]; load_y(y2); Real g[32]; wave_gram32<NP2>(y2, g); store(g); }
    template <int NP2> DM_DEV void gram64() const {
        R2 y2[NP2]; load_y(y2);
        Real g[32];
        wave_gram64_half<NP2, 1>(y2, g); store(g, 32);       // (the order of the call site: entries 32..63 first)
        wave_gram64_half<NP2, 0>(y2, g); store(g, 0);
    }
    template <int NP2> DM_DEV void duo_gram() const { R2 y2[NP2]; load_y(y2); Real g[32]; duo_gram32<NP2>(y2, g); store(g); }
    template <int NP2, int X, int Y> DM_DEV void xd_block() const {
        R2 y2[NP2]; load_y(y2);
        xd_gram_operands<NP2>(y2);
        Real g[32];
        xd_gram_block<NP2, X, Y>(y2, [&](auto rc, Real v) { g[decltype(rc)::value] = v; });
        store(g);
    }
    template <int N, int MASK> DM_DEV void tr_stage() const {
        constexpr int NP2 = 17;
        Real w[NP2];
#pragma unroll
        for (int i = 0; i < NP2; ++i) w[i] = (Real)x[i];
        xd_tr_stage<N, MASK, NP2>(w, hl);
        store(w);
    }
    // a row file of N entries: filled from the lane's row by static indices, then entry s[k] := x[k] for every k with s[k] >= 0, then out[k] = entry g[k]; s and g are the
    // second halves of the rows of lanes 0 and 1.  The float specialisations take the runtime index itself (M0-relative register indexing); the generic Real v[N] -- fp64, and
    // the 56 of the plain dog3d instantiation -- is only ever indexed statically by the kernels and is here too (a compare chain picks the static index), or it would live in scratch.
    template <int N> DM_DEV void row_file() const {
#ifdef DM_EMU
        constexpr bool RT = true;
#else
        constexpr bool RT = std::is_same<Real, float>::value && N != 56;
#endif
        RowFile<Real, N> f;
        static_for<0, N>([&](auto kc) { constexpr int k = decltype(kc)::value; f.set(k, (Real)x[k]); });
        const double* s = x0 + 64; const double* g = x0 + DM_WAVE_PROBE_IN + 64;
        if constexpr (RT) {
#pragma unroll 1
            for (int k = 0; k < N; ++k) { const int i = (int)s[k]; if (i >= 0 && i < N) f.set(i, (Real)x[k]); }
#pragma unroll 1
            for (int k = 0; k < N; ++k) { const int i = (int)g[k]; if (i >= 0 && i < N) y[k] = (double)f.get(i); }
        } else {
            // entry by entry, each under its static index: the last k with s[k] == j is what entry j holds in the end; then entry j goes to every column that asks for it
            // (a chain of `if (i == j) f.set(j, v)` inside the k loop is folded back into one store at a runtime index, and the file moves to scratch)
            static_for<0, N>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                Real e = f.get(j);
#pragma unroll 1
                for (int k = 0; k < N; ++k) if ((int)s[k] == j) e = (Real)x[k];
                f.set(j, e);
            });
            static_for<0, N>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const double e = (double)f.get(j);
#pragma unroll 1
                for (int k = 0; k < N; ++k) if ((int)g[k] == j) y[k] = e;
            });
        }
    }
    template <int CHUNK> DM_DEV void lane_sels() const {
        uint64_t z = 0; DM_OPAQUE_S(z);
        const Real a = (Real)x[0], b = (Real)x[1];
        static_for<0, 64>([&](auto cc) { constexpr int c = decltype(cc)::value; y[c] = (double)lane_sel<wp_mask(CHUNK, c)>(a, b, l, z); });
    }

    DM_DEV void run(int op, int arg) const {
        switch (op) {
        case DM_WOP_WAVE_SHFL: y[0] = (double)wave_shfl((Real)x[0], (int)x[1]); break;
        case DM_WOP_LANE_BCAST: {
            const Real v = (Real)x[0];
#pragma unroll 1
            for (int c = 0; c < 63; ++c) y[c] = (double)lane_bcast(v, (int)x0[1 + c]);
            break;
        }
        case DM_WOP_HALF_BCAST: {
            const Real v = (Real)x[0];
#pragma unroll 1
            for (int c = 0; c < 63; ++c) y[c] = (double)half_bcast(v, (int)x0[1 + c], half);
            break;
        }
        case DM_WOP_HALF_BCAST_C: {
            const Real v = (Real)x[0];
            static_for<0, 32>([&](auto sc) { constexpr int S = decltype(sc)::value; y[S] = (double)half_bcast_c<S>(v, half); });
            break;
        }
        case DM_WOP_SHFL_XOR_C: {
            const Real v = (Real)x[0];
            static_for<0, 6>([&](auto bc) { constexpr int B = decltype(bc)::value; y[B] = (double)wave_shfl_xor_c<(1 << B)>(v); });
            break;
        }
        case DM_WOP_LANE_SEL:
            static_for<0, DM_WAVE_PROBE_MASK_CHUNKS>([&](auto hc) { constexpr int H = decltype(hc)::value; if (arg == H) lane_sels<H>(); });
            break;
        case DM_WOP_ROW_SEL_C: {
            uint32_t one = 1; DM_OPAQUE_S(one);
            const Real o = (Real)x[0], n = (Real)x[1];
            static_for<0, 64>([&](auto rc) { constexpr int R = decltype(rc)::value; y[R] = (double)row_sel_c<R>(o, n, l, one); });
            break;
        }
        case DM_WOP_HALF_SEL_C: {
            uint32_t one = 1u; DM_OPAQUE_S(one);
            const Real o = (Real)x[0], n = (Real)x[1];
            static_for<0, 32>([&](auto rc) { constexpr int R = decltype(rc)::value; y[R] = (double)half_sel_c<R>(o, n, hl, one); });
            break;
        }
        case DM_WOP_CHAIN_KEEP: {
            const Real v = (Real)x[0];
            const uint32_t lo = (uint32_t)x[1], hi = (uint32_t)x[2];
            static_for<0, 64>([&](auto jc) { constexpr int J = decltype(jc)::value; y[J] = (double)chain_keep<J>(v, lo, hi); });
            break;
        }
        case DM_WOP_ROW_FILE:
            if (arg == 32) row_file<32>(); else if (arg == 40) row_file<40>(); else if (arg == 48) row_file<48>(); else if (arg == 56) row_file<56>(); else row_file<64>();
            break;
        case DM_WOP_BALLOT: {
            const uint64_t m = wave_ballot(x[0] != 0.0);
            y[0] = (double)(uint32_t)(m & 0xffffffffull); y[1] = (double)(uint32_t)(m >> 32);
            break;
        }
        case DM_WOP_WAVE_SUM: y[0] = (double)wave_sum((Real)x[0]); break;
        case DM_WOP_HALF_SUM: y[0] = (double)half_sum((Real)x[0]); break;
        case DM_WOP_RCP:
#pragma unroll 1
            for (int c = 0; c < 64; ++c) y[c] = (double)dm_rcp((Real)x[c]);
            break;
        case DM_WOP_RSQRT:
#pragma unroll 1
            for (int c = 0; c < 64; ++c) y[c] = (double)dm_rsqrt((Real)x[c]);
            break;
        case DM_WOP_MED3:
#pragma unroll 1
            for (int c = 0; c < 32; ++c) y[c] = (double)dm_med3((Real)x[3 * c], (Real)x[3 * c + 1], (Real)x[3 * c + 2]);
            break;
        case DM_WOP_WG_UNIT: y[0] = (double)dm_wg_unit(); break;
        case DM_WOP_GRAM32: if (arg == 17) gram32<17>(); else if (arg == 20) gram32<20>(); else gram32<32>(); break;
        case DM_WOP_GRAM64: if (arg == 17) gram64<17>(); else gram64<32>(); break;
        case DM_WOP_DUO_GRAM32: if (arg == 17) duo_gram<17>(); else duo_gram<20>(); break;
        case DM_WOP_XD_OPERANDS: {
            R2 y2[17]; load_y(y2);
            xd_gram_operands<17>(y2);
#pragma unroll
            for (int p = 0; p < 17; ++p) { y[2 * p] = (double)y2[p][0]; y[2 * p + 1] = (double)y2[p][1]; }
            break;
        }
        case DM_WOP_XD_BLOCK:
            if (arg == 0) xd_block<17, 0, 0>(); else if (arg == 1) xd_block<17, 0, 1>(); else if (arg == 2) xd_block<17, 1, 0>(); else xd_block<17, 1, 1>();
            break;
        case DM_WOP_XD_TR_STAGE:       // the four stages of duo_rows_xd behind its shuffle-by-one stage (NP2 = 17)
            if (arg == 0) tr_stage<17, 2>(); else if (arg == 1) tr_stage<9, 4>(); else if (arg == 2) tr_stage<5, 8>(); else tr_stage<3, 16>();
            break;
        default: break;                 // (the entry point refuses an unknown op before the launch)
        }
    }
};

template <typename Real>
__global__ void __launch_bounds__(64) k_wave_probe(int op, int arg, const double* in, double* out) {
    const WaveProbe<Real> p(in, out);
    p.run(op, arg);
}

}  // namespace dmw

namespace dmk {
template <typename Real> void launch_wave_probe(unsigned grid, rt_stream s, int op, int arg, const double* in, double* out) {
    RT_LAUNCH(dmw::k_wave_probe<Real>, grid, s, op, arg, in, out);
}
}  // namespace dmk
