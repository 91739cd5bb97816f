// The kernel families of libdm_hip.so, described once.  Everything that has to know "which class, which variant, which packing is family n" reads it
// here: the launcher and its explicit instantiation (dm_kernels.cpp, one object per precision and family), the host's launch tables (dm_host.cpp), the
// object lists of both Makefiles (families.mk reads the F( rows and DM_MISC_FAMILY) and the ledger of tests/test_kernel_families.py.
// A new family is one F( row (and, for a new class, one C( row); ids are never renumbered: bench.py, profiles/ and build/k_f32_<id>.o.res name them.
#pragma once
#include "dm_types.h"

namespace dmk {

// step-kernel variants: the plain production instantiation, the AMP / goal / perturbation instantiation, the tap build
enum { SV_PLAIN = 0, SV_AMP = 1, SV_TAPS = 2, SV_V2 = 3, SV_COUNT };      // SV_V2: the AMP instantiation + DM-physics v2

// host class ids: C(kernel class, id, base class) -- the base class is the one whose model tables (MdlLds), pair and row capacities and AMP expert the class shares
#define DM_CLASSES(C)                   \
    C(ClsBiped, 0, ClsBiped)            \
    C(ClsLarge, 1, ClsLarge)            \
    C(ClsBipedObj, 2, ClsBiped)         \
    C(ClsLargeTree, 3, ClsLarge)        \
    C(ClsBipedTree, 4, ClsBiped)

// step families: F(id, characters per wavefront, kernel class, variant), one row per line.
// 0-2 two per wave, 3-5 biped, 6-8 large, 9-10 biped + free body, 12-14 large on the compiled dog3d topology (tree factor), 15-17 biped on the compiled
// humanoid3d topology, 18-23 DM-physics v2, 24 biped + free body two per wave (dribble_amp)
#define DM_STEP_FAMILIES(F)             \
    F(0, 2, ClsBiped, SV_PLAIN)         \
    F(1, 2, ClsBiped, SV_AMP)           \
    F(2, 2, ClsBiped, SV_TAPS)          \
    F(3, 1, ClsBiped, SV_PLAIN)         \
    F(4, 1, ClsBiped, SV_AMP)           \
    F(5, 1, ClsBiped, SV_TAPS)          \
    F(6, 1, ClsLarge, SV_PLAIN)         \
    F(7, 1, ClsLarge, SV_AMP)           \
    F(8, 1, ClsLarge, SV_TAPS)          \
    F(9, 1, ClsBipedObj, SV_AMP)        \
    F(10, 1, ClsBipedObj, SV_TAPS)      \
    F(12, 1, ClsLargeTree, SV_PLAIN)    \
    F(13, 1, ClsLargeTree, SV_AMP)      \
    F(14, 1, ClsLargeTree, SV_TAPS)     \
    F(15, 1, ClsBipedTree, SV_PLAIN)    \
    F(16, 1, ClsBipedTree, SV_AMP)      \
    F(17, 1, ClsBipedTree, SV_TAPS)     \
    F(18, 1, ClsBiped, SV_V2)           \
    F(19, 1, ClsLarge, SV_V2)           \
    F(20, 1, ClsLargeTree, SV_V2)       \
    F(21, 1, ClsBipedTree, SV_V2)       \
    F(22, 2, ClsBiped, SV_V2)           \
    F(23, 1, ClsBipedObj, SV_V2)        \
    F(24, 2, ClsBipedObj, SV_AMP)

// the reset / query / probe family: M(class) for every class, E(class) for the classes with an AMP expert and a time-warp sampler of their own (every class runs its base class's)
#define DM_MISC_FAMILY 11
#define DM_MISC_CLASSES(M) M(ClsBiped) M(ClsBipedObj) M(ClsLarge) M(ClsLargeTree) M(ClsBipedTree)
#define DM_EXPERT_CLASSES(E) E(ClsBiped) E(ClsLarge)

#define DM_CLS_ENUM(Cls, id, Base) k##Cls = id,
enum ClsId { DM_CLASSES(DM_CLS_ENUM) kNumCls };
#undef DM_CLS_ENUM

// the row of a step family; an id without a row has no StepFamily and fails the build
template <int ID> struct StepFamily;
#define DM_STEP_ROW(id, pack, Cls, V) \
    template <> struct StepFamily<id> { typedef Cls C; static constexpr int PACK = pack, VARIANT = V; };
DM_STEP_FAMILIES(DM_STEP_ROW)
#undef DM_STEP_ROW

}  // namespace dmk
