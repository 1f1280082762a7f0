// score_registry.hpp -- registry of the unrolled kernels' launch shims: what an instantiation unit (score_*_inst.hip) fills in
// for its motif lengths, the list of those units, and the look-ups the launch code calls (defined in score_plan.hip).
#pragma once

#include "score_u8.hpp"

namespace lm {

// Arrays indexed by the motif length M; c32 / c32w rows by SLOT_* (score_kernels.hpp).  nullptr = no such kernel.
struct KernelRegistry {
    ScoreC32Launcher (*c32)[kRegistrySlots];
    PrefilterLauncher *pre, *pre2;
    PrefilterLauncher *pre2_protein;  // the pair scan over the 441 residue pairs (K = 21)
    ScoreU8Launcher *u8, *u8_pairs;
    PrefilterMultiLauncher *pre2_multi;  // several motifs per pass (prefilter2_multi(M) > 1)
    // the same kernels for alphabets of more than 16 symbols (WIDE: 8-byte LDS reads, score_kernels.hpp)
    ScoreC32Launcher (*c32w)[kRegistrySlots];
    PrefilterLauncher *prew;
    ScoreU8Launcher *u8w;
    PrefilterLauncher *preblk;  // protein one-symbol scan on 4-row symbol blocks (score_prefilter_blk.hpp)
};

// One entry per compilation of an instantiation unit: INST (score_inst.hip, LM_INST_ID), LONG (score_long_inst.hip),
// XLONG (score_xlong_inst.hip) and PAIR (score_pair_inst.hip, LM_PAIR_LO) of lightmotif_amd/build.py.  An entry without its
// object fails to link; an object without its entry leaves rows empty, which score_registry_hole reports.
#define LM_REGISTERING_UNITS(X)                                                                                        \
    X(register_score_c32_0) X(register_score_c32_1) X(register_score_c32_2) X(register_score_c32_3)                    \
    X(register_score_c32_4) X(register_score_c32_5) X(register_score_c32_6) X(register_score_c32_7)                    \
    X(register_score_c32_8)                                                                                            \
    X(register_score_c32_long_40) X(register_score_c32_long_44) X(register_score_c32_long_48)                          \
    X(register_score_c32_long_52) X(register_score_c32_long_56) X(register_score_c32_long_60)                          \
    X(register_score_c32_long_64)                                                                                      \
    X(register_score_c32_xlong_72) X(register_score_c32_xlong_80) X(register_score_c32_xlong_88)                       \
    X(register_score_pair_65) X(register_score_pair_81) X(register_score_pair_97) X(register_score_pair_113)
#define LM_DECLARE_UNIT(f) void f(const KernelRegistry &r);
LM_REGISTERING_UNITS(LM_DECLARE_UNIT)
#undef LM_DECLARE_UNIT

#define LM_CAT2(a, b) a##b
#define LM_CAT(a, b) LM_CAT2(a, b)

// nullptr: every row the list promises is filled; else a message naming the first empty one (lm_hip_ctx_create fails with it)
const char *score_registry_hole();

// `wide`: the kernels for alphabets of more than 16 symbols (lds_wide(K): 8-byte LDS reads)
ScoreC32Launcher score_c32_lookup(int M, int slot, bool wide = false);
const char *score_c32_name(int M, int mode);  // the three modes only
// `blocks`: the scan on 4-row symbol blocks (score_prefilter_blk.hpp: K = 21, 4-byte aligned matrix)
PrefilterLauncher score_c32_prefilter_lookup(int M, bool wide = false, bool blocks = false);
PrefilterLauncher score_c32_prefilter2_lookup(int M, int K = 5);
PrefilterMultiLauncher score_c32_prefilter2_multi_lookup(int M);
ScoreU8Launcher score_c32_lookup_u8(int M, bool pairs, bool wide);
// seqset_best.hip keeps a table of its own (WalkKernels, seqset_walk_launch.hpp): seqset_best_fused<M>, M = 1 ... kMaxFastM
// (nullptr: no such kernel)
const void *seqset_best_fused_row(int M);

}  // namespace lm
