// score_inst.hip -- instantiates score_c32<M, MODE> for M in [LM_M_LO, LM_M_HI].
// Compiled several times with different -DLM_M_LO/-DLM_M_HI/-DLM_INST_ID so the
// fully unrolled kernels build in parallel (see build.py).
#include "score_registry.hpp"

#ifndef LM_M_LO
#error "LM_M_LO / LM_M_HI / LM_INST_ID must be defined"
#endif

namespace lm {

// the exact f32 kernels of one length for one alphabet width (WIDE: more than 16 symbols, 8-byte LDS reads)
template <int M, int WIDE>
static void fill_c32_row(ScoreC32Launcher *tab)
{
    tab[SLOT_STORE] = &score_c32_launch<M, MODE_STORE, 0, 32, WIDE>;
    tab[SLOT_ARGMAX] = &score_c32_launch<M, MODE_ARGMAX, 0, 32, WIDE>;
    tab[SLOT_THRESHOLD] = &score_c32_launch<M, MODE_THRESHOLD, 0, 32, WIDE>;
    if constexpr (M % 4 == 0) {
        tab[SLOT_STORE_QL] = &score_c32_launch<M, MODE_STORE, 1, 32, WIDE>;
        tab[SLOT_STORE_C16] = &score_c32_launch<M, MODE_STORE, 1, 16, WIDE>;
        tab[SLOT_STORE_TRACK] = &score_c32_launch<M, MODE_STORE_TRACK, 1, 32, WIDE>;
    }
    tab[SLOT_STORE_ARGMAX] = &score_c32_launch<M, MODE_STORE_ARGMAX, 1, 32, WIDE>;
    tab[SLOT_CONTINUE] = &score_c32_launch<M, MODE_CONTINUE, 1, 32, WIDE>;
}

template <int M>
struct RegisterRange {
    static void run(const KernelRegistry &r)
    {
        r.pre[M] = &launch_scan<score_c32_prefilter<M>>;
        r.u8[M] = &launch_scan<score_c32_u8<M>>;  // DiscreteMatrix scores (score_u8.hpp)
        if constexpr (M >= 2) {
            r.pre2[M] = &launch_scan<score_c32_prefilter2<M>>;
            r.pre2_protein[M] = &launch_scan<score_c32_prefilter2<M, 21>>;
            r.u8_pairs[M] = &score_c32_u8_pairs_launch<M>;
            if constexpr (prefilter2_multi(M) > 1)
                r.pre2_multi[M] = &score_c32_prefilter2_multi_launch<M>;
        }
        fill_c32_row<M, 0>(r.c32[M]);
        // wide alphabets (protein)
        r.prew[M] = &launch_scan<score_c32_prefilter<M, kScorePF, 1>>;
        r.preblk[M] = &launch_scan<score_c32_prefilter_blk<M>>;
        r.u8w[M] = &launch_scan<score_c32_u8<M, kScorePF, 1>>;
        fill_c32_row<M, 1>(r.c32w[M]);
        if constexpr (M < LM_M_HI)
            RegisterRange<M + 1>::run(r);
    }
};

void LM_CAT(register_score_c32_, LM_INST_ID)(const KernelRegistry &r) { RegisterRange<LM_M_LO>::run(r); }

}  // namespace lm
