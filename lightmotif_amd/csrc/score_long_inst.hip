// score_long_inst.hip -- the exact f32 kernels for ONE padded motif length LM_LONG_M in {40, 44 ... 64}.
// Compiled once per length (build.py) with -mllvm -pragma-unroll-threshold raised: the M x M step / weight loops
// of a group only become register-indexed accumulators when they unroll completely, and LLVM's default
// budget for `#pragma unroll` (16 K unrolled instructions) ends at M ~ 40 -- past it the accumulators fall into
// scratch (2 564 scratch instructions at M = 40 without the flag, none with it).
#include "score_registry.hpp"

#ifndef LM_LONG_M
#error "LM_LONG_M must be defined"
#endif

namespace lm {

static_assert(LM_LONG_M > kMaxFastM && LM_LONG_M <= kMaxLongM && LM_LONG_M % 4 == 0, "padded long motif length");

// every kernel of this family fetches symbols with dword loads (M % 4 == 0, 4-byte aligned matrix); WIDE: alphabets of
// more than 16 symbols (8-byte LDS reads)
template <int M, int WIDE>
static void fill_long_row(ScoreC32Launcher *tab)
{
    tab[SLOT_STORE] = tab[SLOT_STORE_QL] = &score_c32_launch<M, MODE_STORE, 1, 32, WIDE>;
    tab[SLOT_ARGMAX] = &score_c32_launch<M, MODE_ARGMAX, 1, 32, WIDE>;
    tab[SLOT_THRESHOLD] = &score_c32_launch<M, MODE_THRESHOLD, 1, 32, WIDE>;
    tab[SLOT_STORE_ARGMAX] = &score_c32_launch<M, MODE_STORE_ARGMAX, 1, 32, WIDE>;
    tab[SLOT_CONTINUE] = &score_c32_launch<M, MODE_CONTINUE, 1, 32, WIDE>;
    tab[SLOT_STORE_TRACK] = &score_c32_launch<M, MODE_STORE_TRACK, 1, 32, WIDE>;
}

void LM_CAT(register_score_c32_long_, LM_LONG_M)(const KernelRegistry &r)
{
    constexpr int M = LM_LONG_M;
    fill_long_row<M, 0>(r.c32[M]);
    fill_long_row<M, 1>(r.c32w[M]);
    // the pair-symbol prefilter scan (score_prefilter2.hpp) of the four exact lengths that pad to M: the fused
    // threshold / argmax of 36 < M <= 64 flag candidates with it like the shorter motifs do (DNA)
    r.pre2[M - 3] = &launch_scan<score_c32_prefilter2<M - 3>>;
    r.pre2[M - 2] = &launch_scan<score_c32_prefilter2<M - 2>>;
    r.pre2[M - 1] = &launch_scan<score_c32_prefilter2<M - 1>>;
    r.pre2[M] = &launch_scan<score_c32_prefilter2<M>>;
}

}  // namespace lm
