// seqset_best.hip -- the best window of every motif in every record of a resident sequence set, without a score
// matrix and without a hit list: a scan whose reduction is segmented by record.
//
// The README of the reference shows the question for ONE sequence (`pssm.score(&striped).argmax()`, scores.rs:190-192)
// and its CLI would ask it once per (motif, record) job (main.rs:502-561).  Here the records lie end to end in one
// StripedSequence (seqset.hip); the windows of record r are positions p with p + M <= len(r) (scan.rs:185-190, per
// RECORD) and each scores as `score_into` scores it: M sequential f32 adds from +0.0 in row order (pli/mod.rs:96-105).
//
// The walk down the records, the kernel bodies (seqset_best_fused<M> for M <= kMaxFastM, seqset_best_generic for any M)
// and the launcher are those of seqset_walk.hpp / seqset_walk_launch.hpp; this unit holds the reduction.  A lane keeps a
// running (score, position); at a record's end and at the end of its run it MERGES its partial into slot (job, record)
// with one 64-bit atomicMax on
//       order-preserving map of the f32 bits << 32 | 0xFFFFFFFF - position in the record
// so the greatest score wins and, among equal scores, the lowest position: the merge is order-independent and the answer
// deterministic.  NaN windows never compete, -inf windows do; a slot nobody merged into stays 0 ("none": no valid key is
// 0).  seqset_best_finalize turns slots into lm_hip_set_best.
#include "seqset_walk_launch.hpp"

namespace lm {

namespace best {  // (named: tools/kernel_regs.py lists kernels by their demangled names)

struct BestJob {
    const float *dense;             // M x K weights, row-major
    unsigned long long slot_base;   // first slot of the job: slots[slot_base + record]
};

__device__ __forceinline__ unsigned ordered_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered_bits(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

struct BestReducer {
    typedef unsigned long long Slot;
    float best;  // NaN: none yet
    unsigned long long best_pos;

    __device__ __forceinline__ void begin(const BestJob &)
    {
        best = __uint_as_float(0x7FC00000u);
        best_pos = 0;
    }
    __device__ __forceinline__ void window(unsigned long long p, float v, bool inside)
    {
        if (inside && v == v && !(v <= best)) {  // strictly greater, or the first: the lowest position of a tie stays
            best = v;
            best_pos = p;
        }
    }
    __device__ __forceinline__ void flush(Slot *slots, unsigned long long rec, unsigned long long start, unsigned long long)
    {
        if (best == best) {
            const unsigned long long key = ((unsigned long long)ordered_bits(best) << 32) |
                                           (unsigned long long)(0xFFFFFFFFu - (unsigned)(best_pos - start));
            atomicMax(slots + rec, key);
            best = __uint_as_float(0x7FC00000u);
        }
    }
};

template <int M>
__global__ __launch_bounds__(kBlock) void seqset_best_fused(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned long long rows_total, const unsigned K, const BestJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned long long *__restrict__ slots)
{
    walk_fused<M, table_stride(M, 0), BestReducer>(seq, stride, cols, rows, rows_total, K, jobs, g_offsets, n_records, offsets_in_lds, T,
                                                   slots);
}

__global__ __launch_bounds__(kBlock) void seqset_best_generic(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned M, const unsigned K, const int w_in_lds, const BestJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned long long *__restrict__ slots)
{
    walk_generic<BestReducer>(seq, stride, cols, rows, M, K, w_in_lds, jobs, g_offsets, n_records, offsets_in_lds, T, slots);
}

__global__ __launch_bounds__(kBlock) void seqset_best_finalize(const unsigned long long *__restrict__ slots,
                                                               const unsigned long long count, lm_hip_set_best *__restrict__ out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count)
        return;
    const unsigned long long key = slots[i];
    lm_hip_set_best b;
    b.found = key != 0;
    b.position = key ? (unsigned long long)(0xFFFFFFFFu - (unsigned)key) : 0ull;
    b.score = key ? unordered_bits((unsigned)(key >> 32)) : __uint_as_float(0x7FC00000u);
    out[i] = b;
}

struct BestWalk {
    typedef BestJob Job;
    typedef BestReducer::Slot Slot;
    static constexpr const char *kName = "seqset_best";
    static constexpr int kTally = LM_HIP_FAMILY_BEST_FUSED;
    template <int M>
    static constexpr auto fused() { return seqset_best_fused<M>; }
    static constexpr auto generic() { return seqset_best_generic; }
};

}  // namespace best
using namespace best;

const void *seqset_best_fused_row(int M)
{
    return (M >= 1 && M <= kMaxFastM) ? reinterpret_cast<const void *>(WalkKernels<BestWalk>::get().fn[M]) : nullptr;
}

}  // namespace lm

using namespace lm;

extern "C" int lm_hip_scan_best_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const lm_hip_seqset *set,
                                       lm_hip_set_best *best)
{
    if (!ctx || !set || (n && !pssms))
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_best_seqset: null argument");
    std::vector<char> degenerate;
    bool run;
    LM_TRY(check_walk_call("scan_best_seqset", pssms, n, set, best, sizeof(lm_hip_set_best), 0, "the merge addresses", degenerate, &run));
    if (!run)
        return LM_HIP_OK;
    const size_t records = set->offsets.size() - 1;  // a job: its slots, then its results
    return launch_walk<BestWalk>(
        ctx, pssms, degenerate.data(), n, set, records, records * (sizeof(unsigned long long) + sizeof(lm_hip_set_best)),
        [&](size_t i, unsigned long long slot_base) { return BestJob{pssms[i]->d_dense, slot_base}; },
        [&](size_t c0, size_t nc, unsigned long long *d_slots) {
            const unsigned long long count = (unsigned long long)nc * records;
            lm_hip_set_best *d_out = reinterpret_cast<lm_hip_set_best *>(d_slots + count);
            hipLaunchKernelGGL(seqset_best_finalize, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, d_slots,
                               count, d_out);
            LM_HIP_TRY(hipGetLastError());
            LM_HIP_TRY(hipMemcpyAsync(best + c0 * records, d_out, count * sizeof(lm_hip_set_best), hipMemcpyDeviceToHost, ctx->stream));
            return (int)LM_HIP_OK;
        });
}
