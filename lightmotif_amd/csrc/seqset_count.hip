// seqset_count.hip -- how many windows of every motif in every record of a resident sequence set reach a cut-off, at up
// to LM_HIP_MAX_COUNT_LEVELS cut-offs per motif, without a score matrix and without a hit list.
//
// The reference's CLI would collect the hits of every (motif, record) job (main.rs:502-561) and the caller would count
// them; the question itself needs no list.  The windows of record r are the positions p with p + M <= len(r)
// (scan.rs:185-190, per RECORD) and each scores as `score_into` scores it: M sequential f32 adds from +0.0 in row order
// (pli/mod.rs:96-105).  A window counts at level l when `score >= t[l]` under f32 comparison: NaN windows and NaN
// thresholds count nothing, -inf windows count at a threshold of -inf alone.
//
// The walk down the records (Walker), seqset_count_generic's body and the launcher are those of seqset_walk.hpp /
// seqset_walk_launch.hpp; this unit holds the reduction, and the body of seqset_count_fused<M> (see there).  A lane keeps
// LM_HIP_MAX_COUNT_LEVELS 32-bit counters in registers; the loop over levels is unrolled to that constant and the levels a
// call does not use carry a NaN threshold, so nothing is indexed dynamically.  At a record's end and at the end of its
// run a lane adds every non-zero counter to its cell
//       slots[(job * levels + level) * records + record]
// with one 32-bit atomicAdd whose result nobody reads.  Integer addition is associative and commutative, so the cells do
// not depend on the order in which the lanes arrive: the answer is deterministic.  The cells are the caller's final
// uint32_t values: one memset before the launches of a group of motifs, one copy back after them, no finalize kernel.
#include <cmath>

#include "seqset_walk_launch.hpp"

namespace lm {

namespace setcount {  // (named: tools/kernel_regs.py lists kernels by their demangled names)

constexpr int kLevels = LM_HIP_MAX_COUNT_LEVELS;

struct CountJob {
    const float *dense;             // M x K weights, row-major
    unsigned long long slot_base;   // first cell of the job: slots[slot_base + level * records + record]
    float t[kLevels];               // cut-offs; NaN: level not in use
};

struct CountReducer {
    typedef unsigned Slot;
    float t[kLevels];
    unsigned c[kLevels];  // windows of the current record counted by this lane and not yet added to the cells

    __device__ __forceinline__ void begin(const CountJob &job)
    {
#pragma unroll
        for (int l = 0; l < kLevels; ++l) {
            t[l] = job.t[l];
            c[l] = 0;
        }
    }
    __device__ __forceinline__ void window(unsigned long long, float v, bool inside)
    {
#pragma unroll
        for (int l = 0; l < kLevels; ++l)
            c[l] += (inside && v >= t[l]) ? 1u : 0u;  // false for a NaN score and for a NaN threshold
    }
    __device__ __forceinline__ void flush(Slot *slots, unsigned long long rec, unsigned long long, unsigned long long n)
    {
#pragma unroll
        for (int l = 0; l < kLevels; ++l)
            if (c[l]) {
                atomicAdd(slots + (unsigned long long)l * n + rec, c[l]);
                c[l] = 0;
            }
    }
};

// The text of walk_fused<M, TS, CountReducer> (seqset_walk.hpp; comments there), kept in the kernel: as a call the compiler
// optimises the body on its own before it inlines it, and seqset_count_fused<17> then takes 97 VGPRs instead of 96, one
// wavefront per SIMD less.
template <int M>
__global__ __launch_bounds__(kBlock) void seqset_count_fused(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned long long rows_total, const unsigned K, const CountJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned *__restrict__ slots)
{
    constexpr int TS = table_stride(M, 0);
    constexpr int MP = 4 * ((M + 3) / 4);
    const CountJob job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);
    const unsigned wbytes = (K * TS * 4u + 15u) & ~15u;
    for (unsigned i = threadIdx.x; i < K * TS; i += kBlock) {
        const unsigned s = i / TS, j = i % TS;
        s_w[i] = j < (unsigned)M ? job.dense[j * K + s] : 0.0f;
    }
    Walker<CountReducer> wk;
    wk.off = stage_offsets(s_dyn + wbytes, g_offsets, n_records, offsets_in_lds);
    __syncthreads();

    const unsigned long long lane = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long col = lane % cols, r0 = (lane / cols) * T;
    if (r0 >= rows)
        return;
    const unsigned long long r1 = r0 + T < rows ? r0 + T : rows;
    wk.n = n_records;
    wk.m = M;
    wk.slots = slots + job.slot_base;
    wk.begin(col * rows + r0, job);

    const unsigned long long total = (r1 - r0) + (M - 1);
    const long long base = (long long)(col * rows + r0) - (M - 1);
    const unsigned long long last_row = rows_total - 1;
    const uint8_t *sp = seq + col;
    float acc[M];
#pragma unroll
    for (int j = 0; j < M; ++j)
        acc[j] = 0.0f;
    for (unsigned long long g = 0; g < total; g += M) {
        unsigned sym[M];
#pragma unroll
        for (int s = 0; s < M; ++s) {
            const unsigned long long row = r0 + g + s;
            sym[s] = sp[(row < last_row ? row : last_row) * stride];
        }
        float w[2][MP];
        fetch_weights<MP>(w[0], s_w + sym[0] * TS);
#pragma unroll
        for (int s = 0; s < M; ++s) {
            if (s + 1 < M)
                fetch_weights<MP>(w[(s + 1) & 1], s_w + sym[s + 1] * TS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < M; ++j)
                acc[(s - j + M) % M] = acc[(s - j + M) % M] + w[s & 1][j];
#pragma unroll
            for (int j = 0; j < M; ++j)
                asm volatile("" : "+v"(acc[j]));
            const unsigned long long t = g + s;
            const float v = acc[(s + 1) % M];
            acc[(s + 1) % M] = 0.0f;
            wk.take((unsigned long long)(base + (long long)t), v, t >= (unsigned long long)(M - 1) && t < total);
        }
    }
    wk.flush();
}

__global__ __launch_bounds__(kBlock) void seqset_count_generic(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned M, const unsigned K, const int w_in_lds, const CountJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned *__restrict__ slots)
{
    walk_generic<CountReducer>(seq, stride, cols, rows, M, K, w_in_lds, jobs, g_offsets, n_records, offsets_in_lds, T, slots);
}

struct CountWalk {
    typedef CountJob Job;
    typedef CountReducer::Slot Slot;
    static constexpr const char *kName = "seqset_count";
    static constexpr int kTally = -1;
    template <int M>
    static constexpr auto fused() { return seqset_count_fused<M>; }
    static constexpr auto generic() { return seqset_count_generic; }
};

}  // namespace setcount
using namespace setcount;

}  // namespace lm

using namespace lm;

extern "C" int lm_hip_scan_count_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds, size_t levels,
                                        size_t n, const lm_hip_seqset *set, uint32_t *counts)
{
    if (!ctx || !set || (n && (!pssms || !thresholds)))
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_count_seqset: null argument");
    if (levels < 1 || levels > (size_t)LM_HIP_MAX_COUNT_LEVELS)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_count_seqset: %zu levels, a call takes 1 ... %d", levels, LM_HIP_MAX_COUNT_LEVELS);
    std::vector<char> degenerate;
    bool run;
    LM_TRY(check_walk_call("scan_count_seqset", pssms, n, set, counts, sizeof(uint32_t) * levels, levels, "a cell counts to", degenerate, &run));
    if (!run)
        return LM_HIP_OK;
    const size_t cells = levels * (set->offsets.size() - 1);  // of a job
    return launch_walk<CountWalk>(
        ctx, pssms, degenerate.data(), n, set, cells, cells * sizeof(uint32_t),
        [&](size_t i, unsigned long long slot_base) {
            CountJob job{pssms[i]->d_dense, slot_base, {}};
            for (size_t l = 0; l < (size_t)kLevels; ++l)
                job.t[l] = l < levels ? thresholds[i * levels + l] : std::nanf("");
            return job;
        },
        [&](size_t c0, size_t nc, unsigned *d_slots) {
            LM_HIP_TRY(hipMemcpyAsync(counts + c0 * cells, d_slots, nc * cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            return (int)LM_HIP_OK;
        });
}
