// seqset_expect.hip -- the expected site counts of every motif over a resident sequence set: the E-step of motif EM
// (MEME's OOPS / ZOOPS), the deterministic form of the sampler's step "score the record, weigh every window by
// 2^(score / temperature), rebuild the count matrix" (sampler.rs:528-538, pwm/mod.rs:209-237; windows per RECORD as
// scan.rs:185-190).  Per motif an M x K table
//       E[j][s] = sum over records r and windows p of z(r, p) * [symbol(r, p + j) == s],   z = min(odds * gain[r], 1)
// in fixed point: the rule, the weight of a window and the run of a lane are seqset_expect_plan.hpp.
//
// The walk down the records is the Walker of seqset_walk.hpp and the launcher that of seqset_walk_launch.hpp (jobs,
// groups of motifs, rows_per_stream, offsets in LDS); the kernel body is this unit's own, because a window's weight goes
// to M cells of a table and not to a slot of its record: seqset_expect_generic is the generic body (a window summed from scratch)
// followed, for a window of non-zero weight, by the scatter of its M symbols.  A workgroup keeps the motif's table as u64
// counters in LDS behind the weights and the offsets (no-return ds_add_u64), and adds its non-zero counters to the
// motif's Q in global memory at the end, one 64-bit integer atomic each; a table that does not fit there adds to global
// memory directly.  The launcher's one memset per group of motifs zeroes Q.  No floating-point atomic anywhere: the
// result is a pure function of (set, matrix, scale, gains).
#include <cmath>

#include "seqset_expect_plan.hpp"
#include "seqset_walk_launch.hpp"

namespace lm {

namespace setexpect {  // (named: tools/kernel_regs.py lists kernels by their demangled names)

struct ExpectJob {
    const float *dense;            // M x K weights, row-major
    unsigned long long slot_base;  // the job's Q table (M x K counters at the head of its slots)
    const double *gains;           // one per record
    float scale;
    double unit;                   // 2^F
};

struct LdsAdd {
    unsigned long long *tab;
    __device__ __forceinline__ void operator()(unsigned cell, unsigned long long q) const { atomicAdd(tab + cell, q); }
};
struct GlobalAdd {
    unsigned long long *tab;
    __device__ __forceinline__ void operator()(unsigned cell, unsigned long long q) const { atomicAdd(tab + cell, q); }
};

__global__ __launch_bounds__(kBlock) void seqset_expect_generic(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned M, const unsigned K, const int w_in_lds, const ExpectJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned long long *__restrict__ slots)
{
    const ExpectJob job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);
    const unsigned wbytes = w_in_lds ? (M * K * 4u + 15u) & ~15u : 0u;
    const unsigned obytes = offsets_in_lds ? ((unsigned)n_records + 1u) * 8u : 0u;
    const unsigned cells = M * K;
    const bool t_in_lds = table_in_lds(wbytes + obytes, M, K);
    unsigned long long *s_tab = reinterpret_cast<unsigned long long *>(s_dyn + wbytes + obytes);
    unsigned long long *q_tab = slots + job.slot_base;
    if (w_in_lds)
        for (unsigned i = threadIdx.x; i < cells; i += kBlock)
            s_w[i] = job.dense[i];
    const unsigned long long *off = stage_offsets(s_dyn + wbytes, g_offsets, n_records, offsets_in_lds);
    if (t_in_lds)
        for (unsigned i = threadIdx.x; i < cells; i += kBlock)
            s_tab[i] = 0;
    __syncthreads();

    const unsigned long long lane = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long col = lane % cols, r0 = (lane / cols) * T;
    if (r0 < rows) {  // (a lane without a run still meets the barrier below)
        const unsigned long long r1 = r0 + T < rows ? r0 + T : rows;
        if (t_in_lds)
            expect_run(seq, stride, rows, col, r0, r1, M, K, s_w, off, n_records, job.gains, job.scale, job.unit, LdsAdd{s_tab});
        else if (w_in_lds)
            expect_run(seq, stride, rows, col, r0, r1, M, K, s_w, off, n_records, job.gains, job.scale, job.unit, GlobalAdd{q_tab});
        else
            expect_run(seq, stride, rows, col, r0, r1, M, K, job.dense, off, n_records, job.gains, job.scale, job.unit, GlobalAdd{q_tab});
    }
    if (!t_in_lds)
        return;  // (uniform over the workgroup)
    __syncthreads();
    for (unsigned i = threadIdx.x; i < cells; i += kBlock) {
        const unsigned long long c = s_tab[i];
        if (c)
            atomicAdd(q_tab + i, c);
    }
}

struct ExpectWalk {
    typedef ExpectJob Job;
    typedef unsigned long long Slot;
    static constexpr const char *kName = "seqset_expect";
    static constexpr int kTally = -1;
    // one body for every motif length (seqset_walk_launch.hpp: a route with `table_lds` has no fused family)
    typedef void (*Fused)(const uint8_t *, unsigned long long, unsigned, unsigned long long, unsigned long long, unsigned, const ExpectJob *,
                          const unsigned long long *, unsigned long long, int, unsigned long long, unsigned long long *);
    template <int M>
    static constexpr Fused fused() { return nullptr; }
    static constexpr auto generic() { return seqset_expect_generic; }
    static size_t table_lds(size_t staged, size_t m, size_t k) { return table_in_lds(staged, m, k) ? m * k * sizeof(unsigned long long) : 0; }
};

}  // namespace setexpect
using namespace setexpect;

}  // namespace lm

using namespace lm;

extern "C" int lm_hip_seqset_expected_counts(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *scales, const double *gains,
                                             size_t n, const lm_hip_seqset *set, double *counts, int *frac_bits)
{
    if (!ctx || !set || (n && !pssms))
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_expected_counts: null argument");
    const size_t records = set->offsets.size() - 1;
    const int F = frac_bits_of(set->offsets.back());
    if (frac_bits)
        *frac_bits = F;
    for (size_t i = 0; scales && i < n; ++i)
        if (!(std::isfinite(scales[i]) && scales[i] > 0.0f))
            return fail(LM_HIP_ERR_BAD_ARGS, "seqset_expected_counts: scale %zu is %g, a scale is finite and > 0", i, (double)scales[i]);
    if (n && records && !gains)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_expected_counts: null gains");
    if (n && records && n > ~(size_t)0 / sizeof(double) / records)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_expected_counts: %zu motifs x %zu records overflow the gains' size", n, records);
    for (size_t i = 0; gains && i < n * records; ++i)
        if (!(std::isfinite(gains[i]) && gains[i] >= 0.0))
            return fail(LM_HIP_ERR_BAD_ARGS, "seqset_expected_counts: the gain of motif %zu in record %zu is %g, a gain is finite and >= 0",
                        i / records, i % records, gains[i]);
    std::vector<char> degenerate;
    bool run;
    LM_TRY(check_walk_call("seqset_expected_counts", pssms, n, set, counts, sizeof(double), 0, nullptr, degenerate, &run));
    if (!run)
        return LM_HIP_OK;
    // the caller's tables, one behind the other
    std::vector<size_t> at(n + 1, 0);
    size_t cap = 1;
    for (size_t i = 0; i < n; ++i) {
        const size_t cells = pssms[i]->m * pssms[i]->k;
        at[i + 1] = at[i] + cells;
        cap = std::max(cap, cells);
    }
    // a job's block on the device: `cap` counters, then its records' gains
    const size_t per_job = (cap + records) * sizeof(double);
    const size_t group = walk_group_size(n, per_job);
    const size_t head = (group * sizeof(ExpectJob) + 255) & ~(size_t)255;  // (launch_walk: the job table in front of the slots)
    const double unit = pow2_of(F), inv = 1.0 / unit;
    std::vector<unsigned long long> q;
    int upload = LM_HIP_OK;
    size_t uploaded = ~(size_t)0;
    return launch_walk<ExpectWalk>(
        ctx, pssms, degenerate.data(), n, set, cap, per_job,
        [&](size_t i, unsigned long long slot_base) {
            // the gains of a group of motifs lie behind the group's tables; they go up with the group's first job
            const size_t c0 = i / group * group, nc = std::min(n, c0 + group) - c0;
            double *d_gains = reinterpret_cast<double *>(static_cast<char *>(ctx->scratch.ptr) + head) + group * cap;
            if (uploaded != c0) {
                uploaded = c0;
                if (hipMemcpyAsync(d_gains, gains + c0 * records, nc * records * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                    upload = LM_HIP_ERR_HIP;
            }
            return ExpectJob{pssms[i]->d_dense, slot_base, d_gains + (i - c0) * records, scales ? scales[i] : 1.0f, unit};
        },
        [&](size_t c0, size_t nc, unsigned long long *d_slots) {
            if (upload != LM_HIP_OK)
                return fail(upload, "seqset_expected_counts: the gains did not reach the device");
            q.resize(nc * cap);
            LM_HIP_TRY(hipMemcpyAsync(q.data(), d_slots, nc * cap * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (size_t i = c0; i < c0 + nc; ++i)  // (a degenerate motif: the memset's zeros)
                for (size_t c = 0; c < at[i + 1] - at[i]; ++c)
                    counts[at[i] + c] = (double)q[(i - c0) * cap + c] * inv;
            return (int)LM_HIP_OK;
        });
}
