// seqset_sum.hip -- the total odds of every motif in every record of a resident sequence set: the sum over the record's
// windows of 2^(scale * score), as a double, without a score matrix and without a hit list.  With seqset_best.hip (max
// odds) and seqset_count.hip (total hits) the third statistic of motif-enrichment tools ("sum odds", and over the
// number of windows "average odds"): the affinity of a record for a factor.
//
// The windows of record r are the positions p with p + M <= len(r) (scan.rs:185-190, per RECORD) and each scores as
// `score_into` scores it: M sequential f32 adds from +0.0 in row order (pli/mod.rs:96-105), the score best and count
// see.  A window adds 2^x, x = fl32(scale * v): one f32 multiply (exact for scale 1), then exp2_wide of
// seqset_sum_plan.hpp -- x - rint(x) is exact, one v_exp_f32 on [-1/2, 1/2], a convert, one v_ldexp_f64 -- so that the
// term is right to 1 ulp of f32 over the whole range of a double, and one f64 add.  NaN windows add nothing, -inf
// windows add 0, a +inf window makes the cell +inf.
//
// The walk down the records (Walker), both kernel bodies and the launcher are those of seqset_walk.hpp /
// seqset_walk_launch.hpp; this unit holds the reduction's device half and the fix-up.  A lane keeps ONE f64 accumulator.
// A sum of doubles depends on its order, so the lanes do not meet in an atomic: a record whose windows lie in one lane's
// run is stored by that lane, the others leave a head and a tail per run in the job's scratch and sum_fixup adds them in
// ascending run order (the rules and their arithmetic: seqset_sum_plan.hpp).  The cells are the caller's final doubles:
// one memset before the launches of a group of motifs (cells without a window and the rows of motifs without one keep
// it), one copy back after the fix-up.
#include <cmath>

#include "seqset_sum_plan.hpp"
#include "seqset_walk_launch.hpp"

namespace lm {

namespace setsum {  // (named: tools/kernel_regs.py lists kernels by their demangled names)

struct LaunchLane {  // the lane of the walk: lane L owns column L % cols of stream L / cols (seqset_walk.hpp)
    __device__ __forceinline__ unsigned long long operator()() const { return (unsigned long long)blockIdx.x * kBlock + threadIdx.x; }
};
typedef SumReducerT<LaunchLane> SumReducer;

struct SumJob {
    const float *dense;            // M x K weights, row-major
    unsigned long long slot_base;  // the job's `records` cells (the cells of a group of motifs lie together, as they go home)
    unsigned long long scratch_off;  // doubles from there to the job's { head, tail } per run, behind the group's cells
    const unsigned long long *offsets;
    Geometry geo;
    float scale;
    __device__ __forceinline__ LaunchLane lane_id() const { return LaunchLane(); }
};

template <int M>
__global__ __launch_bounds__(kBlock) void seqset_sum_fused(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned long long rows_total, const unsigned K, const SumJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, double *__restrict__ slots)
{
    walk_fused<M, table_stride(M, 0), SumReducer>(seq, stride, cols, rows, rows_total, K, jobs, g_offsets, n_records, offsets_in_lds, T,
                                                  slots);
}

__global__ __launch_bounds__(kBlock) void seqset_sum_generic(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned M, const unsigned K, const int w_in_lds, const SumJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, double *__restrict__ slots)
{
    walk_generic<SumReducer>(seq, stride, cols, rows, M, K, w_in_lds, jobs, g_offsets, n_records, offsets_in_lds, T, slots);
}

// One thread per (job, record): block b serves records [b % per_job * kBlock, ...) of job b / per_job of the table.
__global__ __launch_bounds__(kBlock) void sum_fixup(const SumJob *__restrict__ jobs, const unsigned per_job, const unsigned long long n_records,
                                                    double *__restrict__ slots)
{
    const unsigned long long r = (unsigned long long)(blockIdx.x % per_job) * kBlock + threadIdx.x;
    if (r >= n_records)
        return;
    const SumJob job = jobs[blockIdx.x / per_job];
    double *cells = slots + job.slot_base;
    double sum;
    if (merge_record(job.geo, cells + job.scratch_off, job.offsets[r], job.offsets[r + 1], &sum))
        cells[r] = sum;
}

struct SumWalk {
    typedef SumJob Job;
    typedef SumReducer::Slot Slot;
    static constexpr const char *kName = "seqset_sum";
    static constexpr int kTally = -1;
    template <int M>
    static constexpr auto fused() { return seqset_sum_fused<M>; }
    static constexpr auto generic() { return seqset_sum_generic; }
};

}  // namespace setsum
using namespace setsum;

}  // namespace lm

using namespace lm;

extern "C" int lm_hip_scan_sum_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *scales, size_t n,
                                      const lm_hip_seqset *set, double *sums)
{
    if (!ctx || !set || (n && !pssms))
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_sum_seqset: null argument");
    for (size_t i = 0; scales && i < n; ++i)
        if (!(std::isfinite(scales[i]) && scales[i] > 0.0f))
            return fail(LM_HIP_ERR_BAD_ARGS, "scan_sum_seqset: scale %zu is %g, a scale is finite and > 0", i, (double)scales[i]);
    std::vector<char> degenerate;
    bool run;
    LM_TRY(check_walk_call("scan_sum_seqset", pssms, n, set, sums, sizeof(double), 0, nullptr, degenerate, &run));
    if (!run)
        return LM_HIP_OK;
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1;
    // The scratch of a job holds the runs of the shortest streams its walk can take: the rows per lane only grow with the
    // jobs of a group.  The jobs of a group are known once the scratch is (it bounds the group), hence the bound first.
    unsigned long long run_cap = 0;
    for (size_t i = 0; i < n; ++i)
        if (!degenerate[i])
            run_cap = std::max(run_cap, runs_of(seq->rows, walk_rows_per_lane(ctx, seq, pssms[i]->m, 1), seq->cols));
    const size_t per_job_slots = slots_per_job(records, run_cap);
    if (per_job_slots > (~(size_t)0 / sizeof(double)))
        return fail(LM_HIP_ERR_CAPACITY, "scan_sum_seqset: %zu records and %llu lane runs overflow a job's block", records, run_cap);
    const size_t group = walk_group_size(n, per_job_slots * sizeof(double));
    std::vector<size_t> live((n + group - 1) / group, 0);  // the jobs launch_walk launches together
    for (size_t i = 0; i < n; ++i)
        live[i / group] += !degenerate[i];
    return launch_walk<SumWalk>(
        ctx, pssms, degenerate.data(), n, set, per_job_slots, per_job_slots * sizeof(double),
        [&](size_t i, unsigned long long) {
            const unsigned long long T = walk_rows_per_lane(ctx, seq, pssms[i]->m, live[i / group]);
            const size_t c0 = i / group * group, nc = std::min(n, c0 + group) - c0, at = i - c0;
            return SumJob{pssms[i]->d_dense, at * records, (nc - at) * records + at * 2 * run_cap, set->d_offsets,
                          Geometry{seq->rows, T, streams_of(seq->rows, T), run_cap, (unsigned)seq->cols, (unsigned)pssms[i]->m},
                          scales ? scales[i] : 1.0f};
        },
        [&](size_t c0, size_t nc, double *d_slots) {
            // the job table of the group lies at the head of the scratch block, its live jobs in front
            const size_t jobs = live[c0 / group];
            const size_t per_job = (records + kBlock - 1) / kBlock;
            if (jobs) {
                hipLaunchKernelGGL(sum_fixup, dim3((unsigned)(per_job * jobs)), dim3(kBlock), 0, ctx->stream,
                                   static_cast<const SumJob *>(ctx->scratch.ptr), (unsigned)per_job, (unsigned long long)records, d_slots);
                LM_HIP_TRY(hipGetLastError());
            }
            LM_HIP_TRY(hipMemcpyAsync(sums + c0 * records, d_slots, nc * records * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            return (int)LM_HIP_OK;
        });
}
