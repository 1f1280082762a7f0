// score_argmax_exact.hip -- the exact route of the fused argmax: the scoring kernels leave per-workgroup records; plan,
// enqueue the groups, deliver (argmax_plan.hpp: Delivery).
#include <cstring>

#include "argmax_plan.hpp"
#include "score_launch.hpp"

namespace lm {

// Final reduction of per-block records; also applies the reference's "scores[0]
// is NaN -> (0,0)" rule (pli/mod.rs:142,146: nothing ever compares >= NaN).  In
// the fused path scores[0][0] does not exist in memory, so it is recomputed here.
__global__ __launch_bounds__(kBlock) void argmax_finalize(
    const ArgmaxRecord *__restrict__ blocks, const unsigned nblocks,
    const float *__restrict__ scores00,  // non-null: materialised scores
    const uint8_t *__restrict__ seq00, const unsigned long long seq_stride,
    const float *__restrict__ pssm, const int M, const int K, const int first_cell_rule,
    ArgmaxRecord *__restrict__ out)
{
    __shared__ float sm_v[kBlock / 64];
    __shared__ long long sm_i[kBlock / 64];
    float v = -INFINITY;
    long long i = -1;
    for (unsigned b = threadIdx.x; b < nblocks; b += kBlock)
        if (blocks[b].found)
            best_merge(v, i, blocks[b].value, blocks[b].index);
    best_block_reduce(v, i, sm_v, sm_i);
    if (threadIdx.x == 0 && first_cell_rule) {
        float first;
        if (scores00) {
            first = scores00[0];
        } else {
            first = 0.0f;
            for (int j = 0; j < M; ++j)
                first = first + pssm[j * K + seq00[j * seq_stride]];
        }
        if (first != first) {  // NaN
            v = first;
            i = 0;
        }
    }
    if (threadIdx.x == 0) {
        out->value = v;
        out->index = i;
        out->found = i >= 0;
    }
}

// One entry per job of a batch: where its block records are and how to recompute its
// scores[0][0] (first-cell rule).
struct FinalizeJob {
    const ArgmaxRecord *blocks;
    unsigned nblocks;
    int M, K;
    const uint8_t *seq00;
    unsigned long long seq_stride;
    const float *pssm;
};

// grid = number of jobs: block j reduces the block records of job j.
__global__ __launch_bounds__(kBlock) void argmax_finalize_batch(const FinalizeJob *__restrict__ jobs,
                                                                const int first_cell_rule,
                                                                ArgmaxRecord *__restrict__ out)
{
    __shared__ float sm_v[kBlock / 64];
    __shared__ long long sm_i[kBlock / 64];
    const FinalizeJob job = jobs[blockIdx.x];
    float v = -INFINITY;
    long long i = -1;
    for (unsigned b = threadIdx.x; b < job.nblocks; b += kBlock)
        if (job.blocks[b].found)
            best_merge(v, i, job.blocks[b].value, job.blocks[b].index);
    best_block_reduce(v, i, sm_v, sm_i);
    if (threadIdx.x == 0) {
        if (first_cell_rule) {
            float first = 0.0f;
            for (int j = 0; j < job.M; ++j)
                first = first + job.pssm[j * job.K + job.seq00[j * job.seq_stride]];
            if (first != first) {  // NaN (pli/mod.rs:142-146)
                v = first;
                i = 0;
            }
        }
        out[blockIdx.x].value = v;
        out[blockIdx.x].index = i;
        out[blockIdx.x].found = i >= 0;
    }
}

static_assert(sizeof(ArgmaxRecord) == argmax::kRecordBytes && sizeof(FinalizeJob) == argmax::kFinalizeJobBytes && sizeof(uint4) == 16 &&
                  kBlock == argmax::kPlanBlock && kPinArgmaxBatch.cap == argmax::kPinBatchBytes && kPinFoldRecords.cap == argmax::kPinFoldBytes,
              "argmax_plan.hpp repeats these sizes and the capacities of the pinned regions");
static_assert(argmax::pinned_jobs_off(1) >= kPinRecord.end() && argmax::pinned_jobs_off(1) + sizeof(FinalizeJob) <= kPinFoldRecords.off,
              "single-job argmax: the job table lies between the record with its generation word and the wavefront records");

// One small job off the C = 32 kernels (C = 1 is the Generic geometry of the reference's own bench, dna.rs:112-116):
// ONE launch.  The tiled store kernel scores into the chunk buffer and leaves a (value, cell) record per workgroup
// in the pinned block, folded here -- what score_into + argmax on handles do (27 us per iteration of configs[0]);
// the chunked route takes a store, a reduction and a finalize launch (41 us).  *done = false: the shape is not this
// route's, or the kernel left no records (the stream is then quiescent) -- the planned route below takes the job.
// (C = 16 has an unrolled store kernel of its own, which leaves no records; the cheap conditions come first)
static int argmax_tiled_host_fold(lm_hip_ctx *ctx, const ScoreArgs &a, int first_cell_rule, ArgmaxRecord *out, bool *done)
{
    *done = false;
    if (!ctx->host_fold || a.cols == 32 || a.cols == 16 || !chunked_ok(ctx, a) || plan_c32(ctx, a, false).ok)
        return LM_HIP_OK;
    const unsigned long long rows = a.row_end - a.row_begin;
    const unsigned nrec = tiled_records(ctx, a);
    if (!nrec || rows > chunk_rows_for(ctx, a) || rows * a.cols >= (1ull << 32) || !pinned_at<uint4>(ctx, kPinFoldRecords, (size_t)nrec + 1))
        return LM_HIP_OK;
    LM_TRY(ctx->chunk_scores.reserve(rows * a.cols * sizeof(float)));
    const FoldSlots fold = begin_fold(ctx, nrec);
    unsigned written = 0;
    ScoreArgs t = a;
    t.d_out = static_cast<float *>(ctx->chunk_scores.ptr);
    t.out_stride = a.cols;
    t.track_records = fold.records;
    t.track_generation = fold.generation;
    t.track_cap = (size_t)nrec + 1;
    t.track_nrec = &written;
    LM_TRY(launch_score_store(ctx, t));
    if (!written) {
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // (no records after all: the general route, buffer quiescent)
        return LM_HIP_OK;
    }
    ctx->last_kernel = "score_tiled+host_fold";
    *done = true;
    return fold_host_records(ctx, fold.records, written, fold.generation, first_cell_rule != 0, out);
}

// An exact argmax call of n jobs as planned.  (In place: a single short scan is launch-latency bound, and the two staged
// copies of table and results were a third of its wall time.)
struct ExactCall {
    std::vector<JobGroup> groups;
    ScanPlan sp;
    std::vector<unsigned> grids;    // records (workgroups) of job i ...
    std::vector<size_t> block_pos;  // ... starting at blocks[block_pos[i]]
    argmax::Delivery form;
    ArgmaxRecord *blocks;
    ArgmaxRecord *results;  // [n], where the kernels write them; at n = 1 the generation word follows results[0]
    FinalizeJob *d_jobs;    // [n], where the finalize kernel reads the table
    FinalizeJob *fj;        // [n], where the host fills it in (in place: d_jobs itself)
    std::vector<FinalizeJob> fj_heap;
    FoldSlots fold{nullptr, 0};  // one launch: its generation; HostFoldRecords: the wavefronts' records in the pinned block
    size_t wave_records = 0;     // one launch: wavefronts of the kernel
};

static int plan_exact(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, ExactCall *c)
{
    c->groups = group_jobs(ctx, jobs, n, [&](size_t i) {
        return plan_c32(ctx, jobs[i], false).ok ? KIND_EXACT : chunked_ok(ctx, jobs[i]) ? KIND_CHUNKED : KIND_GENERIC;
    });
    c->sp = plan_scans(ctx, jobs, n, c->groups, false);  // (exact kernels only: nothing is padded or dropped)
    record_scan_shape(ctx, c->sp, c->groups, jobs, n);
    c->grids.resize(n);
    for (const JobGroup &g : c->groups)
        for (size_t i : g.idx) {
            const unsigned long long ncells =
                (unsigned long long)(jobs[i].row_end - jobs[i].row_begin) * jobs[i].cols;
            c->grids[i] = g.kind == KIND_GENERIC   ? generic_grid(ctx, ncells).x
                          : g.kind == KIND_CHUNKED ? (unsigned)(chunk_count(ctx, jobs[i]) * chunk_argmax_grid(ctx))
                                                   : g.plan.grid.x;
        }
    c->block_pos.resize(n);
    size_t total_blocks = 0;
    for (size_t i = 0; i < n; total_blocks += c->grids[i++])
        c->block_pos[i] = total_blocks;
    const argmax::ExactScratch lay = argmax::exact_scratch(n, total_blocks);
    LM_TRY(ctx->scratch.reserve(lay.bytes));
    char *base = static_cast<char *>(ctx->scratch.ptr);
    c->blocks = reinterpret_cast<ArgmaxRecord *>(base + lay.off_blocks);
    const bool zero_copy = argmax::exact_zero_copy(n);
    if (zero_copy) {
        c->d_jobs = c->fj = pinned_at<FinalizeJob>(ctx, kPinArgmaxBatch, n, argmax::pinned_jobs_off(n));
        c->results = pinned_at<ArgmaxRecord>(ctx, kPinArgmaxBatch, n);
    } else {
        c->results = reinterpret_cast<ArgmaxRecord *>(base + lay.off_results);
        c->d_jobs = reinterpret_cast<FinalizeJob *>(base + lay.off_jobs);
        c->fj_heap.resize(n);
        c->fj = c->fj_heap.data();
    }
    const JobGroup &g0 = c->groups[0];
    const ScoreArgs &a0 = jobs[g0.idx[0]];
    c->wave_records = g0.kind == KIND_EXACT ? (size_t)g0.plan.grid.x * (kBlock / 64) : 0;
    c->form = argmax::pick_delivery(n, c->groups.size(), g0.kind == KIND_EXACT, zero_copy, ctx->host_fold,
                                    (unsigned long long)(a0.row_end - a0.row_begin) * a0.cols, c->wave_records);
    return LM_HIP_OK;
}

// the scoring kernels back to back, each leaving per-workgroup records in its own region (a group's jobs: by BatchParams)
static int enqueue_groups(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, int first_cell_rule, ExactCall &c)
{
    std::vector<BatchParams> bparams;  // in launch order: the jobs of a group are contiguous
    BatchParams *d_bparams = nullptr;
    if (n > 1) {
        bparams.reserve(n);
        for (size_t gi = 0; gi < c.groups.size(); ++gi)
            for (size_t i : c.groups[gi].idx)
                bparams.push_back(BatchParams{scan_table(c.sp, gi, c.groups[gi].kind, jobs[i]), c.blocks + c.block_pos[i], 0.0f, 0u, 0ull});
        LM_TRY(ctx->scratch2.reserve(sizeof(BatchParams) * n));
        d_bparams = static_cast<BatchParams *>(ctx->scratch2.ptr);
        LM_HIP_TRY(hipMemcpyAsync(d_bparams, bparams.data(), sizeof(BatchParams) * n,
                                  hipMemcpyHostToDevice, ctx->stream));
    }
    BatchStreams streams(ctx, c.groups.size());
    LM_TRY(streams.fork());
    const bool one_launch = c.form == argmax::Delivery::HostFoldRecords || c.form == argmax::Delivery::PolledRecord;
    if (one_launch)
        LM_TRY(ensure_ticket(ctx));
    for (size_t gi = 0; gi < c.groups.size(); ++gi) {
        const JobGroup &g = c.groups[gi];
        const ScoreArgs &a = jobs[g.idx[0]];
        hipStream_t st = streams.next();
        FusedOut fo{};
        fo.block_best = c.blocks + c.block_pos[g.idx[0]];
        if (one_launch) {
            // the last workgroup folds the records and writes the result straight into the pinned block, or (HostFoldRecords)
            // the wavefronts' records go there unfolded
            c.fold = begin_fold(ctx, c.wave_records, c.form == argmax::Delivery::HostFoldRecords);
            fo.ticket = ctx->d_ticket;
            fo.final_out = reinterpret_cast<ArgmaxRecord *>(ctx->d_ticket + 4);  // device copy nobody reads: 16 spare bytes
            fo.final_host = c.results;                                           // pinned: record, then the generation word
            fo.generation = c.fold.generation;
            *pinned_at<volatile unsigned>(ctx, kPinRecord, 1, kPinGenerationWordOff) = 0u;  // (the block is shared staging: no stale match)
            fo.first_cell_rule = first_cell_rule;
            fo.host_records = c.fold.records;
        }
        if (g.kind == KIND_EXACT) {
            fo.batch = n > 1 ? d_bparams + c.sp.groups[gi].pos : nullptr;
            LM_TRY(launch_group_scan(ctx, c.sp, gi, g, a, MODE_ARGMAX, 0u, st, fo));
        } else if (g.kind == KIND_CHUNKED) {
            // (always on ctx->stream: the chunk buffer is shared)
            const unsigned cg = chunk_argmax_grid(ctx);
            ArgmaxRecord *recs = fo.block_best;
            const unsigned long long per = chunk_rows_for(ctx, a);
            LM_TRY(for_each_scored_chunk(ctx, a, [&](const float *buf, unsigned long long c0, unsigned long long rows) {
                return launch_argmax_blocks_flat(ctx, ctx->stream, buf, rows * a.cols, (long long)(c0 * a.cols), cg,
                                                 recs + (c0 / per) * cg);
            }));
        } else {
            ctx->last_kernel = "score_generic<1>";
            LM_TRY(launch_generic<MODE_ARGMAX>(ctx, a, fo, dim3(c.grids[g.idx[0]]), st));
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const ScoreArgs &a = jobs[i];
        c.fj[i] = FinalizeJob{c.blocks + c.block_pos[i], c.grids[i], (int)a.pssm->m, (int)a.pssm->k,
                              a.d_seq + a.row_begin * a.seq_stride,
                              (unsigned long long)a.seq_stride, a.pssm->d_dense};
    }
    return streams.join();
}

// the kernel raises the generation word behind the pinned record: poll it (bounded, then synchronise), not the completion signal
static int deliver_polled_record(lm_hip_ctx *ctx, const ExactCall &c, ArgmaxRecord *out)
{
    if (!poll_generation(pinned_at<volatile unsigned>(ctx, kPinRecord, 1, kPinGenerationWordOff), c.fold.generation))
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, c.results, sizeof(ArgmaxRecord));
    return LM_HIP_OK;
}

// ONE finalize launch reduces every job and ONE synchronisation returns; `staged`: table and results travel by copies
static int deliver_by_finalize(lm_hip_ctx *ctx, const ExactCall &c, size_t n, int first_cell_rule, bool staged, ArgmaxRecord *out)
{
    if (staged)
        LM_HIP_TRY(hipMemcpyAsync(c.d_jobs, c.fj, sizeof(FinalizeJob) * n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(argmax_finalize_batch, dim3((unsigned)n), dim3(kBlock), 0, ctx->stream, c.d_jobs, first_cell_rule, c.results);
    LM_HIP_TRY(hipGetLastError());
    if (staged)
        LM_HIP_TRY(hipMemcpyAsync(out, c.results, sizeof(ArgmaxRecord) * n, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // also keeps `fj` alive long enough
    if (!staged)
        memcpy(out, c.results, sizeof(ArgmaxRecord) * n);
    return LM_HIP_OK;
}

// Fused score+argmax of `n` independent jobs (one motif each) through the exact kernels.
int launch_score_argmax_exact(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, int first_cell_rule, ArgmaxRecord *out)
{
    if (n == 0)
        return LM_HIP_OK;
    if (n == 1) {
        bool done = false;
        LM_TRY(argmax_tiled_host_fold(ctx, jobs[0], first_cell_rule, out, &done));
        if (done)
            return LM_HIP_OK;
    }
    ExactCall c;
    LM_TRY(plan_exact(ctx, jobs, n, &c));
    LM_TRY(enqueue_groups(ctx, jobs, n, first_cell_rule, c));
    switch (c.form) {
    case argmax::Delivery::HostFoldRecords:
        return fold_host_records(ctx, c.fold.records, (unsigned)c.wave_records, c.fold.generation, first_cell_rule != 0, out);
    case argmax::Delivery::PolledRecord:
        return deliver_polled_record(ctx, c, out);
    default:  // FinalizeInPlace, FinalizeStaged
        return deliver_by_finalize(ctx, c, n, first_cell_rule, c.form == argmax::Delivery::FinalizeStaged, out);
    }
}

}  // namespace lm

