// seqset_walk_launch.hpp -- the host half of the record walk (seqset_walk.hpp): the table of a route's fused kernels, the
// rows a lane walks, the launcher and the checks of an entry point, once for seqset_best.hip, seqset_count.hip and
// seqset_sum.hip, and for seqset_expect.hip.
//
// A route describes itself with a struct W: Job (an entry of the job table, { dense, slot_base, ... }), Slot (what the
// kernels merge into), kName ("seqset_best": the kernels are <kName>_fused<M> and <kName>_generic), kTally (registry family
// tallied per fused launch, -1: none), fused<M>() and generic() (the __global__ functions).  A route that keeps a table
// of its own in LDS behind the weights and the offsets declares table_lds(staged bytes, m, k), the bytes of it (0: it
// does not fit); such a route has one body, the generic one, for every motif length (seqset_expect.hip).
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "score_launch.hpp"
#include "seqset_walk.hpp"

namespace lm {

template <typename W, typename = void>
struct WalkTable {
    static constexpr bool kOwn = false;
    static size_t lds(size_t, size_t, size_t) { return 0; }
};
template <typename W>
struct WalkTable<W, std::void_t<decltype(&W::table_lds)>> {
    static constexpr bool kOwn = true;
    static size_t lds(size_t staged, size_t m, size_t k) { return W::table_lds(staged, m, k); }
};

template <typename W>
struct WalkKernels {
    typedef decltype(W::template fused<1>()) Fused;
    Fused fn[kMaxFastM + 1] = {};
    char name[kMaxFastM + 1][32] = {};
    char generic_name[32];
    template <int M>
    void fill()
    {
        fn[M] = W::template fused<M>();
        snprintf(name[M], sizeof name[M], "%s_fused<%d>", W::kName, M);
        if constexpr (M > 1)
            fill<M - 1>();
    }
    WalkKernels()
    {
        fill<kMaxFastM>();
        snprintf(generic_name, sizeof generic_name, "%s_generic", W::kName);
    }
    static const WalkKernels &get()
    {
        static const WalkKernels k;
        return k;
    }
};

constexpr size_t kWalkBlockBytes = (size_t)256 << 20;  // slots (and results) of one group of motifs on the device

// Rows per lane: long enough that the M - 1 fill steps of a run cost little, short enough that the `njobs` jobs of the
// call put a few wavefronts on every SIMD.
static inline unsigned long long walk_rows_per_lane(const lm_hip_ctx *ctx, const lm_hip_seq *seq, size_t m, size_t njobs)
{
    if (ctx->rows_per_stream)
        return ctx->rows_per_stream;
    const unsigned long long cells = (unsigned long long)seq->rows * seq->cols * njobs;
    const unsigned long long lanes = (unsigned long long)ctx->num_cus * 512;
    return std::min<unsigned long long>(std::max<unsigned long long>({4ull * m, cells / lanes, 16ull}), 4096ull);
}

// Motifs of one group: what launch_walk runs between two copies home (a route whose jobs depend on the group asks too).
static inline size_t walk_group_size(size_t n, size_t per_job)
{
    return std::max<size_t>(1, std::min<size_t>(n, kWalkBlockBytes / std::max<size_t>(per_job, 1)));
}

// What an entry point checks behind its own null arguments, in `call`'s name (`degenerate`: the motif has no window in
// the set; `cell_bytes` per (motif, record); `levels`: 0 where the call has none; `limit`: what 32 bits of a record's
// length bound in this route, null where nothing does).  *run: there is something to launch.
static inline int check_walk_call(const char *call, const lm_hip_pssm *const *pssms, size_t n, const lm_hip_seqset *set, const void *result,
                                  size_t cell_bytes, size_t levels, const char *limit, std::vector<char> &degenerate, bool *run)
{
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1;
    *run = false;
    if (n && records && !result)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: null result array", call);
    degenerate.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {  // as lm_hip_scan_threshold_seqset: alphabet, then wrap (avx2.rs:832-837)
        if (pssms[i])
            LM_TRY(check_alphabet(call, pssms[i]->k, seq));
        LM_TRY(check_score_args(pssms[i], seq->rows + seq->wrap, seq->stride, seq->cols, seq->wrap, 0, seq->rows));
        degenerate[i] = seq->length < pssms[i]->m || seq->rows == 0 || pssms[i]->m == 0;  // pli/mod.rs:85-88: no scores
    }
    if (n == 0 || records == 0)
        return LM_HIP_OK;
    if (limit && seq->length >> 32)
        for (size_t r = 0; r < records; ++r)
            if ((set->offsets[r + 1] - set->offsets[r]) >> 32)
                return fail(LM_HIP_ERR_CAPACITY, "%s: record %zu holds %llu symbols, %s 2^32 - 1", call, r,
                            (unsigned long long)(set->offsets[r + 1] - set->offsets[r]), limit);
    if (records > (~(size_t)0 / cell_bytes) / n)
        return levels ? fail(LM_HIP_ERR_CAPACITY, "%s: %zu motifs x %zu levels x %zu records overflow the result's size", call, n, levels, records)
                      : fail(LM_HIP_ERR_CAPACITY, "%s: %zu motifs x %zu records overflow the result's size", call, n, records);
    *run = true;
    return LM_HIP_OK;
}

// The launches of a call, under the context's lock.  A job owns `slots_per_job` slots and `per_job` bytes of the scratch
// block; more than kWalkBlockBytes run in groups of motifs.  make_job(i, slot_base): the table entry of motif i;
// after(c0, nc, d_slots), behind the join: what brings the answer of motifs [c0, c0 + nc) to the caller.
template <typename W, typename MakeJob, typename After>
int launch_walk(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const char *degenerate, size_t n, const lm_hip_seqset *set,
                size_t slots_per_job, size_t per_job, MakeJob make_job, After after)
{
    typedef typename W::Job Job;
    typedef typename W::Slot Slot;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    const WalkKernels<W> &kernels = WalkKernels<W>::get();
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1;
    const bool off_lds = records + 1 <= kSetLdsOffsets;
    const size_t off_bytes = off_lds ? (records + 1) * sizeof(unsigned long long) : 0;
    const size_t group = walk_group_size(n, per_job);
    const size_t head = (group * sizeof(Job) + 255) & ~(size_t)255;
    LM_TRY(ctx->scratch.reserve(head + group * per_job));
    char *block = static_cast<char *>(ctx->scratch.ptr);
    Job *d_jobs = reinterpret_cast<Job *>(block);
    Slot *d_slots = reinterpret_cast<Slot *>(block + head);
    std::vector<Job> table;
    std::vector<ScoreArgs> args;
    for (size_t c0 = 0; c0 < n; c0 += group) {
        const size_t c1 = std::min(n, c0 + group), nc = c1 - c0;
        // the live jobs of this group of motifs, in launch order: JobGroups of one motif length each (grid.y)
        args.clear();
        std::vector<size_t> caller;  // caller index - c0 of args[i]
        for (size_t i = c0; i < c1; ++i)
            if (!degenerate[i]) {
                args.push_back(ScoreArgs{pssms[i], seq->d_data, seq->stride, seq->cols, 0, seq->rows, nullptr, 0});
                caller.push_back(i - c0);
            }
        const std::vector<JobGroup> groups = group_jobs(ctx, args.data(), args.size(), [&](size_t i) {
            return !WalkTable<W>::kOwn && args[i].pssm->m <= (size_t)kMaxFastM ? KIND_EXACT : KIND_GENERIC;
        });
        table.clear();
        std::vector<size_t> first(groups.size());
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            first[gi] = table.size();
            for (size_t i : groups[gi].idx)
                table.push_back(make_job(c0 + caller[i], (unsigned long long)caller[i] * slots_per_job));
        }
        LM_HIP_TRY(hipMemsetAsync(d_slots, 0, nc * slots_per_job * sizeof(Slot), ctx->stream));
        if (!table.empty()) {
            const size_t tbytes = table.size() * sizeof(Job);
            if (Job *pin = pinned_at<Job>(ctx, kPinUploadHead, table.size())) {
                memcpy(pin, table.data(), tbytes);
                LM_HIP_TRY(hipMemcpyAsync(d_jobs, pin, tbytes, hipMemcpyHostToDevice, ctx->stream));
            } else {
                LM_HIP_TRY(hipMemcpy(d_jobs, table.data(), tbytes, hipMemcpyHostToDevice));
            }
        }
        BatchStreams streams(ctx, groups.size());
        LM_TRY(streams.fork());
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const JobGroup &g = groups[gi];
            const lm_hip_pssm *p = args[g.idx[0]].pssm;
            const unsigned long long T = walk_rows_per_lane(ctx, seq, p->m, args.size());
            const unsigned long long lanes = ((unsigned long long)seq->rows + T - 1) / T * seq->cols;
            const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)g.idx.size());
            hipStream_t st = streams.next();
            if (g.kind == KIND_EXACT) {
                const size_t lds = (((size_t)p->k * table_stride((int)p->m, 0) * 4 + 15) & ~(size_t)15) + off_bytes;
                if (W::kTally >= 0)
                    tally_launch(ctx, W::kTally, false, p->m);
                hipLaunchKernelGGL(kernels.fn[p->m], grid, dim3(kBlock), lds, st, seq->d_data, (unsigned long long)seq->stride,
                                   (unsigned)seq->cols, (unsigned long long)seq->rows, (unsigned long long)(seq->rows + seq->wrap),
                                   (unsigned)p->k, d_jobs + first[gi], set->d_offsets, (unsigned long long)records, (int)off_lds, T,
                                   d_slots);
                ctx->last_kernel = kernels.name[p->m];
            } else {
                const size_t wbytes = p->m * p->k * sizeof(float);
                const int w_lds = wbytes + off_bytes <= 60 * 1024;
                const size_t staged = (w_lds ? (wbytes + 15) & ~(size_t)15 : 0) + off_bytes;
                const size_t lds = std::max<size_t>(staged + WalkTable<W>::lds(staged, p->m, p->k), 16);
                hipLaunchKernelGGL(W::generic(), grid, dim3(kBlock), lds, st, seq->d_data, (unsigned long long)seq->stride,
                                   (unsigned)seq->cols, (unsigned long long)seq->rows, (unsigned)p->m, (unsigned)p->k, w_lds,
                                   d_jobs + first[gi], set->d_offsets, (unsigned long long)records, (int)off_lds, T, d_slots);
                ctx->last_kernel = kernels.generic_name;
            }
            LM_HIP_TRY(hipGetLastError());
        }
        LM_TRY(streams.join());
        LM_TRY(after(c0, nc, d_slots));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return LM_HIP_OK;
}

}  // namespace lm
