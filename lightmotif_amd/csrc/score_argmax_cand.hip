// score_argmax_cand.hip -- the candidate route of the fused argmax: sample, prefilter scans, exact re-scoring of the
// candidates, reduction of the hit list.  Who qualifies, geometry, capacities and scratch layout: argmax_plan.hpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "argmax_plan.hpp"
#include "score_launch.hpp"

namespace lm {

// ---- fused argmax through the prefilter ---------------------------------------------------------
//
// For large inputs the maximum is found like the Scanner finds hits: (1) the exact scores of
// an evenly spread SAMPLE of the job's rows give a lower bound L of the maximum (it IS a score of
// the matrix); (2) the packed 16-bit prefilter scan flags every row range that may hold a
// score >= L; (3) `rescore_candidates` turns them into exact hits -- all cells with score
// >= L, so the maximum and every tie of it are among them; (4) the hit list is reduced with
// the Generic rule: greatest score, ties -> greatest row-major index (pli/mod.rs:144-151).
// The scan costs half the LDS traffic and adds of the exact kernel (0.42 vs 0.66 ms per Gbp
// at M = 20); sample, re-scoring and reduction add a few tens of microseconds.  PSSMs with
// a prefilter have no NaN / +inf weights, so no score is NaN and the first-cell rule is
// moot.  Jobs whose sample is all -inf, or whose lists overflow (many cells tie with the
// bound), are left to the exact kernel.

struct SampleJob {
    const uint8_t *seq;  // row `row_begin` of the striped matrix (C = 32, stride 32)
    const float *dense;  // M x K weights
    unsigned m, k;
    unsigned long long nchunks, stride;  // chunk c starts at row c * stride
    double pre_offset, pre_factor, pre_emax;
    unsigned td_drop;  // drop-last form of the scan (lm_hip_pssm::d_image2_drop): what the unscanned last row may add; else 0
};

__device__ __forceinline__ unsigned ordered_bits(float v)
{
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotone map f32 -> u32 (no NaN here)
}
__device__ __forceinline__ float from_ordered_bits(unsigned k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
constexpr unsigned kOrderedNegInf = 0x007fffffu;  // ordered_bits(-inf)

// grid (blocks, jobs): exact scores of `nchunks` chunks of kSampleRows x 32 cells spread evenly
// over the job's rows.  Chunks, not single cells: a lone cell costs M cache sectors for M
// bytes (3.9 M scattered cells = 1.3 ms), a chunk reads its rows once.
using argmax::kSampleRows;  // one row per half-wave: a chunk is one pass of the block
constexpr unsigned kMaxSampleM = kMaxLongM;    // the candidate route needs a prefilter kernel: the DNA pair scan goes up to kMaxLongM
// exact score of the cell at `p` for a motif of at most MAXM rows: all symbol loads in flight at
// once, then all weight loads, then the reference's add order -- one HBM latency + one L2 latency
// per chunk instead of M / 4 of each (slots past the motif re-read its last row; the wrap rows
// keep the address valid)
template <unsigned MAXM>
__device__ __forceinline__ float sample_cell(const SampleJob &jb, const uint8_t *__restrict__ p)
{
    unsigned sy[MAXM];
    float w[MAXM];
#pragma unroll
    for (unsigned j = 0; j < MAXM; ++j)
        sy[j] = p[(j < jb.m ? j : jb.m - 1) * 32];
#pragma unroll
    for (unsigned j = 0; j < MAXM; ++j)
        w[j] = jb.dense[(j < jb.m ? j : jb.m - 1) * jb.k + sy[j]];
    float sc = 0.0f;
#pragma unroll
    for (unsigned j = 0; j < MAXM; ++j)
        sc = j < jb.m ? sc + w[j] : sc;
    return sc;
}

// motifs beyond kMaxSampleM rows (the pair scan goes up to kMaxPairM): row by row, the same add order
__device__ __forceinline__ float sample_cell_loop(const SampleJob &jb, const uint8_t *__restrict__ p)
{
    float sc = 0.0f;
    for (unsigned j = 0; j < jb.m; ++j)
        sc = sc + jb.dense[j * jb.k + p[j * 32]];
    return sc;
}

__global__ __launch_bounds__(kBlock) void argmax_sample(const SampleJob *__restrict__ jobs,
                                                        unsigned *__restrict__ partial)
{
    const SampleJob jb = jobs[blockIdx.y];
    unsigned best = kOrderedNegInf;
    const unsigned col = threadIdx.x & 31, sub = threadIdx.x >> 5;
    for (unsigned long long c = blockIdx.x; c < jb.nchunks; c += gridDim.x) {
        const unsigned long long r0 = c * jb.stride;  // chunk rows r0 .. r0 + kSampleRows - 1
        const uint8_t *p = jb.seq + (r0 + sub) * 32 + col;
        // (three unroll depths: most motifs of a batch are short, and every slot costs two loads)
        const float sc = jb.m <= 12   ? sample_cell<12>(jb, p)
                         : jb.m <= 24 ? sample_cell<24>(jb, p)
                         : jb.m <= 36 ? sample_cell<36>(jb, p)
                         : jb.m <= kMaxSampleM ? sample_cell<kMaxSampleM>(jb, p)
                                               : sample_cell_loop(jb, p);
        const unsigned key = ordered_bits(sc);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    // one record per workgroup, folded by argmax_prepare: thousands of atomics on one address serialise at ~12 ns each
    // (round 5 tried a ticket per workgroup so that the last one folds, to save that launch: 19 + 5 -> 62 us)
    __shared__ unsigned wave_best[kBlock / 64];
    if ((threadIdx.x & 63) == 0)
        wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w)
            best = wave_best[w] > best ? wave_best[w] : best;
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = best;
    }
}

// one wavefront per job: folds the sample's per-workgroup records into the lower bound, then
// lower bound -> f32 threshold of the re-scoring and discrete threshold of the scan (the map of
// launch_score_threshold_batch, argmax::discrete_threshold, restated below); td = 0xffffffff = "skip"
__global__ __launch_bounds__(64) void argmax_prepare(const SampleJob *__restrict__ jobs, const unsigned n,
                                                     const unsigned *__restrict__ partial, const unsigned nper,
                                                     RescoreJob *__restrict__ rjobs,
                                                     BatchParams *__restrict__ bparams)
{
    const unsigned j = blockIdx.x;
    unsigned bound = kOrderedNegInf;
    for (unsigned i = threadIdx.x; i < nper; i += 64) {
        const unsigned v = partial[(size_t)j * nper + i];
        bound = v > bound ? v : bound;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(bound, off);
        bound = o > bound ? o : bound;
    }
    if (threadIdx.x != 0)
        return;
    unsigned td = 0xffffffffu;
    float t = INFINITY;
    if (bound != kOrderedNegInf) {
        t = from_ordered_bits(bound);
        // argmax::discrete_threshold (argmax_plan.hpp), kept in its own words: a call of that function allocates one
        // register more and orders the instructions differently, and this kernel's text is held identical
        const double scaled = floor(((double)t - jobs[j].pre_offset) / jobs[j].pre_factor) -
                              ceil(jobs[j].pre_emax / jobs[j].pre_factor) - 1.0;
        if (scaled >= 1.0)
            td = scaled > 65535.0 ? 65535u : (unsigned)scaled;
        else
            t = INFINITY;  // the bound is too low for the 16-bit range: leave the job to the exact kernel
        if (td != 0xffffffffu && jobs[j].td_drop) {
            if (td > 4u * jobs[j].td_drop) {
                td -= jobs[j].td_drop;
            } else {  // the unscanned row carries too much of the bound: nothing is flagged, the exact kernel takes over
                td = 0xffffffffu;
                t = INFINITY;
            }
        }
    }
    rjobs[j].threshold = t;
    bparams[j].td = td;
}

// reduction of the hit list: per job the greatest score, then the greatest key among its ties
// atomicMax(&target[job], value) for every live lane, with ONE atomic per distinct job of the
// wavefront: the list is clustered by job in runs shorter than a wavefront (a re-scoring
// workgroup stages the hits of several rounds = several jobs before it flushes), and a
// wavefront-wide atomic with 64 different addresses costs 64 operations -- 10^6 records took
// 2.4 ms that way.  `value` 0 = nothing to contribute (0 is below every real value here).
template <typename T>
__device__ __forceinline__ void wave_atomic_max_by_job(const unsigned long long job, const T value,
                                                       const bool live, T *__restrict__ target)
{
    const int lane = threadIdx.x & 63;
    unsigned long long active = __ballot(live);
    while (active) {  // wave-uniform
        const int leader = __ffsll((long long)active) - 1;
        const unsigned long long j = __shfl(job, leader);
        const bool mine = live && job == j;
        T x = mine ? value : (T)0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const T o = __shfl_xor(x, off);
            x = o > x ? o : x;
        }
        if (lane == leader && x != (T)0)
            atomicMax(&target[j], x);
        active &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(kBlock) void hits_best_value(const HitRecord *__restrict__ hits,
                                                          const unsigned long long *__restrict__ count,
                                                          const unsigned long long capacity,
                                                          unsigned *__restrict__ best_value)
{
    unsigned long long n = *count;
    if (n > capacity)
        n = capacity;
    const unsigned long long span = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long i0 = (unsigned long long)blockIdx.x * kBlock; i0 < n; i0 += span) {
        const unsigned long long i = i0 + threadIdx.x;
        const bool live = i < n;
        HitRecord h{};
        if (live)
            h = hits[i];
        wave_atomic_max_by_job(h.key >> 40, live ? ordered_bits(h.value) : 0u, live, best_value);
    }
}

__global__ __launch_bounds__(kBlock) void hits_best_key(const HitRecord *__restrict__ hits,
                                                        const unsigned long long *__restrict__ count,
                                                        const unsigned long long capacity,
                                                        const unsigned *__restrict__ best_value,
                                                        unsigned long long *__restrict__ best_key)
{
    unsigned long long n = *count;
    if (n > capacity)
        n = capacity;
    const unsigned long long span = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long i0 = (unsigned long long)blockIdx.x * kBlock; i0 < n; i0 += span) {
        const unsigned long long i = i0 + threadIdx.x;
        const bool live = i < n;
        HitRecord h{};
        if (live)
            h = hits[i];
        const unsigned long long job = h.key >> 40;
        // 0 = not a tie of the job's best score
        const unsigned long long k = (live && ordered_bits(h.value) == best_value[job])
                                         ? (h.key & ((1ull << 40) - 1)) + 1 : 0ull;
        wave_atomic_max_by_job(job, k, live, best_key);
    }
}

__global__ void argmax_collect(const unsigned n, const unsigned *__restrict__ best_value,
                               const unsigned long long *__restrict__ best_key,
                               ArgmaxRecord *__restrict__ out,
                               const unsigned long long *__restrict__ counters,
                               unsigned long long *__restrict__ counters_out)
{
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && counters_out) {  // {hits, candidates}: the host checks them for overflow
        counters_out[0] = counters[0];
        counters_out[1] = counters[1];
    }
    if (j >= n)
        return;
    ArgmaxRecord r;
    r.found = best_key[j] != 0;
    r.value = from_ordered_bits(best_value[j]);
    r.index = (long long)best_key[j] - 1;
    out[j] = r;
}

// ONE job: the three launches above in one workgroup -- best value, greatest key among its ties, the record and the
// counters for the host.  The list holds ~10^3 records (at most its capacity, 8 192 + 65 536) and every launch of the
// tail costs ~5 us whatever it does (profiles/r05_timeline_fused.txt), 15 of the call's 280.
constexpr int kBestSingleBlock = 1024;
__global__ __launch_bounds__(kBestSingleBlock) void hits_best_single(const HitRecord *__restrict__ hits,
                                                                     const unsigned long long *__restrict__ counters,
                                                                     const unsigned long long capacity,
                                                                     ArgmaxRecord *__restrict__ out,
                                                                     unsigned long long *__restrict__ counters_out)
{
    __shared__ unsigned wave_value[kBestSingleBlock / 64];
    __shared__ unsigned long long wave_key[kBestSingleBlock / 64];
    unsigned long long n = counters[0];
    if (n > capacity)
        n = capacity;
    unsigned bv = kOrderedNegInf;
    for (unsigned long long i = threadIdx.x; i < n; i += kBestSingleBlock) {
        const unsigned v = ordered_bits(hits[i].value);
        bv = v > bv ? v : bv;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(bv, off);
        bv = o > bv ? o : bv;
    }
    if ((threadIdx.x & 63) == 0)
        wave_value[threadIdx.x >> 6] = bv;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBestSingleBlock / 64; ++w)
        bv = wave_value[w] > bv ? wave_value[w] : bv;
    unsigned long long bk = 0;  // (low + 1) of the greatest tied key; 0 = no record reaches the value
    for (unsigned long long i = threadIdx.x; i < n; i += kBestSingleBlock) {
        const HitRecord h = hits[i];
        const unsigned long long k = ordered_bits(h.value) == bv ? (h.key & ((1ull << 40) - 1)) + 1 : 0ull;
        bk = k > bk ? k : bk;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(bk, off);
        bk = o > bk ? o : bk;
    }
    if ((threadIdx.x & 63) == 0)
        wave_key[threadIdx.x >> 6] = bk;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (int w = 0; w < kBestSingleBlock / 64; ++w)
        bk = wave_key[w] > bk ? wave_key[w] : bk;
    if (counters_out) {
        counters_out[0] = counters[0];
        counters_out[1] = counters[1];
    }
    ArgmaxRecord r;
    r.found = bk != 0;
    r.value = from_ordered_bits(bv);
    r.index = (long long)bk - 1;
    out[0] = r;
}

static_assert(sizeof(ArgmaxRecord) == argmax::kRecordBytes && sizeof(SampleJob) == argmax::kSampleJobBytes &&
                  sizeof(RescoreJob) == argmax::kRescoreJobBytes && sizeof(BatchParams) == argmax::kBatchParamsBytes &&
                  kBlock == argmax::kPlanBlock && kHitListHead == argmax::kListHead,
              "argmax_plan.hpp repeats these sizes");

// A call of the route as planned: the jobs it takes, their scans, the tables and where everything lives in the scratch block.
struct CandCall {
    std::vector<size_t> pick;      // the jobs that qualify, as indices of the caller's ...
    std::vector<ScoreArgs> qjobs;  // ... and by value: job q of the route
    std::vector<JobGroup> groups;
    ScanPlan sp;
    size_t npos = 0;  // positions in launch order, padding included
    argmax::CandLists lists;
    argmax::CandHead head;
    std::vector<SampleJob> sj;  // the three job tables in launch order
    std::vector<RescoreJob> rj;
    std::vector<BatchParams> bparams;
    FusedOut fo{};
    char *base = nullptr;
    template <class T>
    T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
};

// the jobs the route takes; none when the call as a whole does not pay
static std::vector<size_t> pick_jobs(const lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, const char *done)
{
    std::vector<size_t> pick;
    unsigned long long picked_cells = 0;
    for (size_t i = 0; i < n; ++i) {
        const ScoreArgs &a = jobs[i];
        const unsigned long long cells = (unsigned long long)(a.row_end - a.row_begin) * a.cols;
        if (!done[i] && argmax::cand_job_qualifies(cells, a.pssm->m, a.pssm->k, a.pssm->has_prefilter, [&] {
                return plan_c32(ctx, a, false, 1).ok || plan_c32(ctx, a, false, 2).ok;
            })) {
            pick.push_back(i);
            picked_cells += cells;
        }
    }
    if (!argmax::cand_call_qualifies(pick.size(), picked_cells))
        pick.clear();
    return pick;
}

static void plan_candidates(lm_hip_ctx *ctx, const ScoreArgs *jobs, CandCall &c)
{
    const size_t nq = c.pick.size();
    c.qjobs.resize(nq);
    for (size_t q = 0; q < nq; ++q)
        c.qjobs[q] = jobs[c.pick[q]];
    c.groups = group_jobs(ctx, c.qjobs.data(), nq, [&](size_t q) {
        return (ctx->pair_prefilter && plan_c32(ctx, c.qjobs[q], false, 2).ok) ? (int)KIND_PREFILTER2
                                                                               : (int)KIND_PREFILTER;
    });
    // (drop-last form of a lone pair scan: argmax_prepare declines on the device when the unscanned row carries too much)
    c.sp = plan_scans(ctx, c.qjobs.data(), nq, c.groups, true);
    record_scan_shape(ctx, c.sp, c.groups, c.qjobs.data(), nq);
    c.npos = c.sp.order.size();
    c.head = argmax::cand_head(c.npos, sizeof(RescoreJob), sizeof(BatchParams), sizeof(SampleJob));
    // the three job tables in launch order; a padding position samples nothing, so argmax_prepare leaves its td at "skip"
    c.sj.resize(c.npos);
    c.rj.resize(c.npos);
    c.bparams.resize(c.npos);
    unsigned long long max_chunks = 0;
    for (size_t gi = 0; gi < c.groups.size(); ++gi)
        for (size_t pos = c.sp.groups[gi].pos; pos < c.sp.group_end(gi); ++pos) {
            const size_t q = c.sp.order[pos].job;
            const ScoreArgs &a = c.qjobs[q];
            const lm_hip_pssm *p = a.pssm;
            const argmax::SampleGeometry g = argmax::sample_geometry(a.row_end - a.row_begin, c.qjobs.size(), (unsigned)ctx->num_cus);
            max_chunks = std::max(max_chunks, g.nchunks);
            c.sj[pos] = SampleJob{a.d_seq + a.row_begin * a.seq_stride, p->d_dense, (unsigned)p->m, (unsigned)p->k,
                                  c.sp.order[pos].pad ? 0ull : g.nchunks, g.stride,
                                  p->pre_offset, p->pre_factor, p->pre_emax, c.sp.drop.ok && q == 0 ? p->drop_dmax : 0u};
            c.rj[pos] = RescoreJob{c.sj[pos].seq, p->d_dense, (unsigned)p->m, (unsigned)p->k, INFINITY, 0, 0};
            c.bparams[pos] = BatchParams{scan_table(c.sp, gi, c.groups[gi].kind, a), nullptr, 0.0f, 0xffffffffu,
                                         (unsigned long long)pos << 40};
        }
    c.lists = argmax::cand_lists(c.npos, max_chunks, (unsigned)ctx->num_cus);
}

// the head of the scratch block goes up, the sample runs, and argmax_prepare turns its maxima into the jobs' thresholds
static int upload_and_sample(lm_hip_ctx *ctx, CandCall &c)
{
    const size_t npos = c.npos;
    const argmax::CandHead &h = c.head;
    LM_TRY(reserve_hit_lists(ctx, h.off_hits, c.lists.cap, c.lists.ccap, argmax::cand_tail_bytes(npos, c.lists.sgrid), &c.fo, &c.base));
    unsigned *d_partial = reinterpret_cast<unsigned *>(c.fo.cands + c.lists.ccap);
    const HeadPart parts[5] = {{h.off_bval, nullptr, npos * 4, kOrderedNegInf},  // best values start at -inf,
                               {h.off_bkey, nullptr, npos * 8, 0u},             // best keys at zero
                               {h.off_rj, c.rj.data(), npos * sizeof(RescoreJob), 0u},
                               {h.off_bp, c.bparams.data(), npos * sizeof(BatchParams), 0u},
                               {h.off_sj, c.sj.data(), npos * sizeof(SampleJob), 0u}};
    LM_TRY(upload_head(ctx, ctx->stream, c.base, h.off_res, h.off_rj, parts, 5));
    hipLaunchKernelGGL(argmax_sample, dim3(c.lists.sgrid, (unsigned)npos), dim3(kBlock), 0, ctx->stream, c.at<SampleJob>(h.off_sj), d_partial);
    hipLaunchKernelGGL(argmax_prepare, dim3((unsigned)npos), dim3(64), 0, ctx->stream, c.at<SampleJob>(h.off_sj), (unsigned)npos, d_partial,
                       c.lists.sgrid, c.at<RescoreJob>(h.off_rj), c.at<BatchParams>(h.off_bp));
    LM_HIP_TRY(hipGetLastError());
    return LM_HIP_OK;
}

// the prefilter scans, alternating between the two streams (tables and thresholds come from the jobs' BatchParams)
static int launch_candidate_scans(lm_hip_ctx *ctx, CandCall &c)
{
    BatchStreams streams(ctx, c.groups.size());
    scan_timer_begin(ctx, ctx->stream);
    LM_TRY(streams.fork());
    for (size_t gi = 0; gi < c.groups.size(); ++gi) {
        c.fo.batch = c.at<BatchParams>(c.head.off_bp) + c.sp.groups[gi].pos;
        LM_TRY(launch_group_scan(ctx, c.sp, gi, c.groups[gi], c.qjobs[c.groups[gi].idx[0]], MODE_THRESHOLD, 0xffffffffu, streams.next(), c.fo));
    }
    LM_TRY(streams.join());
    scan_timer_end(ctx, ctx->stream);
    c.fo.batch = nullptr;
    return LM_HIP_OK;
}

int argmax_by_prefilter(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, ArgmaxRecord *out, char *done)
{
    CandCall c;
    c.pick = pick_jobs(ctx, jobs, n, done);
    if (c.pick.empty())
        return LM_HIP_OK;
    plan_candidates(ctx, jobs, c);  // scans, head layout, the three job tables, list sizes
    LM_TRY(upload_and_sample(ctx, c));
    LM_TRY(launch_candidate_scans(ctx, c));
    LM_TRY(launch_rescore(ctx, ctx->stream, c.at<RescoreJob>(c.head.off_rj), c.fo, c.rj.data(), c.npos));
    // reduction of the list, by one kernel or by three; results and the two list counters go straight into the pinned block
    const size_t npos = c.npos;
    const unsigned long long cap = c.lists.cap, ccap = c.lists.ccap;
    hipStream_t st = ctx->stream;
    unsigned long long *h_counts = pinned_at<unsigned long long>(ctx, kPinCounters, 2), *counts_out = nullptr;
    ArgmaxRecord *d_res = c.at<ArgmaxRecord>(c.head.off_res), *res = d_res;
    if (ArgmaxRecord *pin_res = pinned_at<ArgmaxRecord>(ctx, kPinCandResults, npos)) {
        res = pin_res;
        counts_out = h_counts;
    }
    if (npos == 1) {
        hipLaunchKernelGGL(hits_best_single, dim3(1), dim3(kBestSingleBlock), 0, st, c.fo.hits, c.fo.hit_count, cap, res, counts_out);
    } else {
        const unsigned hgrid = (unsigned)ctx->num_cus * 2;
        unsigned *d_bval = c.at<unsigned>(c.head.off_bval);
        unsigned long long *d_bkey = c.at<unsigned long long>(c.head.off_bkey);
        hipLaunchKernelGGL(hits_best_value, dim3(hgrid), dim3(kBlock), 0, st, c.fo.hits, c.fo.hit_count, cap, d_bval);
        hipLaunchKernelGGL(hits_best_key, dim3(hgrid), dim3(kBlock), 0, st, c.fo.hits, c.fo.hit_count, cap, d_bval, d_bkey);
        hipLaunchKernelGGL(argmax_collect, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, st, (unsigned)npos, d_bval, d_bkey, res,
                           c.fo.hit_count, counts_out);
    }
    LM_HIP_TRY(hipGetLastError());
    std::vector<ArgmaxRecord> host_res(res == d_res ? npos : 0);
    if (res == d_res) {
        LM_HIP_TRY(hipMemcpyAsync(h_counts, c.base, 16, hipMemcpyDeviceToHost, st));
        LM_HIP_TRY(hipMemcpyAsync(host_res.data(), d_res, npos * sizeof(ArgmaxRecord), hipMemcpyDeviceToHost, st));
        res = host_res.data();
    }
    LM_HIP_TRY(hipStreamSynchronize(st));
    scan_timer_read(ctx);
    const unsigned long long nhits = h_counts[0], ncand = h_counts[1];
    if (getenv("LM_HIP_TRACE"))
        fprintf(stderr, "[lm_hip] candidate-route argmax: %zu jobs, %llu candidates (room %llu), %llu hits (room %llu)\n",
                npos, ncand, ccap, nhits, cap);
    if (nhits > cap || ncand > ccap)
        return LM_HIP_OK;  // truncated lists prove nothing: the exact kernel takes over
    for (size_t pos = 0; pos < npos; ++pos)
        if (res[pos].found) {
            const size_t i = c.pick[c.sp.order[pos].job];
            out[i] = res[pos];
            done[i] = 1;
        }
    return LM_HIP_OK;
}

}  // namespace lm
