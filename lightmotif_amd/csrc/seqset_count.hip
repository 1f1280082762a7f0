// seqset_count.hip -- how many windows of every motif in every record of a resident sequence set reach a cut-off, at up
// to LM_HIP_MAX_COUNT_LEVELS cut-offs per motif, without a score matrix and without a hit list: the walk of
// seqset_best.hip with another reduction.
//
// The reference's CLI would collect the hits of every (motif, record) job (main.rs:502-561) and the caller would count
// them; the question itself needs no list.  The windows of record r are the positions p with p + M <= len(r)
// (scan.rs:185-190, per RECORD) and each scores as `score_into` scores it: M sequential f32 adds from +0.0 in row order
// (pli/mod.rs:96-105).  A window counts at level l when `score >= t[l]` under f32 comparison: NaN windows and NaN
// thresholds count nothing, -inf windows count at a threshold of -inf alone.
//
//   seqset_count_fused<M>   M <= kMaxFastM.  A lane owns rows [r0, r1) of one column, one symbol load per row, the M
//                           windows that symbol belongs to in M rotating accumulators, the loop unrolled M steps (see
//                           seqset_best_fused<M>: the same walk, the same two devices against register pressure).
//   seqset_count_generic    any M: the same walk, every window summed from scratch over its M symbols.
//
// Both keep, per lane, the current record, the position of the next EVENT (the first window of the record that no longer
// fits, then the record's end) and LM_HIP_MAX_COUNT_LEVELS 32-bit counters in registers; the loop over levels is unrolled
// to that constant and the levels a call does not use carry a NaN threshold, so nothing is indexed dynamically.  At a
// record's end and at the end of its run a lane adds every non-zero counter to its cell
//       slots[(job * levels + level) * records + record]
// with one 32-bit atomicAdd whose result nobody reads.  Integer addition is associative and commutative, so the cells do
// not depend on the order in which the lanes arrive: the answer is deterministic.  The cells are the caller's final
// uint32_t values: one memset before the launches of a group of motifs, one copy back after them, no finalize kernel.
//
// Offsets of sets of up to 4 095 records are staged in LDS, larger tables are read from global memory.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "score_launch.hpp"

namespace lm {

namespace setcount {  // (named: tools/kernel_regs.py lists kernels by their demangled names)

constexpr int kLevels = LM_HIP_MAX_COUNT_LEVELS;
constexpr unsigned kCountLdsOffsets = 4096;  // offsets (8 B each) a workgroup stages, as seqset_best does
constexpr unsigned long long kNoEnd = ~0ull;

struct CountJob {
    const float *dense;             // M x K weights, row-major
    unsigned long long slot_base;   // first cell of the job: slots[slot_base + level * records + record]
    float t[kLevels];               // cut-offs; NaN: level not in use
};

// What a lane carries down its run of consecutive positions (the record walk of seqset_best.hip's Segmenter).
struct Counter {
    const unsigned long long *off;  // n + 1 offsets (LDS or global)
    unsigned long long n;           // records
    unsigned long long m;           // motif length
    unsigned *slots;                // of this job
    unsigned long long rec, start, end;
    unsigned long long next;        // position of the next event
    bool competing;                 // windows before `next` lie inside the record
    float t[kLevels];
    unsigned c[kLevels];            // windows of `rec` counted by this lane and not yet added to the cells

    __device__ __forceinline__ void enter(unsigned long long r)
    {
        rec = r;
        start = off[r < n ? r : n];
        end = r < n ? off[r + 1] : kNoEnd;  // behind the last record: padding, nothing fits and nothing ends
        competing = true;
        next = (r < n && end - start >= m) ? end - m + 1 : start;
    }
    __device__ __forceinline__ void begin(unsigned long long p, const CountJob &job)
    {
#pragma unroll
        for (int l = 0; l < kLevels; ++l) {
            t[l] = job.t[l];
            c[l] = 0;
        }
        // largest r with off[r] <= p (seqset.hip: find_record, without a hint)
        unsigned long long lo = 0, hi = n + 1;
        while (lo < hi) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            if (off[mid] <= p)
                lo = mid + 1;
            else
                hi = mid;
        }
        enter(lo - 1);
    }
    __device__ __forceinline__ void flush()
    {
        if (rec >= n)  // (only windows inside a record count, so every counter is 0 here)
            return;
#pragma unroll
        for (int l = 0; l < kLevels; ++l)
            if (c[l]) {
                atomicAdd(slots + (unsigned long long)l * n + rec, c[l]);
                c[l] = 0;
            }
    }
    __device__ __forceinline__ void event(unsigned long long p)
    {
        while (p >= next) {
            if (competing) {  // the first window that no longer fits: straddlers up to the record's end
                competing = false;
                next = end;
            } else {
                flush();
                enter(rec + 1);
            }
        }
    }
    // the window at position p (ascending from call to call) scored v; `live` off: not a window of this lane's run.
    // (v is consumed on the straight path, by selects: behind a branch the compiler would sink the adds that make it
    // to here and keep every weight row of the last M steps in registers instead of M accumulators)
    __device__ __forceinline__ void take(unsigned long long p, float v, bool live = true)
    {
        if (__builtin_expect(live && p >= next, 0))
            event(p);
        const bool inside = live && competing;
#pragma unroll
        for (int l = 0; l < kLevels; ++l)
            c[l] += (inside && v >= t[l]) ? 1u : 0u;  // false for a NaN score and for a NaN threshold
    }
};

// dynamic LDS: [weights, 16-byte padded][offsets when they are staged]
extern __shared__ __attribute__((aligned(16))) char s_dyn[];

__device__ __forceinline__ const unsigned long long *stage_offsets(char *lds, const unsigned long long *g_offsets,
                                                                   unsigned long long n_records, int in_lds)
{
    if (!in_lds)
        return g_offsets;
    unsigned long long *s_off = reinterpret_cast<unsigned long long *>(lds);
    for (unsigned i = threadIdx.x; i <= (unsigned)n_records; i += kBlock)
        s_off[i] = g_offsets[i];
    return s_off;
}

template <int MP>
__device__ __forceinline__ void fetch_weights(float (&w)[MP], const float *row)
{
    const float4 *wr = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int q = 0; q < MP / 4; ++q) {
        const float4 v = wr[q];
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
}

// grid.x: workgroups of kBlock lanes, lane L = blockIdx.x * kBlock + threadIdx.x owns column L % cols of stream L / cols
// (rows [stream * T, stream * T + T)); grid.y: the jobs of one motif length.
template <int M>
__global__ __launch_bounds__(kBlock) void seqset_count_fused(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned long long rows_total, const unsigned K, const CountJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned *__restrict__ slots)
{
    constexpr int TS = table_stride(M, 0);  // floats per symbol, a multiple of 4: 16-byte aligned rows
    constexpr int MP = 4 * ((M + 3) / 4);
    const CountJob job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);  // s_w[s * TS + j] = weights[j][s], zero padded
    const unsigned wbytes = (K * TS * 4u + 15u) & ~15u;
    for (unsigned i = threadIdx.x; i < K * TS; i += kBlock) {
        const unsigned s = i / TS, j = i % TS;
        s_w[i] = j < (unsigned)M ? job.dense[j * K + s] : 0.0f;
    }
    Counter ct;
    ct.off = stage_offsets(s_dyn + wbytes, g_offsets, n_records, offsets_in_lds);
    __syncthreads();

    const unsigned long long lane = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long col = lane % cols, r0 = (lane / cols) * T;
    if (r0 >= rows)
        return;
    const unsigned long long r1 = r0 + T < rows ? r0 + T : rows;
    ct.n = n_records;
    ct.m = M;
    ct.slots = slots + job.slot_base;
    ct.begin(col * rows + r0, job);

    // step t reads row r0 + t; the window it completes started at row r0 + t - (M - 1): position base + t
    const unsigned long long total = (r1 - r0) + (M - 1);
    const long long base = (long long)(col * rows + r0) - (M - 1);
    const unsigned long long last_row = rows_total - 1;  // rows + wrap - 1 >= r1 + M - 2: clamped reads are never used
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
        // the weight rows of step s + 1 are fetched while step s adds, and no further ahead: the scheduler otherwise
        // hoists the rows of all M steps (M * M registers)
        float w[2][MP];
        fetch_weights<MP>(w[0], s_w + sym[0] * TS);
#pragma unroll
        for (int s = 0; s < M; ++s) {
            if (s + 1 < M)
                fetch_weights<MP>(w[(s + 1) & 1], s_w + sym[s + 1] * TS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < M; ++j)
                acc[(s - j + M) % M] = acc[(s - j + M) % M] + w[s & 1][j];  // window (t - j) receives row j
            // pins the sums here: the compiler otherwise sinks each window's adds to the step that completes it, behind
            // the event branches, and keeps the weight rows of M steps alive instead of M accumulators
#pragma unroll
            for (int j = 0; j < M; ++j)
                asm volatile("" : "+v"(acc[j]));
            const unsigned long long t = g + s;
            const float v = acc[(s + 1) % M];  // the window that started M - 1 steps ago is complete
            acc[(s + 1) % M] = 0.0f;
            ct.take((unsigned long long)(base + (long long)t), v, t >= (unsigned long long)(M - 1) && t < total);
        }
    }
    ct.flush();
}

// Any motif length: every window summed over its own M symbols (weights in LDS when they fit, `w_in_lds`).
__global__ __launch_bounds__(kBlock) void seqset_count_generic(
    const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols, const unsigned long long rows,
    const unsigned M, const unsigned K, const int w_in_lds, const CountJob *__restrict__ jobs,
    const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records, const int offsets_in_lds,
    const unsigned long long T, unsigned *__restrict__ slots)
{
    const CountJob job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);
    const unsigned wbytes = w_in_lds ? (M * K * 4u + 15u) & ~15u : 0u;
    if (w_in_lds)
        for (unsigned i = threadIdx.x; i < M * K; i += kBlock)
            s_w[i] = job.dense[i];
    Counter ct;
    ct.off = stage_offsets(s_dyn + wbytes, g_offsets, n_records, offsets_in_lds);
    __syncthreads();

    const unsigned long long lane = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long col = lane % cols, r0 = (lane / cols) * T;
    if (r0 >= rows)
        return;
    const unsigned long long r1 = r0 + T < rows ? r0 + T : rows;
    ct.n = n_records;
    ct.m = M;
    ct.slots = slots + job.slot_base;
    ct.begin(col * rows + r0, job);
    const uint8_t *sp = seq + col;
    for (unsigned long long row = r0; row < r1; ++row) {  // rows row .. row + M - 1 <= rows + wrap - 1
        const uint8_t *s = sp + row * stride;
        float v = 0.0f;
        if (w_in_lds)
            for (unsigned j = 0; j < M; ++j)
                v = v + s_w[j * K + s[j * stride]];
        else
            for (unsigned j = 0; j < M; ++j)
                v = v + job.dense[j * K + s[j * stride]];
        ct.take(col * rows + row, v);
    }
    ct.flush();
}

typedef void (*FusedKernel)(const uint8_t *, unsigned long long, unsigned, unsigned long long, unsigned long long, unsigned,
                            const CountJob *, const unsigned long long *, unsigned long long, int, unsigned long long, unsigned *);
template <int M>
struct FusedTable {
    static void fill(FusedKernel *t, const char **names)
    {
        static char name[32];
        snprintf(name, sizeof name, "seqset_count_fused<%d>", M);
        t[M] = seqset_count_fused<M>;
        names[M] = name;
        FusedTable<M - 1>::fill(t, names);
    }
};
template <>
struct FusedTable<0> {
    static void fill(FusedKernel *, const char **) {}
};

struct Fused {
    FusedKernel fn[kMaxFastM + 1] = {};
    const char *name[kMaxFastM + 1] = {};
    Fused() { FusedTable<kMaxFastM>::fill(fn, name); }
};
const Fused &fused()
{
    static const Fused f;
    return f;
}

constexpr size_t kCountBlockBytes = (size_t)256 << 20;  // the cells of one group of motifs on the device

}  // namespace setcount
using namespace setcount;

// Rows per lane, as launch_seqset_best chooses them: long enough that the M - 1 fill steps of a run cost little, short
// enough that the `njobs` jobs of the call put a few wavefronts on every SIMD.
static unsigned long long count_rows_per_lane(const lm_hip_ctx *ctx, const lm_hip_seq *seq, size_t m, size_t njobs)
{
    if (ctx->rows_per_stream)
        return ctx->rows_per_stream;
    const unsigned long long cells = (unsigned long long)seq->rows * seq->cols * njobs;
    const unsigned long long lanes = (unsigned long long)ctx->num_cus * 512;
    return std::min<unsigned long long>(std::max<unsigned long long>({4ull * m, cells / lanes, 16ull}), 4096ull);
}

int launch_seqset_count(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds, size_t levels,
                        const char *degenerate, size_t n, const lm_hip_seqset *set, uint32_t *counts)
{
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1;
    const bool off_lds = records + 1 <= kCountLdsOffsets;
    const size_t off_bytes = off_lds ? (records + 1) * sizeof(unsigned long long) : 0;
    const size_t per_job = levels * records * sizeof(uint32_t);
    const size_t group = std::max<size_t>(1, std::min<size_t>(n, kCountBlockBytes / std::max<size_t>(per_job, 1)));
    const size_t head = (group * sizeof(CountJob) + 255) & ~(size_t)255;
    LM_TRY(ctx->scratch.reserve(head + group * per_job));
    char *block = static_cast<char *>(ctx->scratch.ptr);
    CountJob *d_jobs = reinterpret_cast<CountJob *>(block);
    unsigned *d_slots = reinterpret_cast<unsigned *>(block + head);
    std::vector<CountJob> table;
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
            return args[i].pssm->m <= (size_t)kMaxFastM ? KIND_EXACT : KIND_GENERIC;
        });
        table.clear();
        std::vector<size_t> first(groups.size());
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            first[gi] = table.size();
            for (size_t i : groups[gi].idx) {
                CountJob job{args[i].pssm->d_dense, (unsigned long long)caller[i] * levels * records, {}};
                for (size_t l = 0; l < (size_t)kLevels; ++l)
                    job.t[l] = l < levels ? thresholds[(c0 + caller[i]) * levels + l] : std::nanf("");
                table.push_back(job);
            }
        }
        LM_HIP_TRY(hipMemsetAsync(d_slots, 0, nc * per_job, ctx->stream));
        if (!table.empty()) {
            const size_t tbytes = table.size() * sizeof(CountJob);
            if (CountJob *pin = pinned_at<CountJob>(ctx, kPinUploadHead, table.size())) {
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
            const unsigned long long T = count_rows_per_lane(ctx, seq, p->m, args.size());
            const unsigned long long lanes = ((unsigned long long)seq->rows + T - 1) / T * seq->cols;
            const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)g.idx.size());
            hipStream_t st = streams.next();
            if (g.kind == KIND_EXACT) {
                const size_t lds = (((size_t)p->k * table_stride((int)p->m, 0) * 4 + 15) & ~(size_t)15) + off_bytes;
                hipLaunchKernelGGL(fused().fn[p->m], grid, dim3(kBlock), lds, st, seq->d_data, (unsigned long long)seq->stride,
                                   (unsigned)seq->cols, (unsigned long long)seq->rows, (unsigned long long)(seq->rows + seq->wrap),
                                   (unsigned)p->k, d_jobs + first[gi], set->d_offsets, (unsigned long long)records, (int)off_lds, T,
                                   d_slots);
                ctx->last_kernel = fused().name[p->m];
            } else {
                const size_t wbytes = p->m * p->k * sizeof(float);
                const int w_lds = wbytes + off_bytes <= 60 * 1024;
                const size_t lds = std::max<size_t>((w_lds ? (wbytes + 15) & ~(size_t)15 : 0) + off_bytes, 16);
                hipLaunchKernelGGL(seqset_count_generic, grid, dim3(kBlock), lds, st, seq->d_data, (unsigned long long)seq->stride,
                                   (unsigned)seq->cols, (unsigned long long)seq->rows, (unsigned)p->m, (unsigned)p->k, w_lds,
                                   d_jobs + first[gi], set->d_offsets, (unsigned long long)records, (int)off_lds, T, d_slots);
                ctx->last_kernel = "seqset_count_generic";
            }
            LM_HIP_TRY(hipGetLastError());
        }
        LM_TRY(streams.join());
        LM_HIP_TRY(hipMemcpyAsync(counts + c0 * levels * records, d_slots, nc * per_job, hipMemcpyDeviceToHost, ctx->stream));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return LM_HIP_OK;
}

}  // namespace lm

using namespace lm;

extern "C" int lm_hip_scan_count_seqset(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds, size_t levels,
                                        size_t n, const lm_hip_seqset *set, uint32_t *counts)
{
    if (!ctx || !set || (n && (!pssms || !thresholds)))
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_count_seqset: null argument");
    if (levels < 1 || levels > (size_t)LM_HIP_MAX_COUNT_LEVELS)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_count_seqset: %zu levels, a call takes 1 ... %d", levels, LM_HIP_MAX_COUNT_LEVELS);
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1;
    if (n && records && !counts)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_count_seqset: null result array");
    std::vector<char> degenerate(n, 0);
    for (size_t i = 0; i < n; ++i) {  // as lm_hip_scan_best_seqset: alphabet, then wrap (avx2.rs:832-837)
        if (pssms[i])
            LM_TRY(check_alphabet("scan_count_seqset", pssms[i]->k, seq));
        LM_TRY(check_score_args(pssms[i], seq->rows + seq->wrap, seq->stride, seq->cols, seq->wrap, 0, seq->rows));
        degenerate[i] = seq->length < pssms[i]->m || seq->rows == 0 || pssms[i]->m == 0;  // pli/mod.rs:85-88: no scores
    }
    if (n == 0 || records == 0)
        return LM_HIP_OK;
    if (seq->length >> 32)  // a cell is 32 bits
        for (size_t r = 0; r < records; ++r)
            if ((set->offsets[r + 1] - set->offsets[r]) >> 32)
                return fail(LM_HIP_ERR_CAPACITY, "scan_count_seqset: record %zu holds %llu symbols, a cell counts to 2^32 - 1", r,
                            (unsigned long long)(set->offsets[r + 1] - set->offsets[r]));
    if (records > (~(size_t)0 / (sizeof(uint32_t) * levels)) / n)
        return fail(LM_HIP_ERR_CAPACITY, "scan_count_seqset: %zu motifs x %zu levels x %zu records overflow the result's size", n,
                    levels, records);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    return launch_seqset_count(ctx, pssms, thresholds, levels, degenerate.data(), n, set, counts);
}
