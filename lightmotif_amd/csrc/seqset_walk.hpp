// seqset_walk.hpp -- the record walk the per-record reductions over a resident sequence set share (seqset_best.hip: the
// best window, seqset_count.hip: the windows that reach a cut-off, seqset_sum.hip: the sum of their odds), and the two
// kernel bodies that drive it.  The host
// half (kernel table, launcher, entry checks) is seqset_walk_launch.hpp; this file needs no more than kBlock, so that the
// walk compiles for the host alone as well (tests/cpp/test_seqset_walk.cpp).
//
// In the striped layout a lane that walks down one column meets CONSECUTIVE positions of the concatenation, so a record
// is a run of rows and its boundaries come to the lane.  A Walker keeps, per lane, the current record (one binary search
// at the start of the run, then advanced) and the position of the next EVENT: the first window of the record that no
// longer fits (offsets[r + 1] - M + 1) and then the record's end, so that a common step pays one compare.  Windows between
// the two are scored and are not `inside` (the straddlers).  What a window inside a record does, and what reaches the
// slots of the job at a record's end and at the end of the run, is the REDUCER's business:
//
//   struct Reducer {
//       typedef ... Slot;                          // what the job's slots are made of
//       void begin(const Job &job);                // before the first window of a run
//       void window(p, v, inside);                 // the window at position p scored v; on the straight path (see take)
//       void flush(Slot *slots, rec, start, n);    // merge what record `rec` (< n, starting at `start`) gathered, and reset
//   };
//
// all of it __forceinline__, nothing virtual.
//
//   walk_fused<M, TS, R>   M <= kMaxFastM.  A lane owns rows [r0, r1) of one column, loads one symbol per row and keeps the
//                          M windows it belongs to in M rotating accumulators (window w receives weight row j at step
//                          w + j: the reference's add order).  The loop is unrolled M steps: nothing is indexed dynamically.
//   walk_generic<R>        any M: the same walk, every window summed from scratch over its M symbols.
//
// A lane's run ends at the bottom of its column; the windows there read the wrap rows, i.e. the top of the next column
// (the last column's hold padding: those windows straddle or lie behind the last record).  Offsets of sets of up to 4 095
// records are staged in LDS, larger tables are read from global memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scan_stream.hpp"  // kBlock

namespace lm {

constexpr unsigned long long kNoEnd = ~0ull;

// largest r in [0, n] with off[r] <= p (off[0] == 0; r == n: p lies behind the last record).  Among empty records that
// share an offset this is the last one.
__host__ __device__ __forceinline__ unsigned long long last_record_at(const unsigned long long *off, const unsigned long long n,
                                                                       const unsigned long long p)
{
    unsigned long long lo = 0, hi = n + 1;  // first index whose offset exceeds p
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (off[mid] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

// What a lane carries down its run of consecutive positions.
template <typename R>
struct Walker {
    const unsigned long long *off;  // n + 1 offsets (LDS or global)
    unsigned long long n;           // records
    unsigned long long m;           // motif length
    typename R::Slot *slots;        // of this job
    unsigned long long rec, start, end;
    unsigned long long next;        // position of the next event
    bool competing;                 // windows before `next` lie inside the record
    R red;

    __host__ __device__ __forceinline__ void enter(unsigned long long r)
    {
        rec = r;
        start = off[r < n ? r : n];
        end = r < n ? off[r + 1] : kNoEnd;  // behind the last record: padding, nothing fits and nothing ends
        competing = true;
        next = (r < n && end - start >= m) ? end - m + 1 : start;
    }
    template <typename Job>
    __host__ __device__ __forceinline__ void begin(unsigned long long p, const Job &job)
    {
        red.begin(job);
        enter(last_record_at(off, n, p));
    }
    __host__ __device__ __forceinline__ void flush()
    {
        if (rec < n)  // (only windows inside a record are `inside`: behind the last one there is nothing to merge)
            red.flush(slots, rec, start, n);
    }
    __host__ __device__ __forceinline__ void event(unsigned long long p)
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
    // (v is consumed on the straight path, by the selects of R::window: behind a branch the compiler would sink the adds
    // that make it to here and keep every weight row of the last M steps in registers instead of M accumulators)
    __host__ __device__ __forceinline__ void take(unsigned long long p, float v, bool live = true)
    {
        if (__builtin_expect(live && p >= next, 0))
            event(p);
        red.window(p, v, live && competing);
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
// (rows [stream * T, stream * T + T)); grid.y: the jobs of one motif length.  TS: floats per symbol of the weight table in
// LDS, a multiple of 4 (16-byte aligned rows).  (seqset_count_fused<M> holds this text once more, for a register it
// would lose as a call: seqset_count.hip.  A change here is made there as well.)
template <int M, int TS, typename R, typename Job>
__device__ __forceinline__ void walk_fused(const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols,
                                           const unsigned long long rows, const unsigned long long rows_total, const unsigned K,
                                           const Job *__restrict__ jobs, const unsigned long long *__restrict__ g_offsets,
                                           const unsigned long long n_records, const int offsets_in_lds, const unsigned long long T,
                                           typename R::Slot *__restrict__ slots)
{
    constexpr int MP = 4 * ((M + 3) / 4);
    const Job job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);  // s_w[s * TS + j] = weights[j][s], zero padded
    const unsigned wbytes = (K * TS * 4u + 15u) & ~15u;
    for (unsigned i = threadIdx.x; i < K * TS; i += kBlock) {
        const unsigned s = i / TS, j = i % TS;
        s_w[i] = j < (unsigned)M ? job.dense[j * K + s] : 0.0f;
    }
    Walker<R> wk;
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
            wk.take((unsigned long long)(base + (long long)t), v, t >= (unsigned long long)(M - 1) && t < total);
        }
    }
    wk.flush();
}

// Any motif length: every window summed over its own M symbols (weights in LDS when they fit, `w_in_lds`).
template <typename R, typename Job>
__device__ __forceinline__ void walk_generic(const uint8_t *__restrict__ seq, const unsigned long long stride, const unsigned cols,
                                             const unsigned long long rows, const unsigned M, const unsigned K, const int w_in_lds,
                                             const Job *__restrict__ jobs, const unsigned long long *__restrict__ g_offsets,
                                             const unsigned long long n_records, const int offsets_in_lds, const unsigned long long T,
                                             typename R::Slot *__restrict__ slots)
{
    const Job job = jobs[blockIdx.y];
    float *s_w = reinterpret_cast<float *>(s_dyn);
    const unsigned wbytes = w_in_lds ? (M * K * 4u + 15u) & ~15u : 0u;
    if (w_in_lds)
        for (unsigned i = threadIdx.x; i < M * K; i += kBlock)
            s_w[i] = job.dense[i];
    Walker<R> wk;
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
        wk.take(col * rows + row, v);
    }
    wk.flush();
}

}  // namespace lm
