// seqset_sum_plan.hpp -- the arithmetic of seqset_sum.hip that decides WHO writes a sum of odds: the lane runs of the
// record walk, which runs the windows of a record touch, whether a flush is the only writer of its cell, the scratch of
// the partial sums and the order in which they are merged; and the term of one window.  Host- and device-compilable
// (no HIP call, no launch), so that tests/cpp/test_seqset_sum.cpp runs it with the Walker in plain C++.
//
// The walk cuts every column of the striped layout into STREAMS of T rows; lane L owns stream L / cols of column
// L % cols (seqset_walk.hpp).  In the order of the concatenation the lanes' RUNS are numbered
//       run = col * streams + stream,   streams = ceil(rows / T)
// and run `run` owns the contiguous positions [col * rows + stream * T, col * rows + min(stream * T + T, rows)), so that
//       run_of(p) = (p / rows) * streams + (p % rows) / T
// is ascending in p.  A record of L >= M symbols that starts at `start` has its windows at [start, start + L - M]: they
// touch the runs run_of(start) ... run_of(start + L - M), every one of them.
//
//   one run     the lane of that run is the only one that ever holds a window of the record: at the record's end (or
//               at the end of its run) it STORES its sum to the cell.  Nobody else writes the cell.
//   more runs   only the first and the last record of a run can be shared with a neighbouring run, so a lane has at most
//               two partial sums: `head` (the record began in an earlier run) and `tail` (it goes on in a later one); a
//               lane whose whole run lies inside one record has a head alone.  They go to the scratch of the job,
//                     scratch[2 * run]  (head)    scratch[2 * run + 1]  (tail)
//               16 bytes per run, behind the cells in the walk's block, and sum_fixup, one thread per (job, record), adds
//               tail[first run], head[first run + 1], ... head[last run] in that order and stores the cell.  Each of
//               these is written by its lane before (the lane of every run the windows touch flushes the record), so
//               the scratch needs no clearing.
//
// Every f64 addition of a cell therefore happens in an order that (rows, cols, T, M, offsets) fix: there is no
// floating-point atomic, and two calls with the same context settings give the same bits.  Another T (the option
// rows_per_stream, or another number of motifs in the call, which moves the default T) cuts the records elsewhere and
// adds the same terms in another order: the last bits of a cell may then differ (n * 2^-53 relative for n windows).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LM_SUM_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define LM_SUM_HD inline
#endif

namespace lm {
namespace setsum {

typedef unsigned long long u64;

// What a job's lanes and the fix-up know of the walk.  (rows, T, cols) are the launch's: the job table is made under the
// same lock and by the same function as the launch (walk_rows_per_lane), `run_cap` is what the scratch was sized for.
struct Geometry {
    u64 rows;     // of a column (without the wrap rows)
    u64 T;        // rows per stream
    u64 streams;  // ceil(rows / T)
    u64 run_cap;  // runs the job's scratch holds: nothing is written or read at or behind it
    unsigned cols;
    unsigned m;   // motif length
};

LM_SUM_HD u64 streams_of(u64 rows, u64 T) { return (rows + T - 1) / T; }
LM_SUM_HD u64 runs_of(u64 rows, u64 T, u64 cols) { return streams_of(rows, T) * cols; }
LM_SUM_HD size_t slots_per_job(size_t records, u64 run_cap) { return records + 2 * (size_t)run_cap; }

LM_SUM_HD u64 run_of(const Geometry &g, u64 p) { return (p / g.rows) * g.streams + (p % g.rows) / g.T; }
LM_SUM_HD u64 run_of_lane(const Geometry &g, u64 lane) { return (lane % g.cols) * g.streams + lane / g.cols; }
LM_SUM_HD u64 run_begin(const Geometry &g, u64 run) { return (run / g.streams) * g.rows + (run % g.streams) * g.T; }
LM_SUM_HD u64 run_end(const Geometry &g, u64 run)
{
    const u64 r0 = (run % g.streams) * g.T;
    return (run / g.streams) * g.rows + (r0 + g.T < g.rows ? r0 + g.T : g.rows);
}

enum Target { kNone, kCell, kHead, kTail };

// Where the lane of run [p0, p1) puts what it gathered of the record [start, end): nowhere when the record has no window
// (the lane gathered nothing and the cell keeps its zero).
LM_SUM_HD Target flush_target(u64 start, u64 end, unsigned m, u64 p0, u64 p1)
{
    if (end - start < m)
        return kNone;
    if (start < p0)
        return kHead;
    return end - m < p1 ? kCell : kTail;
}

// 2^x as a double for a finite or infinite f32 x, NaN excluded by the caller: x = i + f with i = rint(x) and f = x - i in
// [-1/2, 1/2], exact in f32; 2^f in f32 (one v_exp_f32 on the device: 1 ulp), widened, and scaled by 2^i in f64, which
// neither overflows nor flushes while the value is a double (denormals included).  |x| is clamped to 2 000 first: 2^2000
// is +inf and 2^-2000 is 0 in f64 as well, and the clamp keeps i an int and f finite (-inf gives 0, +inf gives +inf).
LM_SUM_HD double exp2_wide(float x)
{
    const float xc = x < -2000.0f ? -2000.0f : x > 2000.0f ? 2000.0f : x;
#if defined(__HIP_DEVICE_COMPILE__)
    const float i = __builtin_rintf(xc);
    const float e = __builtin_amdgcn_exp2f(xc - i);
    return __builtin_amdgcn_ldexp((double)e, (int)i);
#else
    if (xc != xc)  // (the device converts a NaN to 0 and the caller drops the term)
        return 0.0;
    const float i = std::rint(xc);
    return std::ldexp((double)std::exp2(xc - i), (int)i);
#endif
}

// Job is { dense, slot_base, scratch_off, offsets, Geometry geo, scale, lane_id() }.  LaneId answers, when called, the
// caller's lane index of the walk: on the device it reads blockIdx / threadIdx again (seqset_sum.hip: no register is held
// for it between the flushes), the host test hands a number over.  A lane keeps ONE f64 accumulator; where its run lies
// is worked out at a flush, once or twice per lane, not carried down the run.
template <typename LaneId>
struct SumReducerT {
    typedef double Slot;
    Geometry geo;
    u64 scratch_off;     // doubles from the job's cells to its { head, tail } pairs
    const u64 *offsets;  // n + 1, global memory: read at a flush, once per record and lane
    float scale;
    LaneId lane;
    double acc;  // of the current record, by this lane, in ascending position

    template <typename Job>
    LM_SUM_HD void begin(const Job &job)
    {
        geo = job.geo;
        offsets = job.offsets;
        scratch_off = job.scratch_off;
        scale = job.scale;
        lane = job.lane_id();
        acc = 0.0;
    }
    LM_SUM_HD void window(u64, float v, bool inside)
    {
        const double term = exp2_wide(scale * v);
        acc += (inside && v == v) ? term : 0.0;  // a NaN window adds nothing
    }
    LM_SUM_HD void flush(Slot *slots, u64 rec, u64 start, u64)
    {
        const u64 end = offsets[rec + 1];
        if (end - start >= geo.m) {  // (a record without a window: nothing was gathered, the cell keeps its zero)
            const u64 run = run_of_lane(geo, lane());
            const Target t = flush_target(start, end, geo.m, run_begin(geo, run), run_end(geo, run));
            if (t == kCell)
                slots[rec] = acc;
            else if (run < geo.run_cap)
                slots[scratch_off + 2 * run + (t == kTail ? 1 : 0)] = acc;
        }
        acc = 0.0;
    }
};

// The cell of a record whose windows touch more than one run: the partial sums in ascending run order.  False (and
// nothing read) when the record has no window or a single writer.
LM_SUM_HD bool merge_record(const Geometry &g, const double *scratch, u64 start, u64 end, double *sum)
{
    if (end - start < g.m)
        return false;
    const u64 a = run_of(g, start), b = run_of(g, end - g.m);
    if (a == b || b >= g.run_cap)
        return false;
    double s = scratch[2 * a + 1];
    for (u64 k = a + 1; k <= b; ++k)
        s += scratch[2 * k];
    *sum = s;
    return true;
}

}  // namespace setsum
}  // namespace lm
