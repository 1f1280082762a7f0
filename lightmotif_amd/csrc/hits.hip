// hits.hip -- puts the hit list of the fused threshold kernels in key order ON THE DEVICE.
//
// The fused kernels append (key, score) records with atomics, i.e. in no particular
// order, while the reference's Threshold pushes cells in row-major order
// (pli/mod.rs:212-218) and its Scanner yields positions in sequence order.  Keys are
// unique (every cell is reported once) and live in a bounded universe --
// key = (job << 40) | low, low < cells of the job -- so ordering is a bucket sort:
//
//   1. hits_bucket_count    bucket = job * nb + (low >> shift); histogram with atomics
//   2. exclusive scan of the histogram (launch_scan_u32, reduce.hip)
//   3. hits_bucket_scatter  records grouped by bucket (any order inside a bucket)
//   4. hits_rank_emit       rank of a record inside its bucket = number of smaller
//                           keys there; the final slot is bucket start + rank, written
//                           directly in the caller's output format
//
// Short lists of ONE job skip steps 1 and 2 as launches: the re-scoring kernel counts while it stores, every workgroup
// of the scatter scans the histogram itself (ShortOrder, below).
//
// Long lists (the JASPAR batch leaves 2.6 M hits, a non-i.i.d. genome 4.6 M) take a different road.  The histogram and the
// scatter are one device-scope atomic per record on buckets whose geometry assumes an even hit density: fine on uniform input
// (0.15 + 0.19 + 0.07 ms for 2.6 M records), but where hits cluster -- low-complexity tracts, short motifs -- or the expected
// count is off (a context's first call: 2.2 + 2.4 + 0.9 ms) the atomics pile up on few addresses.  From kSortFrom records on
// the keys are radix-sorted instead (rocPRIM's device radix sort, LDS-privatised digit histograms: 0.32 ms for 2.6 M (key, value)
// pairs on 52 bits, tools/kbench/radix_sort_bench.hip; insensitive to the distribution): hits_split (records -> key / value
// arrays, unused slots = an all-ones sentinel that sorts last), the sort, hits_sorted_emit (caller's output format),
// hits_sorted_starts (lower bound of every job's first key).  JASPAR batch: 17.6 vs 17.7 ms uniform, 21.5 vs 23.2 ms on the
// non-i.i.d. sequence (tools/sort_ab.py).
//
// `shift` is chosen from the hit density so that a bucket holds ~1 record on
// average; a bucket never holds more records than it has cells (2^shift), which bounds
// step 4 at 8 x (cells of the batch) comparisons whatever the distribution of hits.
//
// The host half is three steps.  hits_plan.hpp (pure arithmetic, tested on the CPU by tests/cpp/test_hits_plan.cpp)
// chooses the form -- Short, Buckets or Sorted -- and lays out ctx->scratch2 and the pinned staging block as named
// regions; `enqueue` launches the kernels of that plan; `deliver` reads counters and job starts, decides the outcome and
// fills the caller's arrays.  Two entry points: order_hits_speculative (enqueued behind the scans before the host knows
// the count; reports Done, Overflow or TooCoarse with the counts) and order_hits_counted (the count is known; nothing
// to report but the list).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "score_kernels.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace lm {

namespace {

using namespace hits;  // constants, geometry and layouts: hits_plan.hpp
static_assert(kBlock == kPlanBlock && sizeof(HitRecord) == kRecordBytes, "hits_plan.hpp plans for these kernels");

__device__ __forceinline__ unsigned long long bucket_of(unsigned long long key, int shift,
                                                        unsigned long long nb)
{
    return (key >> 40) * nb + ((key & kLowMask) >> shift);
}

__device__ __forceinline__ unsigned long long bucket_start(
    unsigned long long b, unsigned long long nbuckets, unsigned long long count,
    const unsigned long long *__restrict__ offsets, const unsigned long long *__restrict__ tiles)
{
    return b < nbuckets ? tiles[b / kScanTile] + offsets[b] : count;
}

// Every kernel reads the record count from the device counter the scans bumped (clamped to
// the list capacity), so the ordering can be enqueued BEFORE the host knows the count.
__device__ __forceinline__ unsigned long long live_count(const unsigned long long *count_ptr,
                                                         const unsigned long long cap)
{
    const unsigned long long n = *count_ptr;
    return n < cap ? n : cap;
}

__global__ __launch_bounds__(kBlock) void hits_bucket_count(const HitRecord *__restrict__ hits,
                                                            const unsigned long long *__restrict__ count_ptr,
                                                            const unsigned long long cap,
                                                            const int shift,
                                                            const unsigned long long nb,
                                                            unsigned *__restrict__ counts)
{
    const unsigned long long count = live_count(count_ptr, cap);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (unsigned long long)gridDim.x * kBlock)
        atomicAdd(&counts[bucket_of(hits[i].key, shift, nb)], 1u);
}

__global__ __launch_bounds__(kBlock) void hits_bucket_scatter(
    const HitRecord *__restrict__ hits, const unsigned long long *__restrict__ count_ptr,
    const unsigned long long cap, const int shift,
    const unsigned long long nb, const unsigned long long *__restrict__ offsets,
    const unsigned long long *__restrict__ tiles, unsigned *__restrict__ counts,
    HitRecord *__restrict__ grouped)
{
    const unsigned long long count = live_count(count_ptr, cap);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (unsigned long long)gridDim.x * kBlock) {
        const HitRecord r = hits[i];
        const unsigned long long b = bucket_of(r.key, shift, nb);
        const unsigned left = atomicSub(&counts[b], 1u);  // counts down to 0
        grouped[tiles[b / kScanTile] + offsets[b] + left - 1] = r;
    }
}

// EMIT 0: lm_hip_coords {low / cols, low % cols} + score (Threshold, pli/mod.rs:215)
// EMIT 1: lm_hip_hit {low, score} (Scanner: low is the sequence position)
// EMIT 2: the record itself, key included, into `out_hits` (a device list for the segment pass of seqset.hip)
template <int EMIT>
__global__ __launch_bounds__(kBlock) void hits_rank_emit(
    const HitRecord *__restrict__ grouped, const unsigned long long *__restrict__ count_ptr,
    const unsigned long long cap, const int shift,
    const unsigned long long nb, const unsigned long long nbuckets,
    const unsigned long long *__restrict__ offsets, const unsigned long long *__restrict__ tiles,
    const unsigned long long cols, lm_hip_coords *__restrict__ coords, float *__restrict__ values,
    lm_hip_hit *__restrict__ out_hits, const unsigned long long max_bucket, unsigned *__restrict__ abort_flag,
    void *__restrict__ pre_out, float *__restrict__ pre_values, const unsigned long long pre,
    const unsigned long long njobs, unsigned long long *__restrict__ starts, unsigned long long *__restrict__ header,
    unsigned *__restrict__ clean_counts, unsigned *__restrict__ clean_cursors, unsigned long long *__restrict__ clean_counters,
    unsigned *__restrict__ done_ticket, unsigned *__restrict__ done_flag, const unsigned generation)
{
    const unsigned long long count = live_count(count_ptr, cap);
    if (clean_counts) {  // ShortOrder: nothing reads the histogram, the cursors or the list's own counters any more (`count_ptr`
                         // is their copy); the next call finds them zero
        for (unsigned long long b = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; b < nbuckets;
             b += (unsigned long long)gridDim.x * kBlock) {
            clean_counts[b] = 0u;
            clean_cursors[b] = 0u;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            clean_counters[0] = 0ull;
            clean_counters[1] = 0ull;
        }
    }
    if (starts && blockIdx.x == 0) {  // few jobs: the job offsets and the raw counters ride along (no launch of their own)
        if (threadIdx.x == 0 && header) {
            header[0] = count_ptr[0];
            header[1] = count_ptr[1];
        }
        for (unsigned long long j = threadIdx.x; j <= njobs; j += kBlock)
            starts[j] = bucket_start(j * nb, nbuckets, count, offsets, tiles);
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (unsigned long long)gridDim.x * kBlock) {
        const HitRecord r = grouped[i];
        const unsigned long long b = bucket_of(r.key, shift, nb);
        const unsigned long long lo = bucket_start(b, nbuckets, count, offsets, tiles);
        const unsigned long long hi = bucket_start(b + 1, nbuckets, count, offsets, tiles);
        if (hi - lo > max_bucket) {  // the bucket geometry was guessed far too coarse: give up, the
            *abort_flag = 1u;        // host re-runs the ordering with the true count
            continue;
        }
        unsigned long long rank = 0;
        for (unsigned long long k = lo; k < hi; ++k) {
            const unsigned long long other = grouped[k].key;
            rank += (other < r.key) || (other == r.key && k < i);
        }
        const unsigned long long pos = lo + rank;
        const unsigned long long low = r.key & kLowMask;
        if (EMIT == 0) {
            lm_hip_coords c;
            c.row = low / cols;
            c.col = low - c.row * cols;
            coords[pos] = c;
            values[pos] = r.value;
            if (pos < pre) {  // the head of the list is mirrored into the staging block
                static_cast<lm_hip_coords *>(pre_out)[pos] = c;
                pre_values[pos] = r.value;
            }
        } else if (EMIT == 1) {
            lm_hip_hit h;
            h.position = low;
            h.score = r.value;
            out_hits[pos] = h;
            if (pos < pre)
                static_cast<lm_hip_hit *>(pre_out)[pos] = h;
        } else {
            reinterpret_cast<HitRecord *>(out_hits)[pos] = r;
        }
    }
    // ShortOrder: the host polls a word in the pinned staging block instead of waiting for the kernel's completion signal
    // (~10 us of a 90-250 us call).  Every workgroup makes its writes -- to the pinned block as well -- visible system-wide,
    // then takes a ticket; the last one resets the ticket for the next call and releases `generation` into the word.
    if (done_flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned t = __hip_atomic_fetch_add(done_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (t == gridDim.x - 1) {
                __hip_atomic_store(done_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(done_flag, generation, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

__global__ void hits_job_starts(const unsigned long long njobs, const unsigned long long nb,
                                const unsigned long long nbuckets,
                                const unsigned long long *__restrict__ count_ptr, const unsigned long long cap,
                                const unsigned long long *__restrict__ offsets,
                                const unsigned long long *__restrict__ tiles,
                                unsigned long long *__restrict__ starts,
                                unsigned long long *__restrict__ header)
{
    const unsigned long long count = live_count(count_ptr, cap);
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && header) {  // raw counters {hits, candidates} for the host
        header[0] = count_ptr[0];
        header[1] = count_ptr[1];
    }
    if (j <= njobs)
        starts[j] = bucket_start(j * nb, nbuckets, count, offsets, tiles);
}

// ---- short lists of one job (ShortOrder) ---------------------------------------------------------------------
//
// Each launch of the tail costs 2-5 us whatever it does (5 as the profiler shows them), and a 1 Gbp scan at p = 1e-5 spent
// 28 of its 280 us in the five above (fill, count, scan, scatter, rank: profiles/r05_timeline_fused.txt), a copy-in of
// zeroed counters + the job table before its scan; a 5 Mbp scan spends more there than in its scan.  For ONE job with a short
// list expected:
//   * the re-scoring kernel bumps the bucket count of every record it stores (rescore_candidates);
//   * hits_short_scatter: every workgroup scans the whole histogram in LDS (<= kShortBuckets counts), workgroup 0
//     publishes the offsets, records go to offset + cursor++;
//   * hits_rank_emit as above, which also clears counts and cursors: the buffers are zero between calls (ctx->d_short,
//     ctx->short_dirty covers calls that failed in between);
//   * the list's counters {hits, candidates} live there as well: the scatter kernel leaves a copy for the ranking kernel,
//     which clears the originals -- the next scan starts without a head block copied in, its job an argument of the
//     re-scoring kernel.
// (kShortRecords, kShortBuckets and the layout of ctx->d_short: hits_plan.hpp)

__global__ __launch_bounds__(kBlock) void hits_short_scatter(
    const HitRecord *__restrict__ hits, const unsigned long long *__restrict__ count_ptr, const unsigned long long cap,
    const int shift, const unsigned nb, const unsigned *__restrict__ counts, unsigned *__restrict__ cursors,
    unsigned long long *__restrict__ offsets, HitRecord *__restrict__ grouped, unsigned long long *__restrict__ counters_copy)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // what the ranking kernel reads while it clears the counters themselves
        counters_copy[0] = count_ptr[0];
        counters_copy[1] = count_ptr[1];
    }
    constexpr int PER = kShortBuckets / kBlock;  // buckets per thread, contiguous
    __shared__ unsigned pre[kShortBuckets];
    __shared__ unsigned wave_sum[kBlock / 64];
    unsigned v[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const unsigned b = threadIdx.x * PER + k;
        v[k] = b < nb ? counts[b] : 0u;
        sum += v[k];
    }
    unsigned inc = sum;  // inclusive scan over the wavefront
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(inc, off);
        if (lane >= off)
            inc += o;
    }
    if (lane == 63)
        wave_sum[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned run = inc - sum;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w)
        run += wave_sum[w];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        pre[threadIdx.x * PER + k] = run;
        run += v[k];
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (unsigned b = threadIdx.x; b < nb; b += kBlock)
            offsets[b] = pre[b];
    const unsigned long long count = live_count(count_ptr, cap);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (unsigned long long)gridDim.x * kBlock) {
        const HitRecord r = hits[i];
        const unsigned b = (unsigned)((r.key & kLowMask) >> shift);
        grouped[pre[b] + atomicAdd(&cursors[b], 1u)] = r;
    }
}

__global__ __launch_bounds__(kBlock) void hits_split(const HitRecord *__restrict__ hits,
                                                     const unsigned long long *__restrict__ count_ptr,
                                                     const unsigned long long cap, const unsigned long long n_sort,
                                                     unsigned long long *__restrict__ keys, float *__restrict__ values,
                                                     unsigned *__restrict__ abort_flag)
{
    const unsigned long long count = live_count(count_ptr, cap);
    if (count > n_sort) {  // more records than the arrays were sized for (speculative form): the host runs the exact form
        if (blockIdx.x == 0 && threadIdx.x == 0 && abort_flag)
            *abort_flag = 1u;
        return;
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < n_sort;
         i += (unsigned long long)gridDim.x * kBlock) {
        if (i < count) {
            const HitRecord r = hits[i];
            keys[i] = r.key;
            values[i] = r.value;
        } else {
            keys[i] = ~0ull;
        }
    }
}

template <int EMIT>
__global__ __launch_bounds__(kBlock) void hits_sorted_emit(
    const unsigned long long *__restrict__ keys, const float *__restrict__ vals,
    const unsigned long long *__restrict__ count_ptr, const unsigned long long cap, const unsigned long long n_sort,
    const unsigned long long cols, lm_hip_coords *__restrict__ coords, float *__restrict__ values,
    lm_hip_hit *__restrict__ out_hits, void *__restrict__ pre_out, float *__restrict__ pre_values,
    const unsigned long long pre, unsigned long long *__restrict__ header)
{
    unsigned long long count = live_count(count_ptr, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0 && header) {  // raw counters {hits, candidates} for the host
        header[0] = count_ptr[0];
        header[1] = count_ptr[1];
    }
    if (count > n_sort)
        return;  // (hits_split raised the abort flag)
    for (unsigned long long pos = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; pos < count;
         pos += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long low = keys[pos] & kLowMask;
        const float v = vals[pos];
        if (EMIT == 0) {
            lm_hip_coords c;
            c.row = low / cols;
            c.col = low - c.row * cols;
            coords[pos] = c;
            values[pos] = v;
            if (pos < pre) {
                static_cast<lm_hip_coords *>(pre_out)[pos] = c;
                pre_values[pos] = v;
            }
        } else if (EMIT == 1) {
            lm_hip_hit h;
            h.position = low;
            h.score = v;
            out_hits[pos] = h;
            if (pos < pre)
                static_cast<lm_hip_hit *>(pre_out)[pos] = h;
        } else {
            HitRecord r;
            r.key = keys[pos];
            r.value = v;
            r.pad = 0;
            reinterpret_cast<HitRecord *>(out_hits)[pos] = r;
        }
    }
}

// starts[j] = number of keys below (j << 40): lower bound in the sorted keys (sentinels sort behind every real key)
__global__ void hits_sorted_starts(const unsigned long long *__restrict__ keys,
                                   const unsigned long long *__restrict__ count_ptr, const unsigned long long cap,
                                   const unsigned long long n_sort, const unsigned long long njobs,
                                   unsigned long long *__restrict__ starts)
{
    const unsigned long long count = std::min(live_count(count_ptr, cap), n_sort);
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > njobs)
        return;
    const unsigned long long want = j << 40;
    unsigned long long lo = 0, hi = count;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) / 2;
        if (keys[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    starts[j] = lo;
}

// ---- host: plan (hits_plan.hpp) -> enqueue -> deliver --------------------------------------------------------------

// the regions of a plan as pointers into ctx->scratch2, ctx->d_short and the pinned staging block
struct Buffers {
    char *base, *pin;
    // Short: histogram, offsets and the (zero) tiles live in the context, with the cursors; otherwise in the work area
    unsigned *counts, *cursors;
    unsigned long long *offsets, *tiles;
    unsigned long long *header;  // pinned: the raw counters {hits, candidates}
    unsigned *abort_flag;        // pinned
    void *pre_out;               // pinned: head of the result
    float *pre_values;
    unsigned long long *starts;      // of the ordering: pinned when speculative and the result's own, else on the device
    unsigned long long *seg_starts;  // of the segment pass: pinned when speculative
    void *d_out;
    float *d_values;
    lm_hip_set_hit *d_set;
    // Short with option "poll_done": the word hits_rank_emit's last workgroup raises, its ticket, the value to wait for
    unsigned *done_ticket = nullptr, *done_flag = nullptr;
    unsigned generation = 0;
};

template <class T>
T *at(char *block, const Region &r) { return reinterpret_cast<T *>(block + r.off); }

Buffers carve(lm_hip_ctx *ctx, const Plan &p, bool speculative, Output output)
{
    Buffers b{};
    b.base = static_cast<char *>(ctx->scratch2.ptr);
    b.pin = pinned_at<char>(ctx, kPinHitStaging, 0);  // (the counted form reads back through kPinHitReadback, the same bytes)
    if (p.form == Form::Short) {
        char *sb = reinterpret_cast<char *>(ctx->d_short);
        b.counts = reinterpret_cast<unsigned *>(sb);
        b.cursors = b.counts + kShortBuckets;
        b.tiles = reinterpret_cast<unsigned long long *>(sb + kShortOffTiles);
        b.offsets = reinterpret_cast<unsigned long long *>(sb + kShortOffOffsets);
    } else {
        b.counts = at<unsigned>(b.base, p.buckets.counts);
        b.offsets = at<unsigned long long>(b.base, p.buckets.offsets);
        b.tiles = at<unsigned long long>(b.base, p.buckets.tiles);
    }
    b.header = reinterpret_cast<unsigned long long *>(b.pin);
    b.abort_flag = reinterpret_cast<unsigned *>(b.pin + Plan::p_abort);
    b.pre_out = b.pin + p.p_out;
    b.pre_values = reinterpret_cast<float *>(b.pin + p.p_values);
    unsigned long long *pin_starts = reinterpret_cast<unsigned long long *>(b.pin + Plan::p_starts);
    // with a segment pass the ordering's own starts stay on the device (unused); the starts of the compacted list take their place
    b.starts = speculative && output != Output::Records ? pin_starts : at<unsigned long long>(b.base, p.starts);
    b.seg_starts = speculative ? pin_starts : at<unsigned long long>(b.base, p.seg_starts);
    b.d_out = b.base + p.out.off;
    b.d_values = at<float>(b.base, p.values);
    b.d_set = at<lm_hip_set_hit>(b.base, p.seg_out);
    // short form, option "poll_done" = 1: the end of the call is polled (hits_rank_emit's last workgroup; the word sits in the
    // zeroed head of the staging block, the ticket next to the context's counters) instead of waited for on the stream.
    // 2.6-4.4 us less per call when nothing synchronises behind it -- and ~13 us MORE when the caller follows the call with a
    // device synchronisation of its own, which then finds the ranking kernel still retiring and pays a full wake-up
    // (bench.py's protocol does: 0.252 -> 0.265 ms).  Hence off unless asked for (profiles/r06_poll_done_ab.txt).
    if (p.form == Form::Short && speculative && ctx->poll_done) {
        b.done_ticket = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(ctx->d_short) + kShortOffTicket);
        b.done_flag = reinterpret_cast<unsigned *>(b.pin + Plan::p_done);
        b.generation = next_generation(ctx->short_generation);
    }
    return b;
}

// hipLaunchKernelGGL of KERNEL<0 | 1 | 2> by the output kind
#define LM_LAUNCH_BY_OUTPUT(KERNEL, output, ...)                                   \
    do {                                                                           \
        if ((output) == Output::Coords)                                            \
            hipLaunchKernelGGL(KERNEL<0>, __VA_ARGS__);                            \
        else if ((output) == Output::Records)                                      \
            hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__);                            \
        else                                                                       \
            hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__);                            \
    } while (0)

// the kernels of a plan, on ctx->stream
int enqueue(lm_hip_ctx *ctx, const Plan &p, const Buffers &b, const HitList &list, const HitShape &shape, bool speculative,
            const ShortOrder *so, const SegmentCut *cut, size_t sort_temp)
{
    hipStream_t st = ctx->stream;
    const dim3 grid(p.grid), block(kBlock);
    const unsigned long long njobs = shape.njobs, cols = shape.cols, cap = list.cap;
    const unsigned long long *d_counters = list.d_counters;
    // Coords write coords + values, the other two kinds whole 16-byte entries through `out_hits`
    lm_hip_coords *coords = shape.output == Output::Coords ? static_cast<lm_hip_coords *>(b.d_out) : nullptr;
    float *values = shape.output == Output::Coords ? b.d_values : nullptr;
    lm_hip_hit *out_hits = shape.output == Output::Coords ? nullptr : static_cast<lm_hip_hit *>(b.d_out);
    unsigned long long *header = speculative ? b.header : nullptr;
    if (p.form == Form::Sorted) {
        unsigned long long *keys_in = at<unsigned long long>(b.base, p.sort.keys_in), *keys_out = at<unsigned long long>(b.base, p.sort.keys_out);
        float *vals_in = at<float>(b.base, p.sort.vals_in), *vals_out = at<float>(b.base, p.sort.vals_out);
        hipLaunchKernelGGL(hits_split, grid, block, 0, st, list.d_hits, d_counters, cap, p.n_sort, keys_in, vals_in,
                           speculative ? b.abort_flag : static_cast<unsigned *>(nullptr));
        LM_HIP_TRY(hipGetLastError());
        size_t tb = sort_temp;
        LM_HIP_TRY(rocprim::radix_sort_pairs(b.base + p.sort.temp.off, tb, keys_in, keys_out, vals_in, vals_out, (size_t)p.n_sort, 0u,
                                             (unsigned)p.end_bit, st));
        LM_LAUNCH_BY_OUTPUT(hits_sorted_emit, shape.output, grid, block, 0, st, keys_out, vals_out, d_counters, cap, p.n_sort, cols,
                            coords, values, out_hits, b.pre_out, b.pre_values, p.order_pre, header);
        hipLaunchKernelGGL(hits_sorted_starts, dim3(p.starts_grid), dim3(256), 0, st, keys_out, d_counters, cap, p.n_sort, njobs, b.starts);
        LM_HIP_TRY(hipGetLastError());
    } else {
        const bool short_form = p.form == Form::Short;
        HitRecord *grouped = at<HitRecord>(b.base, p.buckets.grouped);
        const unsigned long long *rank_counters = short_form ? so->counters_copy : d_counters;
        if (short_form) {  // the re-scoring kernel has counted
            hipLaunchKernelGGL(hits_short_scatter, grid, block, 0, st, list.d_hits, d_counters, cap, p.shift, (unsigned)p.nb, b.counts,
                               b.cursors, b.offsets, grouped, so->counters_copy);
        } else {
            LM_HIP_TRY(hipMemsetAsync(b.counts, 0, p.buckets.counts.bytes, st));  // whole 256-B units: one fill kernel
            hipLaunchKernelGGL(hits_bucket_count, grid, block, 0, st, list.d_hits, d_counters, cap, p.shift, p.nb, b.counts);
            LM_TRY(launch_scan_u32(ctx, b.counts, p.nbuckets, b.offsets, b.tiles, at<unsigned long long>(b.base, p.total)));
            hipLaunchKernelGGL(hits_bucket_scatter, grid, block, 0, st, list.d_hits, d_counters, cap, p.shift, p.nb, b.offsets, b.tiles,
                               b.counts, grouped);
        }
        LM_LAUNCH_BY_OUTPUT(hits_rank_emit, shape.output, grid, block, 0, st, grouped, rank_counters, cap, p.shift, p.nb, p.nbuckets,
                            b.offsets, b.tiles, cols, coords, values, out_hits, p.max_bucket, b.abort_flag, b.pre_out, b.pre_values,
                            p.order_pre, njobs, p.inline_starts ? b.starts : nullptr, p.inline_starts ? header : nullptr,
                            short_form ? b.counts : nullptr, b.cursors, short_form ? so->counters : nullptr, b.done_ticket, b.done_flag,
                            b.generation);
        if (!p.inline_starts)
            hipLaunchKernelGGL(hits_job_starts, dim3(p.starts_grid), dim3(256), 0, st, njobs, p.nb, p.nbuckets, d_counters, cap, b.offsets,
                               b.tiles, b.starts, header);
        LM_HIP_TRY(hipGetLastError());
    }
    if (cut)  // drop the windows that leave their record, make the others record-relative, per-job starts anew (seqset.hip)
        LM_TRY(launch_segment_cut(st, static_cast<const HitRecord *>(b.d_out), d_counters, p.form == Form::Sorted ? p.n_sort : p.room, njobs,
                                  *cut, p.seg_grid, at<unsigned>(b.base, p.seg_counts), b.seg_starts, b.d_set,
                                  static_cast<lm_hip_set_hit *>(b.pre_out), p.pre));
    scan_timer_mark(ctx, st, 3);  // (time_scan) behind the ordering kernels
    return LM_HIP_OK;
}

// What the kernels left, into host arrays for the caller.  Speculative: ONE synchronisation (or the polled word), the
// counters decide the outcome, the head of the list is in the staging block already and only a long list's remainder is
// copied from the device.  Counted: starts | records | values in one pinned block copy when they are few, else straight
// into the caller's arrays.  With a segment pass the list is the compacted one and its length the last of its starts.
int deliver(lm_hip_ctx *ctx, const Plan &p, const Buffers &b, const HitList &list, const HitShape &shape, unsigned long long count,
            HitOutput *out, SpeculativeOrder *spec)
{
    hipStream_t st = ctx->stream;
    const bool records = shape.output == Output::Records;
    const size_t njobs = shape.njobs, starts_bytes = (njobs + 1) * 8;
    static_assert(sizeof(size_t) == 8, "job offsets are read back as 64-bit values");
    // 1. counters and starts
    if (spec) {
        // the ranking kernel's last workgroup raises the word behind everything it and the others wrote
        const bool seen = b.done_flag && poll_generation(b.done_flag, b.generation, 1u << 23);  // bounded: a kernel that never gets there is caught below
        if (!seen || ctx->scan_timed)  // (option "time_scan": the events behind the kernels are read next -- they must have completed)
            LM_HIP_TRY(hipStreamSynchronize(st));
        if (p.form == Form::Short)
            ctx->short_dirty = false;  // both kernels ran: counts and cursors are zero again
        spec->hits = b.header[0];
        spec->candidates = b.header[1];
        // 2. the outcome
        if (spec->hits > list.cap || spec->candidates > list.cand_cap) {
            spec->outcome = SpeculativeOrder::Overflow;
            return LM_HIP_OK;
        }
        if (*b.abort_flag) {
            spec->outcome = SpeculativeOrder::TooCoarse;
            return LM_HIP_OK;
        }
        count = spec->hits;
        if (count == 0)
            return LM_HIP_OK;
        memcpy(out->job_start.data(), b.pin + Plan::p_starts, starts_bytes);
    } else if (records) {
        LM_HIP_TRY(hipMemcpyAsync(out->job_start.data(), b.seg_starts, starts_bytes, hipMemcpyDeviceToHost, st));
        LM_HIP_TRY(hipStreamSynchronize(st));
    }
    if (records) {
        count = out->job_start[njobs];
        if (count > p.room)
            return fail(LM_HIP_ERR_HIP, "fused threshold: the segment pass reports %llu of %llu hits", count, p.room);
        if (count == 0)
            return LM_HIP_OK;
    }
    // 3. the caller's arrays
    const size_t rec_bytes = records ? sizeof(lm_hip_set_hit) : p.rec_bytes;
    const char *d_list = records ? reinterpret_cast<const char *>(b.d_set) : static_cast<const char *>(b.d_out);
    ResultArray<char> host((size_t)count * rec_bytes);
    ResultArray<float> host_values;
    if (shape.output == Output::Coords)
        host_values.p = static_cast<float *>(result_alloc(count * sizeof(float)));
    if (!host.p || (shape.output == Output::Coords && !host_values.p))
        return fail(LM_HIP_ERR_OOM, "fused threshold: cannot allocate %llu hits on the host", count);
    // 4. the head from the staging block
    const unsigned long long have = spec ? std::min(count, p.pre) : 0;
    memcpy(host.p, b.pin + p.p_out, have * rec_bytes);
    if (host_values.p)
        memcpy(host_values.p, b.pin + p.p_values, have * sizeof(float));
    // 5. the rest from the device
    hipError_t e = hipSuccess;
    if (!spec && !records) {
        if (p.readback_pinned) {
            e = hipMemcpyAsync(b.pin, b.base + p.starts.off, p.readback_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e == hipSuccess) {
                memcpy(out->job_start.data(), b.pin, starts_bytes);
                memcpy(host.p, b.pin + (p.out.off - p.starts.off), count * rec_bytes);
                if (host_values.p)
                    memcpy(host_values.p, b.pin + (p.values.off - p.starts.off), count * sizeof(float));
            }
        } else {
            e = hipMemcpyAsync(out->job_start.data(), b.starts, starts_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(host.p, d_list, count * rec_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && host_values.p)
                e = hipMemcpyAsync(host_values.p, b.d_values, count * sizeof(float), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess)
            return fail(LM_HIP_ERR_HIP, "fused threshold: ordering the hit list failed: %s", hipGetErrorString(e));
    } else if (count > have) {  // long list: the rest comes straight from the device
        e = hipMemcpyAsync(host.p + have * rec_bytes, d_list + have * rec_bytes, (count - have) * rec_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && host_values.p)
            e = hipMemcpyAsync(host_values.p + have, b.d_values + have, (count - have) * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return fail(LM_HIP_ERR_HIP, "fused threshold: read-back failed: %s", hipGetErrorString(e));
    }
    out->total = (size_t)count;
    out->values = host_values.release();
    if (records)
        out->set_hits = reinterpret_cast<lm_hip_set_hit *>(host.release());
    else if (shape.output == Output::Coords)
        out->coords = reinterpret_cast<lm_hip_coords *>(host.release());
    else
        out->hits = reinterpret_cast<lm_hip_hit *>(host.release());
    return LM_HIP_OK;
}

// plan, enqueue, deliver.  spec != nullptr: speculative, `count` = the expected records.
int order_hits(lm_hip_ctx *ctx, const HitList &list, const HitShape &shape, unsigned long long count, const ShortOrder *so,
               const SegmentCut *cut, HitOutput *out, SpeculativeOrder *spec)
{
    static_assert(sizeof(HitRecord) == sizeof(lm_hip_hit), "Output::Records writes records where Output::Hits writes lm_hip_hit");
    const bool short_on = so && so->on;
    if ((cut != nullptr) != (shape.output == Output::Records) || (cut && short_on))
        return fail(LM_HIP_ERR_BAD_ARGS, "fused threshold: the segment pass needs position keys and the long ordering");
    out->job_start.assign(shape.njobs + 1, 0);
    out->total = 0;
    out->ordering = "none/counted";
    if (!spec && count == 0)
        return LM_HIP_OK;
    if (shape.max_low > kLowMask + 1)
        return fail(LM_HIP_ERR_CAPACITY, "fused threshold: %llu cells per job exceed the 2^40 key space", shape.max_low);
    Request rq;
    rq.speculative = spec != nullptr;
    rq.count = count;
    rq.cap = list.cap;
    rq.njobs = shape.njobs;
    rq.max_low = std::max<unsigned long long>(shape.max_low, 1);
    rq.output = shape.output;
    rq.sort_hits = ctx->sort_hits;
    rq.num_cus = (unsigned)ctx->num_cus;
    if (short_on)
        rq.short_geom = *so;
    rq.seg_waves_per_group = segment_cut_waves(1);
    rq.staging_cap = kPinHitStaging.cap;
    rq.readback_cap = kPinHitReadback.cap;
    const Geometry g = choose_form(rq);
    if (!g.short_matches || (short_on && list.d_counters != so->counters))
        return fail(LM_HIP_ERR_BAD_ARGS, "fused threshold: the short ordering was begun with another geometry");
    size_t sort_temp = 0;
    if (g.form == Form::Sorted) {  // (the seam of the plan: rocPRIM tells the size of the sort's temporary storage)
        unsigned long long *kp = nullptr;
        float *vp = nullptr;
        LM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_temp, kp, kp, vp, vp, (size_t)g.n_sort, 0u, (unsigned)g.end_bit, ctx->stream));
    }
    const Plan p = lay_out(rq, g, sort_temp);
    static const char *const kNames[2][3] = {{"short/counted", "buckets/counted", "sorted/counted"},
                                             {"short/speculative", "buckets/speculative", "sorted/speculative"}};
    out->ordering = kNames[spec ? 1 : 0][(int)p.form];
    if (spec && !p.staging_fits) {
        spec->outcome = SpeculativeOrder::TooCoarse;  // too many jobs for the staging block: the caller runs the counted form
        unsigned long long counts[2];
        LM_TRY(read_back_counters(ctx, ctx->stream, list.d_counters, counts));
        spec->hits = counts[0];
        spec->candidates = counts[1];
        if (counts[0] > list.cap || counts[1] > list.cand_cap)
            spec->outcome = SpeculativeOrder::Overflow;
        return LM_HIP_OK;
    }
    LM_TRY(ctx->scratch2.reserve(p.bytes));
    const Buffers b = carve(ctx, p, spec != nullptr, shape.output);
    if (spec)
        memset(b.pin, 0, Plan::p_head_zeroed);  // counters, abort flag and done word (the previous call's results were consumed)
    LM_TRY(enqueue(ctx, p, b, list, shape, spec != nullptr, so, cut, sort_temp));
    return deliver(ctx, p, b, list, shape, count, out, spec);
}

}  // namespace

int short_order_begin(lm_hip_ctx *ctx, unsigned long long expected, size_t njobs, unsigned long long max_low, ShortOrder *so)
{
    static_cast<ShortGeometry &>(*so) = short_geometry(expected, njobs, max_low);
    if (!so->on)
        return LM_HIP_OK;
    so->on = false;  // until the buffers stand
    if (!ctx->d_short) {
        LM_HIP_TRY(hipMalloc(&ctx->d_short, kShortBytes));
        ctx->short_dirty = false;
        LM_HIP_TRY(hipMemsetAsync(ctx->d_short, 0, kShortBytes, ctx->stream));
    } else if (ctx->short_dirty) {
        LM_HIP_TRY(hipMemsetAsync(ctx->d_short, 0, kShortBytes, ctx->stream));
    }
    ctx->short_dirty = true;  // until the ordering has seen the clean-up through
    so->counts = ctx->d_short;
    so->counters = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ctx->d_short) + kShortOffCounters);
    so->counters_copy = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ctx->d_short) + kShortOffCopy);
    so->on = true;
    return LM_HIP_OK;
}

void HitOutput::release()
{
    result_free(coords);
    result_free(values);
    result_free(hits);
    result_free(set_hits);
    set_hits = nullptr;
    coords = nullptr;
    values = nullptr;
    hits = nullptr;
    total = 0;
}

int order_hits_speculative(lm_hip_ctx *ctx, const HitList &list, const HitShape &shape, unsigned long long expected,
                           const ShortOrder *so, const SegmentCut *cut, HitOutput *out, SpeculativeOrder *result)
{
    *result = SpeculativeOrder{};
    return order_hits(ctx, list, shape, expected, so, cut, out, result);
}

int order_hits_counted(lm_hip_ctx *ctx, const HitList &list, const HitShape &shape, unsigned long long count,
                       const SegmentCut *cut, HitOutput *out)
{
    return order_hits(ctx, list, shape, count, nullptr, cut, out, nullptr);
}

}  // namespace lm
