// seqset.hip -- many sequences resident as ONE striped matrix, and the segment pass that turns the hit list of a scan
// over that matrix into per-record hits.
//
// lightmotif-cli sends every motif against every record (main.rs:502-561).  A score at position p is M sequential f32
// adds over symbols p .. p + M - 1 (pli/mod.rs:72-106), so records laid end to end in one StripedSequence
// (seq.rs:288-313, no separators) score, in every window that lies inside one record, bit for bit as they do alone.
// What the concatenation adds are windows that straddle two records or run past the last one; the reference never
// sees them because its Scanner cuts at `position + M <= L` per RECORD (scan.rs:185-190).
//
// The segment pass makes that cut ON THE DEVICE, behind the kernels of hits.hip that put the list in
// (job, position) order and before anything is read back:
//
//   seqset_cut<false>   every wavefront owns a contiguous slice of the ordered list; each hit finds its record in the
//                       offsets table (the neighbour's record first, a binary search otherwise), tests
//                       position - offsets[r] + M_job <= len(r), and the wavefront counts its survivors (ballot)
//   seqset_cut<true>    the same walk again; a wavefront's first slot = the sum of the counts before it, a hit's slot
//                       = that + the survivors before it in the wavefront (ballot prefix): a STABLE compaction, so
//                       the list stays ascending in (job, record, position) and nothing is sorted again.  The first
//                       hit of every job also writes the job's new start.
//
// The offsets of small sets are staged in LDS; larger tables are searched in global memory.
#include <algorithm>
#include <new>

#include "score_kernels.hpp"

namespace lm {

namespace {

constexpr unsigned long long kLowMask = (1ull << 40) - 1;
constexpr int kWavesPerBlock = kBlock / 64;

// largest r in [0, n] with off[r] <= p (off[0] == 0; r == n: p lies behind the last record).  `hint` is the record of
// an earlier hit of the same job, or 0.
template <typename Off>
__device__ __forceinline__ unsigned long long find_record(const Off &off, const unsigned long long n,
                                                          const unsigned long long p, unsigned long long hint)
{
    unsigned long long lo = 0;
    if (hint <= n && off(hint) <= p) {
        if (hint == n || p < off(hint + 1))
            return hint;
        if (hint + 1 == n || p < off(hint + 2))
            return hint + 1;
        lo = hint + 2;
    }
    unsigned long long hi = n + 1;  // first index in [lo, n + 1) whose offset exceeds p
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (off(mid) <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

struct GlobalOffsets {
    const unsigned long long *p;
    __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i]; }
};
struct LdsOffsets {
    const unsigned long long *p;  // (LDS)
    __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[(unsigned)i]; }
};

// WRITE = false: wave_counts[w] = survivors of wavefront w's slice.  WRITE = true: the compaction itself.
template <bool WRITE, bool LDS>
__global__ __launch_bounds__(kBlock) void seqset_cut(
    const HitRecord *__restrict__ ordered, const unsigned long long *__restrict__ count_ptr, const unsigned long long room,
    const unsigned long long njobs, const unsigned long long *__restrict__ g_offsets, const unsigned long long n_records,
    const char *__restrict__ job_m, const unsigned long long job_m_stride, unsigned *__restrict__ wave_counts,
    unsigned long long *__restrict__ starts, lm_hip_set_hit *__restrict__ out, lm_hip_set_hit *__restrict__ pre_out,
    const unsigned long long pre)
{
    __shared__ unsigned long long s_off[LDS ? kSetLdsOffsets : 1];
    __shared__ unsigned long long s_part[kBlock];
    if (LDS) {
        for (unsigned i = threadIdx.x; i <= n_records; i += kBlock)
            s_off[i] = g_offsets[i];
        __syncthreads();
    }
    const unsigned long long count = *count_ptr;
    if (count > room)  // the list overflowed, or the speculative sort was sized too small: the host runs the call again
        return;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long gw = (unsigned long long)blockIdx.x * kWavesPerBlock + wave;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * kWavesPerBlock;
    const unsigned long long per_wave = ((count + nwaves - 1) / nwaves + 63ull) & ~63ull;
    const unsigned long long begin = std::min(count, gw * per_wave), end = std::min(count, begin + per_wave);

    unsigned long long slot = 0;  // WRITE: survivors in front of this wavefront's slice
    if (WRITE) {
        unsigned long long part = 0;  // counts of the workgroups before this one
        for (unsigned long long w = threadIdx.x; w < (unsigned long long)blockIdx.x * kWavesPerBlock; w += kBlock)
            part += wave_counts[w];
        s_part[threadIdx.x] = part;
        __syncthreads();
        for (int half = kBlock / 2; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half)
                s_part[threadIdx.x] += s_part[threadIdx.x + half];
            __syncthreads();
        }
        slot = s_part[0];
        for (unsigned w = 0; w < wave; ++w)
            slot += wave_counts[(unsigned long long)blockIdx.x * kWavesPerBlock + w];
        if (count == 0 && gw == 0)  // no hits at all: every job starts (and ends) at 0
            for (unsigned long long j = lane; j <= njobs; j += 64)
                starts[j] = 0;
    }

    unsigned kept = 0;                    // survivors of the slice so far (wave-uniform)
    unsigned long long hint_rec = 0;      // record and job of the slice's previous hit
    long long prev_last_job = -1;         // WRITE: clamped job of the hit in front of this step (-1: none)
    if (WRITE && begin > 0 && begin < end)
        prev_last_job = (long long)std::min(ordered[begin - 1].key >> 40, njobs);
    unsigned long long hint_job = ~0ull;
    for (unsigned long long base = begin; base < end; base += 64) {
        const unsigned long long i = base + lane;
        const bool active = i < end;
        unsigned long long job = ~0ull, p = 0, rec = 0;
        float score = 0.0f;
        bool keep = false;
        if (active) {
            const HitRecord r = ordered[i];
            job = r.key >> 40;
            p = r.key & kLowMask;
            score = r.value;
            if (job < njobs) {  // (a list the ordering gave up on may hold anything: stay inside the tables)
                const unsigned long long m = *reinterpret_cast<const unsigned *>(job_m + job * job_m_stride);
                const unsigned long long hint = job == hint_job ? hint_rec : 0ull;
                if (LDS)
                    rec = find_record(LdsOffsets{s_off}, n_records, p, hint);
                else
                    rec = find_record(GlobalOffsets{g_offsets}, n_records, p, hint);
                if (rec < n_records) {
                    const unsigned long long rec_end = LDS ? s_off[(unsigned)rec + 1] : g_offsets[rec + 1];
                    keep = p + m <= rec_end;  // scan.rs:185-190, per record
                }
            }
        }
        const unsigned long long votes = __ballot(keep);
        if (WRITE) {
            const unsigned long long before = slot + kept + __popcll(votes & ((1ull << lane) - 1ull));
            if (keep) {
                lm_hip_set_hit h;
                h.record = rec;
                h.position = p - (LDS ? s_off[(unsigned)rec] : g_offsets[rec]);
                h.score = score;
                out[before] = h;
                if (before < pre)
                    pre_out[before] = h;
            }
            // the first hit of a job (and of every empty job in front of it) fixes where the job starts in the output
            const long long cj = (long long)std::min(job, njobs);
            long long pj = __shfl_up(cj, 1);
            if (lane == 0)
                pj = prev_last_job;
            if (active) {
                for (long long j = pj + 1; j <= cj; ++j)
                    starts[j] = before;
                if (i + 1 == count)
                    for (long long j = cj + 1; j <= (long long)njobs; ++j)
                        starts[j] = before + (keep ? 1ull : 0ull);
            }
            prev_last_job = __shfl(cj, 63);
        }
        kept += (unsigned)__popcll(votes);
        hint_rec = __shfl(rec, 63);
        hint_job = __shfl(job, 63);
    }
    if (!WRITE && lane == 0)
        wave_counts[gw] = kept;
}

}  // namespace

unsigned segment_cut_waves(unsigned grid) { return grid * (unsigned)kWavesPerBlock; }

int launch_segment_cut(hipStream_t st, const HitRecord *ordered, const unsigned long long *count_ptr, unsigned long long room,
                       unsigned long long njobs, const SegmentCut &seg, unsigned grid, unsigned *wave_counts,
                       unsigned long long *starts, lm_hip_set_hit *out, lm_hip_set_hit *pre_out, unsigned long long pre)
{
    const char *job_m = static_cast<const char *>(seg.d_job_m);
    const unsigned long long stride = seg.job_m_stride;
    if (seg.n_records + 1 <= (unsigned long long)kSetLdsOffsets) {
        hipLaunchKernelGGL((seqset_cut<false, true>), dim3(grid), dim3(kBlock), 0, st, ordered, count_ptr, room, njobs, seg.d_offsets,
                           seg.n_records, job_m, stride, wave_counts, starts, out, pre_out, pre);
        hipLaunchKernelGGL((seqset_cut<true, true>), dim3(grid), dim3(kBlock), 0, st, ordered, count_ptr, room, njobs, seg.d_offsets,
                           seg.n_records, job_m, stride, wave_counts, starts, out, pre_out, pre);
    } else {
        hipLaunchKernelGGL((seqset_cut<false, false>), dim3(grid), dim3(kBlock), 0, st, ordered, count_ptr, room, njobs, seg.d_offsets,
                           seg.n_records, job_m, stride, wave_counts, starts, out, pre_out, pre);
        hipLaunchKernelGGL((seqset_cut<true, false>), dim3(grid), dim3(kBlock), 0, st, ordered, count_ptr, room, njobs, seg.d_offsets,
                           seg.n_records, job_m, stride, wave_counts, starts, out, pre_out, pre);
    }
    LM_HIP_TRY(hipGetLastError());
    return LM_HIP_OK;
}

}  // namespace lm

using namespace lm;

// ---- the resident sequence set (C ABI) ------------------------------------------------------------------------

// offsets[0] == 0, non-decreasing, offsets[n_records] == total; the concatenation must fit the hit list's key space
// (hits.hip: key = job << 40 | cell).  No device is touched.
static int check_offsets(const char *what, const void *data, size_t total, const uint64_t *offsets, size_t n_records, size_t cols)
{
    if (!offsets)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: null offsets", what);
    if (total && !data)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: null data with a total of %zu symbols", what, total);
    if (cols == 0)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: zero columns", what);
    if (offsets[0] != 0)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: offsets[0] is %llu, not 0", what, (unsigned long long)offsets[0]);
    for (size_t r = 0; r < n_records; ++r)
        if (offsets[r + 1] < offsets[r])
            return fail(LM_HIP_ERR_BAD_ARGS, "%s: offsets decrease at record %zu (%llu after %llu)", what, r,
                        (unsigned long long)offsets[r + 1], (unsigned long long)offsets[r]);
    if (offsets[n_records] != total)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: offsets end at %llu, the data holds %zu symbols", what,
                    (unsigned long long)offsets[n_records], total);
    const unsigned long long rows = ((unsigned long long)total + cols - 1) / cols;
    if (rows > (1ull << 40) / cols)
        return fail(LM_HIP_ERR_CAPACITY, "%s: %zu symbols in %zu columns exceed the 2^40 cells a hit list can address", what, total,
                    cols);
    return LM_HIP_OK;
}

static int seqset_wrap(lm_hip_ctx *ctx, lm_hip_seq *seq, const uint64_t *offsets, size_t n_records, lm_hip_seqset **out)
{
    lm_hip_seqset *s = new (std::nothrow) lm_hip_seqset();
    if (!s) {
        lm_hip_seq_destroy(seq);
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    s->device = ctx->device;
    s->seq = seq;
    hipError_t e = hipSuccess;
    try {
        s->offsets.assign(offsets, offsets + n_records + 1);
    } catch (const std::bad_alloc &) {
        lm_hip_seqset_destroy(s);
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard guard(ctx->device);
        e = hipMalloc(&s->d_offsets, (n_records + 1) * sizeof(unsigned long long));
        if (e == hipSuccess)
            e = hipMemcpyAsync(s->d_offsets, s->offsets.data(), (n_records + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice,
                               ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        lm_hip_seqset_destroy(s);
        return fail(e == hipErrorOutOfMemory ? LM_HIP_ERR_OOM : LM_HIP_ERR_HIP, "sequence set: offsets upload failed: %s",
                    hipGetErrorString(e));
    }
    *out = s;
    return LM_HIP_OK;
}

int lm::seqset_adopt(lm_hip_ctx *ctx, lm_hip_seq *seq, std::vector<uint64_t> &&offsets, unsigned long long *d_offsets,
                     lm_hip_seqset **out)
{
    lm_hip_seqset *s = new (std::nothrow) lm_hip_seqset();
    if (!s) {
        {
            DeviceGuard guard(ctx->device);
            (void)hipFree(d_offsets);
        }
        lm_hip_seq_destroy(seq);
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    s->device = ctx->device;
    s->seq = seq;
    s->offsets = std::move(offsets);
    s->d_offsets = d_offsets;
    *out = s;
    return LM_HIP_OK;
}

extern "C" {

int lm_hip_seqset_from_ascii(lm_hip_ctx *ctx, char alphabet, const uint8_t *text, size_t total, const uint64_t *offsets,
                             size_t n_records, size_t cols, int lossy, lm_hip_seqset **out, size_t *bad_record, size_t *bad_index)
{
    LM_TRY(check_offsets("seqset_from_ascii", text, total, offsets, n_records, cols));
    if (!ctx || !out)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_ascii: null argument");
    *out = nullptr;
    lm_hip_seq *seq = nullptr;
    size_t bad = 0;
    const int st = lm_hip_seq_from_ascii(ctx, alphabet, text, total, cols, lossy, &seq, &bad);
    if (st == LM_HIP_ERR_INVALID_SYMBOL) {  // the record that holds the byte: the last one starting at or before it
        const size_t r = (size_t)(std::upper_bound(offsets, offsets + n_records + 1, (uint64_t)bad) - offsets) - 1;
        if (bad_record)
            *bad_record = r;
        if (bad_index)
            *bad_index = bad - (size_t)offsets[r];
        return fail(LM_HIP_ERR_INVALID_SYMBOL, "invalid symbol at position %zu of record %zu", bad - (size_t)offsets[r], r);
    }
    LM_TRY(st);
    return seqset_wrap(ctx, seq, offsets, n_records, out);
}

int lm_hip_seqset_from_encoded(lm_hip_ctx *ctx, const uint8_t *encoded, size_t total, const uint64_t *offsets, size_t n_records,
                               size_t cols, size_t k, lm_hip_seqset **out)
{
    LM_TRY(check_offsets("seqset_from_encoded", encoded, total, offsets, n_records, cols));
    if (!ctx || !out)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_encoded: null argument");
    *out = nullptr;
    lm_hip_seq *seq = nullptr;
    LM_TRY(lm_hip_seq_from_encoded(ctx, encoded, total, cols, k, &seq));
    return seqset_wrap(ctx, seq, offsets, n_records, out);
}

int lm_hip_seqset_configure_wrap(lm_hip_ctx *ctx, lm_hip_seqset *set, size_t m)
{
    if (!ctx || !set)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_configure_wrap: null argument");
    return lm_hip_seq_configure_wrap(ctx, set->seq, m);
}

int lm_hip_seqset_info(const lm_hip_seqset *set, size_t *records, size_t *total_length, size_t *rows, size_t *wrap, size_t *cols,
                       size_t *k)
{
    if (!set)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_info: null sequence set");
    if (records) *records = set->offsets.size() - 1;
    if (total_length) *total_length = set->seq->length;
    if (rows) *rows = set->seq->rows;
    if (wrap) *wrap = set->seq->wrap;
    if (cols) *cols = set->seq->cols;
    if (k) *k = set->seq->k;
    return LM_HIP_OK;
}

int lm_hip_seqset_record_length(const lm_hip_seqset *set, size_t record, size_t *length)
{
    if (!set || !length)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_record_length: null argument");
    if (record + 1 >= set->offsets.size())
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_record_length: record %zu of %zu", record, set->offsets.size() - 1);
    *length = (size_t)(set->offsets[record + 1] - set->offsets[record]);
    return LM_HIP_OK;
}

int lm_hip_seqset_lengths(const lm_hip_seqset *set, size_t *lengths, size_t capacity)
{
    if (!set || !lengths)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_lengths: null argument");
    const size_t n = set->offsets.size() - 1;
    if (capacity < n)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_lengths: room for %zu of %zu records", capacity, n);
    for (size_t r = 0; r < n; ++r)
        lengths[r] = (size_t)(set->offsets[r + 1] - set->offsets[r]);
    return LM_HIP_OK;
}

int lm_hip_seqset_destroy(lm_hip_seqset *set)
{
    if (!set)
        return LM_HIP_OK;
    {
        DeviceGuard guard(set->device);
        if (set->d_offsets)
            (void)hipFree(set->d_offsets);
    }
    lm_hip_seq_destroy(set->seq);
    delete set;
    return LM_HIP_OK;
}

}  // extern "C"
