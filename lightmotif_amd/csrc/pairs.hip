// pairs.hip -- adjacent-pair counts of a resident sequence set: pairs[a * k + b] is the number of positions p of the
// concatenation with p and p + 1 in the same record, sym(p) = a and sym(p + 1) = b.  What a first-order chain is fitted
// from (sample.hip draws from one).
//
// Position p sits at row p % rows, column p / rows (pli/mod.rs:178-200): its successor is the cell below, or row 0 of the
// next column from the last row.
//
//   pair_blocks     every adjacent pair of the CONCATENATION, record borders included: a workgroup takes a band of rows,
//                   lane = column so that a wavefront's loads are consecutive bytes, counts into an LDS table of k * k
//                   u32 and flushes each non-zero counter with one 64-bit atomic (as sites.hip).  A byte >= k counts
//                   nowhere, as in count_symbols.
//   pair_borders    one lane per record: where the record's offset is the FIRST of its value (runs of empty records share
//                   one border) and lies strictly inside the text, the pair that straddles it is taken off again.
//
// All arithmetic is integer and modular in 64 bits: the result is the same from call to call, whatever order the atomics
// land in.
#include <cstring>

#include "lm_internal.hpp"

namespace lm {

namespace {

constexpr unsigned kPairBlock = 256;
constexpr unsigned kPairBandCells = 1u << 16;    // cells of one workgroup's band of rows (at least one row)
constexpr unsigned kPairMaxK = 21;

struct PairGeom {
    const uint8_t *data;
    unsigned long long stride, rows, length;
    unsigned cols, k, band_rows;
};

__device__ __forceinline__ unsigned long long pair_div(unsigned long long a, unsigned long long b)
{
    return ((a | b) >> 32) ? a / b : (unsigned long long)((unsigned)a / (unsigned)b);
}

__global__ __launch_bounds__(kPairBlock) void pair_blocks(const PairGeom g, unsigned long long *__restrict__ table)
{
    __shared__ unsigned s_table[kPairMaxK * kPairMaxK];
    const unsigned kk = g.k * g.k;
    for (unsigned i = threadIdx.x; i < kk; i += kPairBlock)
        s_table[i] = 0;
    __syncthreads();
    const unsigned long long r0 = (unsigned long long)blockIdx.x * g.band_rows;
    const unsigned nrows = (unsigned)min((unsigned long long)g.band_rows, g.rows - r0);
    const unsigned ncells = nrows * g.cols;  // <= max(kPairBandCells, cols) < 2^32
    for (unsigned e = threadIdx.x; e < ncells; e += kPairBlock) {
        const unsigned dr = e / g.cols, col = e - dr * g.cols;
        const unsigned long long row = r0 + dr;
        const unsigned long long p = (unsigned long long)col * g.rows + row;
        if (p + 1 >= g.length)
            continue;
        const unsigned a = g.data[row * g.stride + col];
        // (p + 1 < length <= rows * cols: from the last row there is a next column)
        const unsigned b = row + 1 < g.rows ? g.data[(row + 1) * g.stride + col] : g.data[col + 1];
        if (a < g.k && b < g.k)
            atomicAdd(&s_table[a * g.k + b], 1u);
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < kk; i += kPairBlock)
        if (s_table[i])
            atomicAdd(&table[i], (unsigned long long)s_table[i]);
}

__global__ __launch_bounds__(kPairBlock) void pair_borders(const PairGeom g, const unsigned long long *__restrict__ offsets,
                                                           const unsigned long long records, unsigned long long *__restrict__ table)
{
    const unsigned long long r = (unsigned long long)blockIdx.x * kPairBlock + threadIdx.x + 1;  // record 0 has no border in front
    if (r >= records)
        return;
    const unsigned long long o = offsets[r];
    if (o == 0 || o >= g.length || offsets[r - 1] == o)
        return;
    const unsigned long long c0 = pair_div(o - 1, g.rows), c1 = pair_div(o, g.rows);
    const unsigned a = g.data[(o - 1 - c0 * g.rows) * g.stride + c0], b = g.data[(o - c1 * g.rows) * g.stride + c1];
    if (a < g.k && b < g.k)
        atomicAdd(&table[a * g.k + b], ~0ull);  // minus one
}

}  // namespace

static int launch_count_pairs(lm_hip_ctx *ctx, const lm_hip_seqset *set, uint64_t *counts)
{
    const lm_hip_seq *seq = set->seq;
    const size_t records = set->offsets.size() - 1, kk = seq->k * seq->k;
    PairGeom g;
    g.data = seq->d_data;
    g.stride = seq->stride;
    g.rows = seq->rows;
    g.length = seq->length;
    g.cols = (unsigned)seq->cols;
    g.k = (unsigned)seq->k;
    g.band_rows = seq->cols >= kPairBandCells ? 1u : (unsigned)(kPairBandCells / seq->cols);
    const unsigned long long bands = (seq->rows + g.band_rows - 1) / g.band_rows;
    if (bands >> 31 || (records + kPairBlock - 1) / kPairBlock >> 31)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_count_pairs: %zu rows and %zu records are beyond the grid", seq->rows, records);
    LM_TRY(ctx->scratch.reserve(kk * 8));
    unsigned long long *d_table = static_cast<unsigned long long *>(ctx->scratch.ptr);
    LM_HIP_TRY(hipMemsetAsync(d_table, 0, kk * 8, ctx->stream));
    hipLaunchKernelGGL(pair_blocks, dim3((unsigned)bands), dim3(kPairBlock), 0, ctx->stream, g, d_table);
    if (records > 1)
        hipLaunchKernelGGL(pair_borders, dim3((unsigned)((records - 1 + kPairBlock - 1) / kPairBlock)), dim3(kPairBlock), 0, ctx->stream, g,
                           set->d_offsets, (unsigned long long)records, d_table);
    LM_HIP_TRY(hipGetLastError());
    ctx->last_kernel = "pair_blocks";
    LM_HIP_TRY(hipMemcpyAsync(counts, d_table, kk * 8, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LM_HIP_OK;
}

}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_seqset_count_pairs(lm_hip_ctx *ctx, const lm_hip_seqset *set, uint64_t *counts, size_t capacity)
{
    if (!ctx || !set || !counts)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_count_pairs: null argument");
    const lm_hip_seq *seq = set->seq;
    if (seq->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_count_pairs: the set lives on device %d, the context on %d", seq->device, ctx->device);
    if (seq->k == 0 || seq->k > kPairMaxK)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_count_pairs: an alphabet of %zu symbols", seq->k);
    const size_t kk = seq->k * seq->k;
    if (capacity < kk)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_count_pairs: room for %zu of %zu counts", capacity, kk);
    if (seq->length > seq->rows * seq->cols || seq->cols >> 32)  // (an adopted matrix is taken as described)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_count_pairs: %zu rows x %zu columns do not store %zu symbols", seq->rows, seq->cols,
                    seq->length);
    memset(counts, 0, kk * sizeof(uint64_t));
    if (seq->length < 2)
        return LM_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    return launch_count_pairs(ctx, set, counts);
}

}  // extern "C"
