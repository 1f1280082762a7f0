// composition.hip -- what a resident striped sequence is made of: SymbolCount::count_symbols (seq.rs:444-483) for one
// sequence and, in one call, for every record of a sequence set.
//
// The matrix is row-major bytes, `stride` per row; position p of the sequence sits at row p % rows, column p / rows
// (pli/mod.rs:178-200).  A column is therefore a contiguous run of POSITIONS and a strided run of MEMORY, and a record
// of a set is a run of positions that may start and end anywhere.  Counts come out as differences of prefix counts, in
// three passes and without a global atomic (one long record would send every workgroup's adds to the same k addresses):
//
//   count_blocks   a workgroup takes `T` rows x a chunk of columns -- for the usual matrix, whose chunk is every column,
//                  T * stride contiguous bytes read once, lane = column so that a wavefront's loads are consecutive bytes
//                  -- and counts each column's run into an LDS histogram (ds_add_u32; a byte >= k adds nothing).  It
//                  writes the k counts of every (column, tile) block as u32 into a table laid out symbol-major and, per
//                  symbol, in POSITION order: table[s * nb + c * ntiles + t], nb = cols * ntiles.
//   scan           launch_scan_u32 (reduce.hip) over the k * nb entries as one flat array: the exclusive prefix F.  Within
//                  symbol s, F[s * nb + b] - F[s * nb] is the count of s in front of block b; the subtrahend is the same
//                  at both ends of a record and is never formed.
//   count_prefix   per offset p (records + 1 of them; {0, length} for a single sequence): P_s(p) = F[s * nb + b(p)] + the
//                  count of s over the cells of block b(p) in front of p -- at most T cells, one column, `stride` bytes
//                  apart.  A wavefront per offset where offsets are sparse (64 bases per offset and more); a lane per
//                  offset where they are dense: lanes whose offsets fall into one block walk the same cells in step and
//                  share the loads.
//   count_diff     counts[r][s] = P_s(offsets[r + 1]) - P_s(offsets[r]).
//
// The padded tail needs no special case: it lies behind `length` in position order, and no offset looks past `length`.
// Wrap rows lie behind row `rows` and are never read (seq.rs:469-477).  Everything is integer arithmetic on 64-bit
// positions: the result is the same from call to call and for every tile height (option "count_tile_rows").
#include <algorithm>
#include <cstring>

#include "lm_internal.hpp"

namespace lm {

namespace {

constexpr int kCountBlock = 256;
constexpr int kCountUnroll = 16;               // byte loads a lane has in flight
constexpr unsigned kCountLdsCounters = 12288;  // 48 KB of u32: the columns of one workgroup x k
constexpr size_t kCountTileRows = 1024;        // default T: 4 k / T bytes of table per position (0.02 for DNA)
constexpr size_t kCountMaxTileRows = 65536;    // T * columns of a workgroup stays below 2^32
constexpr unsigned long long kCountMaxTiles = 1ull << 30;  // grid.x
constexpr size_t kCountSparseBases = 64;       // bases per offset from which a wavefront, not a lane, takes an offset

struct CountGeom {
    const uint8_t *data;
    unsigned long long stride, rows, ntiles, nb;
    unsigned cols, k, tile_rows;
};

__global__ __launch_bounds__(kCountBlock) void count_blocks(const CountGeom g, const unsigned chunk_cols,
                                                            unsigned *__restrict__ table)
{
    extern __shared__ unsigned s_hist[];  // [column of the chunk][symbol]
    const unsigned tid = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned c0 = blockIdx.y * chunk_cols, ccn = min(chunk_cols, g.cols - c0);
    const unsigned k = g.k, nhist = ccn * k;
    for (unsigned i = tid; i < nhist; i += kCountBlock)
        s_hist[i] = 0;
    __syncthreads();

    const unsigned long long r0 = t * g.tile_rows;
    const unsigned nrows = (unsigned)min((unsigned long long)g.tile_rows, g.rows - r0);
    const unsigned ncells = nrows * ccn;  // cells of the chunk in (row, column) order; lane e holds cell e, e + 256, ...
    const uint8_t *__restrict__ base = g.data + r0 * g.stride + c0;
    const unsigned drow = kCountBlock / ccn, dcol = kCountBlock % ccn;
    const unsigned long long dbytes = drow * g.stride + dcol, wrap_bytes = g.stride - ccn;
    unsigned col = tid % ccn;
    unsigned long long off = (tid / ccn) * g.stride + col;
    unsigned first = 0;  // of the step: the cell lane 0 holds (uniform)
    for (; first + kCountUnroll * kCountBlock <= ncells; first += kCountUnroll * kCountBlock) {
        unsigned v[kCountUnroll], slot[kCountUnroll];
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u) {
            v[u] = base[off];
            slot[u] = col * k;
            col += dcol;
            off += dbytes;
            if (col >= ccn) {
                col -= ccn;
                off += wrap_bytes;
            }
        }
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u)
            if (v[u] < k)
                atomicAdd(&s_hist[slot[u] + v[u]], 1u);
    }
    for (unsigned e = first + tid; e < ncells; e += kCountBlock) {
        const unsigned v = base[off];
        if (v < k)
            atomicAdd(&s_hist[col * k + v], 1u);
        col += dcol;
        off += dbytes;
        if (col >= ccn) {
            col -= ccn;
            off += wrap_bytes;
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < nhist; i += kCountBlock) {
        const unsigned c = i / k, s = i - c * k;
        table[s * g.nb + (c0 + c) * g.ntiles + t] = s_hist[i];
    }
}

// offsets == nullptr: the single sequence, offsets {0, length}.  G lanes share one offset: G = 1 where offsets are dense (the
// lanes of a wavefront then walk neighbouring blocks in step and their loads coincide), G = 64 where they are sparse (one
// lane alone would wait out a memory latency per cell of its block).
template <int G>
__global__ __launch_bounds__(kCountBlock) void count_prefix(const CountGeom g, const unsigned long long *__restrict__ offsets,
                                                            const unsigned long long n_offsets, const unsigned long long length,
                                                            const unsigned long long *__restrict__ scan_offsets,
                                                            const unsigned long long *__restrict__ scan_tiles,
                                                            unsigned long long *__restrict__ prefix)
{
    static_assert(G == 1 || G == 64, "a lane or a wavefront per offset");
    const unsigned long long i = ((unsigned long long)blockIdx.x * kCountBlock + threadIdx.x) / G;
    const unsigned sub = threadIdx.x % G;
    if (i >= n_offsets)  // (a whole wavefront at once when G = 64)
        return;
    unsigned long long p = offsets ? offsets[i] : (i ? length : 0ull);
    p = min(p, length);  // (a set's offsets end at its length: nothing looks past it)
    unsigned long long c = p / g.rows, r = p - c * g.rows;
    if (c >= g.cols) {  // p == rows * cols: everything, i.e. the whole of the last column
        c = g.cols - 1;
        r = g.rows;
    }
    const unsigned long long t = min(r / g.tile_rows, g.ntiles - 1);
    const unsigned long long b = c * g.ntiles + t;
    const unsigned n = (unsigned)(r - t * g.tile_rows);  // cells of the block in front of p: <= T
    const uint8_t *__restrict__ cell = g.data + t * g.tile_rows * g.stride + c;
    for (unsigned s0 = 0; s0 < g.k; s0 += 8) {  // eight symbols per walk: DNA in one, protein in three
        unsigned cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
        for (unsigned j = sub; j < n; j += G) {
            const unsigned v = (unsigned)cell[j * g.stride] - s0;
#pragma unroll
            for (unsigned q = 0; q < 8; ++q)
                cnt[q] += v == q ? 1u : 0u;
        }
        if (G > 1) {
#pragma unroll
            for (unsigned q = 0; q < 8; ++q)
                for (int m = G / 2; m > 0; m >>= 1)
                    cnt[q] += __shfl_xor(cnt[q], m);
        }
        if (sub == 0) {
#pragma unroll
            for (unsigned q = 0; q < 8; ++q)
                if (s0 + q < g.k) {
                    const unsigned long long e = (s0 + q) * g.nb + b;
                    prefix[i * g.k + s0 + q] = scan_tiles[e / kScanTile] + scan_offsets[e] + cnt[q];
                }
        }
    }
}

__global__ __launch_bounds__(kCountBlock) void count_diff(const unsigned long long *__restrict__ prefix, const unsigned long long n,
                                                          const unsigned k, unsigned long long *__restrict__ out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kCountBlock + threadIdx.x;
    if (i < n)
        out[i] = prefix[i + k] - prefix[i];
}

}  // namespace

// counts[r * k + s] for the `records` records cut by d_offsets (device, records + 1 entries; nullptr: one record, the whole
// sequence).  records > 0 and seq->length > 0.
static int launch_count_symbols(lm_hip_ctx *ctx, const lm_hip_seq *seq, const unsigned long long *d_offsets, size_t records,
                                uint64_t *counts)
{
    size_t T = ctx->count_tile_rows ? ctx->count_tile_rows : kCountTileRows;
    while (T < kCountMaxTileRows && (seq->rows + T - 1) / T > kCountMaxTiles)
        T *= 2;
    CountGeom g;
    g.data = seq->d_data;
    g.stride = seq->stride;
    g.rows = seq->rows;
    g.ntiles = (seq->rows + T - 1) / T;
    g.nb = g.ntiles * seq->cols;
    g.cols = (unsigned)seq->cols;
    g.k = (unsigned)seq->k;
    g.tile_rows = (unsigned)T;
    if (g.ntiles > kCountMaxTiles || seq->cols >> 32)
        return fail(LM_HIP_ERR_CAPACITY, "count_symbols: a matrix of %zu rows x %zu columns is beyond the counting grid", seq->rows,
                    seq->cols);
    const unsigned chunk_cols = (unsigned)std::min<size_t>(seq->cols, kCountLdsCounters / seq->k);
    const unsigned nchunks = (unsigned)((seq->cols + chunk_cols - 1) / chunk_cols);
    if (nchunks > 65535u)
        return fail(LM_HIP_ERR_CAPACITY, "count_symbols: %zu columns of %zu symbols are beyond the counting grid", seq->cols, seq->k);

    // scratch: table u32[n] | scanned u64[n] | scan tiles u64[] | total u64 | prefix u64[(records + 1) k] | counts u64[records k]
    const unsigned long long n = g.nb * g.k;
    const unsigned long long nscan = (n + kScanTile - 1) / kScanTile;
    if (nscan >> 31)
        return fail(LM_HIP_ERR_CAPACITY, "count_symbols: %llu blocks of %zu rows are beyond the scan's grid", g.nb, T);
    const size_t off_prefix = hits::scan_layout(n).bytes;
    const size_t off_out = off_prefix + (records + 1) * seq->k * 8;
    LM_TRY(ctx->scratch.reserve(off_out + records * seq->k * 8));
    char *block = static_cast<char *>(ctx->scratch.ptr);
    const ScanArrays scan = carve_scan_u32(block, n);
    unsigned *table = scan.counts;
    unsigned long long *scanned = scan.offsets, *tiles = scan.tiles;
    unsigned long long *prefix = reinterpret_cast<unsigned long long *>(block + off_prefix);
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(block + off_out);

    // option "time_scan": the three passes between events (lm_hip_ctx_last_phases_ms: [0] blocks, [1] scan, [2] prefix + diff)
    scan_timer_begin(ctx, ctx->stream);
    hipLaunchKernelGGL(count_blocks, dim3((unsigned)g.ntiles, nchunks), dim3(kCountBlock), (size_t)chunk_cols * seq->k * 4, ctx->stream,
                       g, chunk_cols, table);
    LM_HIP_TRY(hipGetLastError());
    ctx->last_kernel = "count_blocks";
    scan_timer_end(ctx, ctx->stream);
    LM_TRY(launch_scan_u32(ctx, scan, n));
    scan_timer_mark(ctx, ctx->stream, 2);
    const unsigned long long n_offsets = (unsigned long long)records + 1, cells = (unsigned long long)records * seq->k;
    if (seq->length / n_offsets >= kCountSparseBases)
        hipLaunchKernelGGL(count_prefix<64>, dim3((unsigned)((n_offsets * 64 + kCountBlock - 1) / kCountBlock)), dim3(kCountBlock), 0,
                           ctx->stream, g, d_offsets, n_offsets, (unsigned long long)seq->length, scanned, tiles, prefix);
    else
        hipLaunchKernelGGL(count_prefix<1>, dim3((unsigned)((n_offsets + kCountBlock - 1) / kCountBlock)), dim3(kCountBlock), 0,
                           ctx->stream, g, d_offsets, n_offsets, (unsigned long long)seq->length, scanned, tiles, prefix);
    hipLaunchKernelGGL(count_diff, dim3((unsigned)((cells + kCountBlock - 1) / kCountBlock)), dim3(kCountBlock), 0, ctx->stream, prefix,
                       cells, g.k, d_out);
    LM_HIP_TRY(hipGetLastError());
    scan_timer_mark(ctx, ctx->stream, 3);
    LM_HIP_TRY(hipMemcpyAsync(counts, d_out, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    scan_timer_read(ctx);
    return LM_HIP_OK;
}

static int count_symbols(const char *what, lm_hip_ctx *ctx, const lm_hip_seq *seq, const unsigned long long *d_offsets, size_t records,
                         uint64_t *counts, size_t capacity)
{
    if (seq->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: the sequence lives on device %d, the context on %d", what, seq->device, ctx->device);
    if (seq->k && records > ~(size_t)0 / 8 / seq->k)
        return fail(LM_HIP_ERR_CAPACITY, "%s: %zu records x %zu symbols overflow the table's size", what, records, seq->k);
    const size_t cells = records * seq->k;
    if (capacity < cells)
        return fail(LM_HIP_ERR_CAPACITY, "%s: room for %zu of %zu counts", what, capacity, cells);
    if (seq->length > seq->rows * seq->cols)  // (an adopted matrix is taken as described)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: %zu rows x %zu columns store fewer than %zu symbols", what, seq->rows, seq->cols,
                    seq->length);
    if (cells == 0)
        return LM_HIP_OK;
    if (seq->length == 0) {
        memset(counts, 0, cells * sizeof(uint64_t));
        return LM_HIP_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    return launch_count_symbols(ctx, seq, d_offsets, records, counts);
}

}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_seq_count_symbols(lm_hip_ctx *ctx, const lm_hip_seq *seq, uint64_t *counts, size_t capacity)
{
    if (!ctx || !seq || !counts)
        return fail(LM_HIP_ERR_BAD_ARGS, "seq_count_symbols: null argument");
    return count_symbols("seq_count_symbols", ctx, seq, nullptr, 1, counts, capacity);
}

int lm_hip_seqset_count_symbols(lm_hip_ctx *ctx, const lm_hip_seqset *set, uint64_t *counts, size_t capacity)
{
    if (!ctx || !set || !counts)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_count_symbols: null argument");
    return count_symbols("seqset_count_symbols", ctx, set->seq, set->d_offsets, set->offsets.size() - 1, counts, capacity);
}

}  // extern "C"
