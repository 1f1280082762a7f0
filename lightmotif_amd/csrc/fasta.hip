// fasta.hip -- a resident sequence set straight from FASTA bytes: the container is parsed on the device.
//
// lightmotif-cli reads its sequences with a compiled FASTA reader and hands every record to encode_lossy
// (main.rs:532-546, seq.rs:122-129).  Here the host hands over the raw bytes of the file and never looks at a
// sequence line: the device finds the header lines and the line ends, drops them, derives the record offsets and feeds
// the residues that are left to the encode + stripe kernels of layout.hip (the XF_ASCII transform, strict or lossy).
//
// THE GRAMMAR, on bytes:
//   lines           end at '\n' (0x0A); the last line need not have one
//   header lines    a line whose FIRST byte is '>' starts a record; records are numbered in file order
//   sequence lines  every other line belongs to the record opened by the nearest header line before it; sequence
//                   lines in front of the first header line belong to no record and are dropped
//   whitespace      in sequence lines the bytes 0x09-0x0D and 0x20 are dropped wherever they stand
//   residues        every other byte of a sequence line, through exactly the table lm_hip_seq_from_ascii uses.  A '>'
//                   that is not first on its line is a residue (an invalid one: the default symbol when lossy, an
//                   error when strict)
//   degenerate      a record may be empty; empty input, or input without a header line, is a set of zero records
// For PLAIN FASTA -- ASCII only, lines ended by "\n" or "\r\n", whitespace in a sequence line only at its ends -- these
// are exactly the records of scan_cli.read_fasta.  Outside that class the two differ: whitespace INSIDE a sequence line
// is dropped here (a default symbol or an error there); a lone '\r' is no line end here (a text-mode reader makes it
// one); non-ASCII bytes are invalid residues here (a text-mode reader refuses or replaces them).
//
// THE PASSES.  Whether a byte is first on its line is local (the byte before it is '\n', or it is byte 0), so header
// starts are local too; what is not local is whether the bytes in front of the first line start of a piece of text lie in
// a header line or in a sequence line, and whether a header has been seen at all.  A piece of text is therefore summed
// up, for either entry state e (0: in a sequence line, 1: in a header line), as
//     out[e]  the kind of the line that is open at its end
//     nh      header lines started in it
//     u[e]    residues in front of its first header start (they count only if a record is open already)
//     v[e]    residues behind its first header start
// and two neighbouring summaries combine associatively.  With tiles of kFastaTile bytes (one workgroup, 64 bytes per
// thread):
//   fasta_summary     every thread walks its 64 bytes (16 per step), a block scan combines the 256 summaries: one summary per tile
//   fasta_tile_scan   one workgroup scans the tile summaries (1 GB = 65 536 of them) with 64-bit counts: per tile the
//                     entry state, the residues kept before it and the records started before it; the two totals are
//                     the ONE 16-byte read-back the host needs before it can allocate
//   fasta_apply       walks every tile again with those three: residues go, compacted through LDS and in 16-byte
//                     stores, to a device-linear buffer; every header start writes offsets[r] and its own position
// No atomic decides an order, so a call repeats byte for byte.  The host finishes a header span's end with memchr over
// that header line alone.  Every position, count and tile index is 64-bit.
//
// UPLOAD.  The text goes up from the caller's (pageable) buffer in 32 MB pieces on the context's copy stream, as
// handles.hip: ingest_tiled sends its tiles; the fasta_summary launch of a piece waits for that piece's event, so summaries
// overlap the copies.  That is ALL that overlaps: the tile scan, the round trip, fasta_apply and the stripe kernel need
// the whole text and run behind the last copy -- unlike lm_hip_seq_from_ascii, whose kernels all hide behind the transfer.
//
// MEMORY.  The raw text (nbytes), the compact text (<= nbytes) and the striped matrix (~ the residues) are all device
// allocations: the peak stays below 3 x nbytes.  The raw text is released before the matrix is allocated, the compact
// text before the call returns.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "score_kernels.hpp"

namespace lm {

constexpr int kFastaLane = 64;                   // bytes one thread walks: four 16-byte loads
constexpr int kFastaTile = kBlock * kFastaLane;  // bytes one workgroup parses
constexpr size_t kFastaUpload = 32u << 20;       // bytes per upload command, as the tiles of handles.hip: ingest_tiled
static_assert(kFastaUpload % kFastaTile == 0, "an upload ends on a tile border");

template <typename N>
struct FastaSummary {
    unsigned out;  // bit e: the line open at the end is a header line, entered in state e
    N nh, u0, u1, v0, v1;
};

template <typename N>
__device__ __forceinline__ FastaSummary<N> fasta_identity()
{
    return FastaSummary<N>{2u, 0, 0, 0, 0, 0};
}

template <typename N, typename M>
__device__ __forceinline__ FastaSummary<N> fasta_combine(const FastaSummary<N> &l, const FastaSummary<M> &r)
{
    const unsigned m0 = l.out & 1u, m1 = (l.out >> 1) & 1u;  // the state `r` is entered in
    FastaSummary<N> s;
    s.out = ((r.out >> m0) & 1u) | (((r.out >> m1) & 1u) << 1);
    s.nh = l.nh + (N)r.nh;
    const N ru0 = m0 ? r.u1 : r.u0, rv0 = m0 ? r.v1 : r.v0;
    const N ru1 = m1 ? r.u1 : r.u0, rv1 = m1 ? r.v1 : r.v0;
    if (l.nh) {
        s.u0 = l.u0, s.v0 = l.v0 + ru0 + rv0;
        s.u1 = l.u1, s.v1 = l.v1 + ru1 + rv1;
    } else {
        s.u0 = l.u0 + ru0, s.v0 = rv0;
        s.u1 = l.u1 + ru1, s.v1 = rv1;
    }
    return s;
}

// Exclusive scan of one summary per thread (Hillis-Steele in LDS); *total = all kBlock of them combined.
template <typename N>
__device__ __forceinline__ FastaSummary<N> fasta_block_scan(const FastaSummary<N> &mine, FastaSummary<N> (*buf)[kBlock],
                                                            FastaSummary<N> *total)
{
    const unsigned tid = threadIdx.x;
    int cur = 0;
    buf[0][tid] = mine;
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)kBlock; d <<= 1) {
        FastaSummary<N> x = buf[cur][tid];
        if (tid >= d)
            x = fasta_combine(buf[cur][tid - d], x);
        buf[cur ^ 1][tid] = x;
        __syncthreads();
        cur ^= 1;
    }
    *total = buf[cur][kBlock - 1];
    const FastaSummary<N> ex = tid ? buf[cur][tid - 1] : fasta_identity<N>();
    __syncthreads();  // the caller may scan again
    return ex;
}

__device__ __forceinline__ bool fasta_space(const unsigned c) { return c - 9u <= 4u || c == 0x20u; }

// The 64 bytes of one thread, the byte in front of them, and how many of them exist.  The text's allocation is padded to
// whole tiles; what lies past `nbytes` reads as '\n', which adds neither a residue nor a header.
struct FastaLane {
    const uint4 *p;  // 16-byte aligned: tiles and lanes are multiples of 64 bytes
    unsigned prev;
    int live;
};

__device__ __forceinline__ FastaLane fasta_load(const uint8_t *__restrict__ text, const unsigned long long nbytes,
                                                const unsigned long long base)
{
    static_assert(kFastaLane % 16 == 0, "a lane is whole 16-byte loads");
    FastaLane ln;
    ln.p = reinterpret_cast<const uint4 *>(text + base);
    ln.prev = (base == 0 || base - 1 >= nbytes) ? (unsigned)'\n' : (unsigned)text[base - 1];
    ln.live = base >= nbytes ? 0 : (int)min((unsigned long long)kFastaLane, nbytes - base);
    return ln;
}

// f(j, byte, first on its line) for the 64 bytes in order
template <class F>
__device__ __forceinline__ void fasta_walk_word(const unsigned word, const int j0, const int live, unsigned &prev, F &f)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned c = j0 + q < live ? (word >> (8 * q)) & 0xffu : (unsigned)'\n';
        f(j0 + q, c, prev == (unsigned)'\n');
        prev = c;
    }
}

// One 16-byte load per step of a loop that is NOT unrolled: the whole walk unrolled keeps all 64 extracted bytes live and
// takes the kernels to the register ceiling (256 VGPRs, one wavefront per SIMD); this way they need ~45 and the loads of
// the other wavefronts hide the latency.  fasta_apply walks twice; its second pass reads what the first left in the cache.
template <class F>
__device__ __forceinline__ void fasta_walk(const FastaLane &ln, F f)
{
    unsigned prev = ln.prev;
#pragma unroll 1
    for (int q = 0; q < kFastaLane / 16; ++q) {
        const uint4 v = ln.p[q];
        const int j0 = 16 * q;
        fasta_walk_word(v.x, j0, ln.live, prev, f), fasta_walk_word(v.y, j0 + 4, ln.live, prev, f);
        fasta_walk_word(v.z, j0 + 8, ln.live, prev, f), fasta_walk_word(v.w, j0 + 12, ln.live, prev, f);
    }
}

__device__ __forceinline__ FastaSummary<unsigned> fasta_lane_summary(const FastaLane &ln)
{
    // before the first line start the kind of the line is the entry state's; behind it everything is known
    bool resolved = false, in_header = false;
    unsigned pre = 0, ub = 0, v = 0, nh = 0;
    fasta_walk(ln, [&](int, const unsigned c, const bool line_start) {
        if (line_start) {
            resolved = true;
            in_header = c == (unsigned)'>';
            nh += in_header ? 1u : 0u;
        }
        const unsigned residue = fasta_space(c) ? 0u : 1u;
        const unsigned kept = resolved && !in_header ? residue : 0u;
        pre += resolved ? 0u : residue;
        v += nh ? kept : 0u;  // (sums, not branches: a choice between two counters would keep them in memory)
        ub += nh ? 0u : kept;
    });
    FastaSummary<unsigned> s;
    s.out = resolved ? (in_header ? 3u : 0u) : 2u;
    s.nh = nh;
    s.u0 = pre + ub, s.u1 = ub;
    s.v0 = v, s.v1 = v;
    return s;
}

__global__ __launch_bounds__(kBlock) void fasta_summary(const uint8_t *__restrict__ text, const unsigned long long nbytes,
                                                        const unsigned long long tile0,
                                                        FastaSummary<unsigned> *__restrict__ sums)
{
    __shared__ FastaSummary<unsigned> s_scan[2][kBlock];
    const unsigned long long tile = tile0 + blockIdx.x;
    const FastaLane ln = fasta_load(text, nbytes, tile * kFastaTile + (unsigned long long)threadIdx.x * kFastaLane);
    FastaSummary<unsigned> total;
    (void)fasta_block_scan(fasta_lane_summary(ln), s_scan, &total);
    if (threadIdx.x == 0)
        sums[tile] = total;
}

struct FastaEntry {
    unsigned long long kept_before, records_before;
    unsigned state, pad;
};

// One workgroup, kBlock tiles per step, the running summary carried from step to step.  Evaluated at entry state 0 (byte 0
// is a line start), v0 of everything in front of a tile is what has been kept: u0 there is text before the first header.
__global__ __launch_bounds__(kBlock) void fasta_tile_scan(const FastaSummary<unsigned> *__restrict__ sums,
                                                          const unsigned long long ntiles, FastaEntry *__restrict__ entries,
                                                          unsigned long long *__restrict__ totals)
{
    __shared__ FastaSummary<unsigned long long> s_scan[2][kBlock];
    FastaSummary<unsigned long long> carry = fasta_identity<unsigned long long>();
    for (unsigned long long base = 0; base < ntiles; base += kBlock) {
        const unsigned long long t = base + threadIdx.x;
        FastaSummary<unsigned long long> mine = fasta_identity<unsigned long long>();
        if (t < ntiles)
            mine = fasta_combine(mine, sums[t]);
        FastaSummary<unsigned long long> total;
        const FastaSummary<unsigned long long> ex = fasta_block_scan(mine, s_scan, &total);
        const FastaSummary<unsigned long long> before = fasta_combine(carry, ex);
        if (t < ntiles)
            entries[t] = FastaEntry{before.v0, before.nh, before.out & 1u, 0u};
        carry = fasta_combine(carry, total);
    }
    if (threadIdx.x == 0) {
        totals[0] = carry.v0;
        totals[1] = carry.nh;
    }
}

__global__ __launch_bounds__(kBlock) void fasta_apply(const uint8_t *__restrict__ text, const unsigned long long nbytes,
                                                      const FastaEntry *__restrict__ entries, const unsigned long long total,
                                                      const unsigned long long n_records, uint8_t *__restrict__ compact,
                                                      unsigned long long *__restrict__ offsets,
                                                      unsigned long long *__restrict__ header_begin)
{
    __shared__ FastaSummary<unsigned> s_scan[2][kBlock];
    __shared__ uint4 s_out[kFastaTile / 16 + 2];  // the tile's residues, shifted so that LDS and global 16-byte chunks coincide
    const unsigned long long tile = blockIdx.x;
    const FastaEntry en = entries[tile];
    const unsigned long long base = tile * kFastaTile + (unsigned long long)threadIdx.x * kFastaLane;
    const FastaLane ln = fasta_load(text, nbytes, base);
    FastaSummary<unsigned> all;
    const FastaSummary<unsigned> ex = fasta_block_scan(fasta_lane_summary(ln), s_scan, &all);

    const bool open = en.records_before != 0;  // a record is open when the tile begins
    const unsigned e = en.state;
    const unsigned shift = (unsigned)(en.kept_before & 15ull);
    bool in_header = ((ex.out >> e) & 1u) != 0;
    unsigned long long record = en.records_before + ex.nh;  // the next header start is this record
    unsigned pos = (open ? (e ? ex.u1 : ex.u0) : 0u) + (e ? ex.v1 : ex.v0);
    unsigned kept = (open ? (e ? all.u1 : all.u0) : 0u) + (e ? all.v1 : all.v0);
    kept = (unsigned)min((unsigned long long)kept, total - min(total, en.kept_before));  // (never past the buffer)
    uint8_t *ob = reinterpret_cast<uint8_t *>(s_out);
    fasta_walk(ln, [&](const int j, const unsigned c, const bool line_start) {
        if (line_start) {
            in_header = c == (unsigned)'>';
            if (in_header) {
                if (record < n_records) {
                    offsets[record] = en.kept_before + pos;
                    header_begin[record] = base + (unsigned long long)j + 1ull;
                }
                ++record;
            }
        }
        if (!in_header && record != 0 && !fasta_space(c)) {
            if (pos < kept)
                ob[shift + pos] = (uint8_t)c;
            ++pos;
        }
    });
    if (tile == 0 && threadIdx.x == 0)
        offsets[n_records] = total;
    __syncthreads();

    const unsigned end = shift + kept;
    uint8_t *dst = compact + (en.kept_before - shift);  // 16-byte aligned
    for (unsigned k = threadIdx.x; k * 16u < end; k += kBlock) {
        const unsigned lo = k * 16u, hi = lo + 16u;
        if (lo >= shift && hi <= end) {
            reinterpret_cast<uint4 *>(dst)[k] = s_out[k];
        } else {  // the chunks this tile shares with its neighbours: only its own bytes
            for (unsigned b = max(lo, shift); b < min(hi, end); ++b)
                dst[b] = ob[b];
        }
    }
}

namespace {

// Releases what the call allocated on every way out; the streams are drained first (hipFree would wait as well).
struct FastaBuffers {
    lm_hip_ctx *ctx;
    uint8_t *d_text = nullptr, *d_compact = nullptr;
    char *d_meta = nullptr;
    unsigned long long *d_offsets = nullptr, *d_header_begin = nullptr;
    lm_hip_seq *seq = nullptr;
    explicit FastaBuffers(lm_hip_ctx *c) : ctx(c) {}
    void drop(void *p)
    {
        if (p)
            (void)hipFree(p);
    }
    ~FastaBuffers()
    {
        if (ctx->copy_stream)
            (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        drop(d_text), drop(d_compact), drop(d_meta), drop(d_offsets), drop(d_header_begin);
        if (seq)
            lm_hip_seq_destroy(seq);
    }
};

int fasta_ingest(lm_hip_ctx *ctx, const bool protein, const uint8_t *text, const size_t nbytes, const size_t cols, const bool lossy,
                 lm_hip_seqset **out, lm_hip_fasta_span **headers, size_t *n_records, size_t *bad_record, size_t *bad_index)
{
    FastaBuffers b(ctx);
    const unsigned long long ntiles = ((unsigned long long)nbytes + kFastaTile - 1) / kFastaTile;
    if (ntiles > 0x7fffffffull)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_from_fasta: %zu bytes are more tiles than one launch takes", nbytes);
    struct Totals { unsigned long long kept, records; } totals{0, 0};
    // d_meta: totals (16) | first bad position (8) | ... | tile summaries | tile entries
    const size_t sums_off = 64, entries_off = sums_off + (size_t)ntiles * sizeof(FastaSummary<unsigned>);
    LM_HIP_TRY(hipMalloc(&b.d_meta, entries_off + (size_t)ntiles * sizeof(FastaEntry)));
    unsigned long long *d_totals = reinterpret_cast<unsigned long long *>(b.d_meta);
    unsigned long long *d_bad = d_totals + 2;
    FastaSummary<unsigned> *d_sums = reinterpret_cast<FastaSummary<unsigned> *>(b.d_meta + sums_off);
    FastaEntry *d_entries = reinterpret_cast<FastaEntry *>(b.d_meta + entries_off);
    LM_HIP_TRY(hipMemsetAsync(d_bad, 0xff, 8, ctx->stream));
    if (ntiles) {
        LM_TRY(ingest_streams(ctx));
        LM_HIP_TRY(hipMalloc(&b.d_text, (size_t)ntiles * kFastaTile));
        // upload and summary kernels overlap: the kernels of one piece run while the next is copied
        for (size_t off = 0, i = 0; off < nbytes; off += kFastaUpload, ++i) {
            const size_t n = std::min(kFastaUpload, nbytes - off);
            hipEvent_t copied = ctx->tile_copied[i & 1];
            LM_HIP_TRY(hipMemcpyAsync(b.d_text + off, text + off, n, hipMemcpyHostToDevice, ctx->copy_stream));
            LM_HIP_TRY(hipEventRecord(copied, ctx->copy_stream));
            LM_HIP_TRY(hipStreamWaitEvent(ctx->stream, copied, 0));
            const unsigned long long tile0 = off / kFastaTile, tiles = (n + kFastaTile - 1) / kFastaTile;
            hipLaunchKernelGGL(fasta_summary, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, b.d_text,
                               (unsigned long long)nbytes, tile0, d_sums);
            LM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(fasta_tile_scan, dim3(1), dim3(kBlock), 0, ctx->stream, d_sums, ntiles, d_entries, d_totals);
        LM_HIP_TRY(hipGetLastError());
        LM_TRY(read_back(ctx, ctx->stream, d_totals, &totals));  // the one round trip: sizes of everything below
    }
    const size_t total = (size_t)totals.kept, n = (size_t)totals.records;
    const unsigned long long rows = ((unsigned long long)total + cols - 1) / cols;
    if (rows > (1ull << 40) / cols)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_from_fasta: %zu residues in %zu columns exceed the 2^40 cells a hit list can address",
                    total, cols);

    LM_HIP_TRY(hipMalloc(&b.d_offsets, (n + 1) * sizeof(unsigned long long)));
    std::vector<uint64_t> offsets, begins;
    try {
        offsets.assign(n + 1, 0);
        begins.assign(n, 0);
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    if (ntiles) {
        LM_HIP_TRY(hipMalloc(&b.d_compact, total + 16));
        LM_HIP_TRY(hipMalloc(&b.d_header_begin, (n + 1) * sizeof(unsigned long long)));
        hipLaunchKernelGGL(fasta_apply, dim3((unsigned)ntiles), dim3(kBlock), 0, ctx->stream, b.d_text, (unsigned long long)nbytes,
                           d_entries, totals.kept, totals.records, b.d_compact, b.d_offsets, b.d_header_begin);
        LM_HIP_TRY(hipGetLastError());
        LM_HIP_TRY(hipMemcpyAsync(offsets.data(), b.d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (n)
            LM_HIP_TRY(hipMemcpyAsync(begins.data(), b.d_header_begin, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        b.drop(b.d_text);  // parsed: the matrix takes its place
        b.d_text = nullptr;
    } else {
        LM_HIP_TRY(hipMemsetAsync(b.d_offsets, 0, sizeof(unsigned long long), ctx->stream));
    }

    // Encode + Stripe of the compact text, as lm_hip_seq_from_ascii runs them (pli/mod.rs:56-66, 178-200)
    const size_t k = protein ? 21 : 5, stride = lm_hip_stride(cols, 1);
    LM_TRY(seq_alloc(ctx, (size_t)rows, stride, cols, total, k, &b.seq));
    if (rows) {
        StripeTile t;
        t.d_src = b.d_compact;
        t.pitch = (size_t)rows;
        t.len = total;
        t.rows = (size_t)rows;
        t.rbase = 0;
        t.nrows = (size_t)rows;
        t.cols = cols;
        t.stride = stride;
        t.def = (uint8_t)(k - 1);
        t.d_data = b.seq->d_data;
        t.transform = StripeTile::Ascii;
        t.k = k;
        t.protein = protein;
        t.lossy = lossy;
        t.d_first_bad = d_bad;
        LM_TRY(launch_stripe_tile(ctx, t));
    }
    unsigned long long bad = ~0ull;
    LM_TRY(read_back(ctx, ctx->stream, d_bad, &bad));
    if (bad != ~0ull) {  // the record that holds the residue: the last one starting at or before it
        const size_t r = (size_t)(std::upper_bound(offsets.begin(), offsets.end(), (uint64_t)bad) - offsets.begin()) - 1;
        if (bad_record)
            *bad_record = r;
        if (bad_index)
            *bad_index = (size_t)(bad - offsets[r]);
        return fail(LM_HIP_ERR_INVALID_SYMBOL, "invalid symbol at position %zu of record %zu", (size_t)(bad - offsets[r]), r);
    }

    lm_hip_fasta_span *spans = nullptr;
    if (headers && n) {
        spans = static_cast<lm_hip_fasta_span *>(result_alloc(n * sizeof(lm_hip_fasta_span)));
        if (!spans)
            return fail(LM_HIP_ERR_OOM, "out of host memory");
        for (size_t r = 0; r < n; ++r) {  // the header line alone: up to its '\n', or to the end of the input
            const size_t begin = (size_t)begins[r];
            const void *nl = begin < nbytes ? memchr(text + begin, '\n', nbytes - begin) : nullptr;
            spans[r].begin = begin;
            spans[r].end = nl ? (uint64_t)(static_cast<const uint8_t *>(nl) - text) : (uint64_t)nbytes;
        }
    }
    lm_hip_seq *seq = b.seq;
    unsigned long long *d_offsets = b.d_offsets;
    b.seq = nullptr, b.d_offsets = nullptr;  // the set owns them from here on
    const int st = seqset_adopt(ctx, seq, std::move(offsets), d_offsets, out);
    if (st != LM_HIP_OK) {
        result_free(spans);
        return st;
    }
    if (headers)
        *headers = spans;
    *n_records = n;
    return LM_HIP_OK;
}

}  // namespace

}  // namespace lm

using namespace lm;

extern "C" {

size_t lm_hip_fasta_tile_bytes(void) { return (size_t)kFastaTile; }

int lm_hip_seqset_from_fasta(lm_hip_ctx *ctx, char alphabet, const uint8_t *text, size_t nbytes, size_t cols, int lossy,
                             lm_hip_seqset **out, lm_hip_fasta_span **headers, size_t *n_records, size_t *bad_record,
                             size_t *bad_index)
{
    if (!ctx || !out || !n_records)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_fasta: null argument");
    *out = nullptr;
    *n_records = 0;
    if (headers)
        *headers = nullptr;
    if (nbytes && !text)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_fasta: null text with %zu bytes", nbytes);
    if (cols == 0)
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_fasta: zero columns");
    if (alphabet != 'D' && alphabet != 'P')
        return fail(LM_HIP_ERR_BAD_ARGS, "seqset_from_fasta: alphabet must be 'D' or 'P'");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    return fasta_ingest(ctx, alphabet == 'P', text, nbytes, cols, lossy != 0, out, headers, n_records, bad_record, bad_index);
}

}  // extern "C"
