// sites.hip -- symbols read back OUT of a resident sequence set: the text of hit windows, the count matrix of a motif's
// sites, whole records.
//
// A site is (record, position) and names the window [position + shift, position + shift + width) of that record:
//   site_windows   the window's symbol bytes, i.e. FIMO's `matched_sequence` of a hit, and with one site per record
//                  StripedSequence's Index (seq.rs:433-442) for every position of the record;
//   site_counts    CountMatrix::from_sequences (pwm/mod.rs:209-237) over the windows of a motif's sites -- the table the
//                  Gibbs sampler builds from its start positions (sampler.rs:412-422) -- without the windows ever
//                  leaving the device.
// Symbol q of the concatenation sits at row q % rows, column q / rows (pli/mod.rs:178-200); both kernels read by (row,
// column) with row < rows, so the wrap rows are never looked at.  A window is valid when its record exists and it lies
// inside the record (sites_plan.hpp: window_start); an invalid site is not an error: its window reads 0xFF and it counts
// nowhere.
//
//   site_windows          splits the work by OUTPUT byte: unit o of a chunk belongs to the segment found by binary search
//                         in the chunk's prefix table (staged in LDS up to kLdsPrefix entries, read from global memory
//                         beyond, as seqset_best does with offsets), to site (o - prefix) / width and symbol (o - prefix) %
//                         width of it.  One window of 100 Mbp runs as wide as a million windows of 12.
//   site_counts<true>     a workgroup takes a contiguous slice of ONE motif's sites, counts (site, j) pairs into a private
//   ("site_counts_lds")   LDS table of width * k u32 counters (ds_add_u32), and adds the non-zero ones to the motif's u64
//                         table with one 64-bit integer atomic each: many sites of one motif meet in LDS, not in L2.
//   site_counts<false>    tables beyond kLdsCounters: every pair adds to global memory directly.
//   ("site_counts_direct")
// Integer adds commute: a call repeats byte for byte.  The host half (chunks, images, checks) is sites_plan.hpp.
#include <algorithm>
#include <cstring>

#include "lm_internal.hpp"
#include "sites_plan.hpp"

namespace lm {

namespace sites {

constexpr int kSiteBlock = 256;
constexpr int kWindowItems = 8;  // output bytes per lane of site_windows

struct SiteGeom {
    const uint8_t *data;
    unsigned long long stride, rows;
    const unsigned long long *offsets;  // records + 1
    unsigned long long records;
    unsigned k;
};

__device__ __forceinline__ unsigned long long div_u64(unsigned long long a, unsigned long long b)
{
    return ((a | b) >> 32) ? a / b : (unsigned long long)((unsigned)a / (unsigned)b);
}

// first symbol of the site's window in the concatenation; false: invalid
__device__ __forceinline__ bool site_start(const SiteGeom &g, const unsigned long long *__restrict__ site, long long shift,
                                           unsigned long long width, unsigned long long *q)
{
    const unsigned long long rec = site[0], pos = site[1];
    if (rec >= g.records)
        return false;
    const unsigned long long o0 = g.offsets[rec], len = g.offsets[rec + 1] - o0;
    unsigned long long start;
    if (!window_start(pos, shift, width, len, &start))
        return false;
    *q = o0 + start;
    return true;
}

__device__ __forceinline__ unsigned symbol_at(const SiteGeom &g, unsigned long long q)
{
    const unsigned long long col = div_u64(q, g.rows), row = q - col * g.rows;
    return g.data[row * g.stride + col];
}

// largest s in [0, nseg) with prefix[s] <= x (prefix[0] = 0 and x < prefix[nseg])
__device__ __forceinline__ unsigned find_segment(const unsigned long long *prefix, unsigned nseg, unsigned long long x)
{
    unsigned lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kSiteBlock) void site_windows(const SiteGeom g, const unsigned long long *__restrict__ image,
                                                           const unsigned nseg, const int prefix_in_lds,
                                                           const unsigned long long total, uint8_t *__restrict__ out,
                                                           uint8_t *__restrict__ valid)
{
    extern __shared__ unsigned long long s_prefix[];
    const unsigned long long *prefix = image;
    if (prefix_in_lds) {
        for (unsigned i = threadIdx.x; i <= nseg; i += kSiteBlock)
            s_prefix[i] = image[i];
        __syncthreads();
        prefix = s_prefix;
    }
    const unsigned long long *__restrict__ segs = image + nseg + 1;
    const unsigned long long *__restrict__ sites = segs + (unsigned long long)nseg * kSegWords;
    const unsigned long long base = (unsigned long long)blockIdx.x * (kSiteBlock * kWindowItems) + threadIdx.x;
#pragma unroll 2
    for (int it = 0; it < kWindowItems; ++it) {
        const unsigned long long o = base + (unsigned long long)it * kSiteBlock;
        if (o >= total)
            break;
        const unsigned s = find_segment(prefix, nseg, o);
        const unsigned long long *seg = segs + s * kSegWords;
        const unsigned long long local = o - prefix[s], width = seg[2];
        const unsigned long long idx = div_u64(local, width), j = local - idx * width;
        const unsigned long long site = seg[0] + idx;
        unsigned long long q;
        const bool ok = site_start(g, sites + 2 * site, (long long)seg[3], width, &q);
        out[o] = ok ? (uint8_t)symbol_at(g, q + j) : (uint8_t)0xFF;
        if (j == 0)
            valid[site] = ok ? 1 : 0;
    }
}

template <bool LDS>
__global__ __launch_bounds__(kSiteBlock) void site_counts(const SiteGeom g, const unsigned long long *__restrict__ image,
                                                          const unsigned nseg, unsigned long long *__restrict__ tables,
                                                          unsigned long long *__restrict__ used)
{
    extern __shared__ unsigned s_tab[];  // LDS: [j][symbol], then the valid sites; direct: the valid sites alone
    const unsigned s = find_segment(image, nseg, blockIdx.x);
    const unsigned long long *__restrict__ seg = image + nseg + 1 + s * kSegWords;
    const unsigned long long *__restrict__ sites = image + nseg + 1 + (unsigned long long)nseg * kSegWords;
    const unsigned long long width = seg[2];
    const long long shift = (long long)seg[3];
    const unsigned slice = (unsigned)seg[6];
    const unsigned long long first = (blockIdx.x - image[s]) * slice;
    const unsigned nsites = (unsigned)min((unsigned long long)slice, seg[1] - first);
    const unsigned k = g.k;
    const unsigned ncounters = LDS ? (unsigned)width * k : 0u;
    unsigned long long *__restrict__ table = tables + seg[4];
    for (unsigned i = threadIdx.x; i <= ncounters; i += kSiteBlock)
        s_tab[i] = 0;
    __syncthreads();

    const unsigned long long *__restrict__ mine = sites + 2 * (seg[0] + first);
    const unsigned long long items = (unsigned long long)nsites * width;
    for (unsigned long long e = threadIdx.x; e < items; e += kSiteBlock) {
        const unsigned long long idx = div_u64(e, width), j = e - idx * width;
        unsigned long long q;
        if (!site_start(g, mine + 2 * idx, shift, width, &q))
            continue;
        if (j == 0)
            atomicAdd(&s_tab[ncounters], 1u);
        const unsigned v = symbol_at(g, q + j);
        if (v < k) {
            if (LDS)
                atomicAdd(&s_tab[(unsigned)j * k + v], 1u);
            else
                atomicAdd(&table[j * k + v], 1ull);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < ncounters; i += kSiteBlock)
        if (s_tab[i])
            atomicAdd(&table[i], (unsigned long long)s_tab[i]);
    if (threadIdx.x == 0 && s_tab[ncounters])
        atomicAdd(&used[seg[5]], (unsigned long long)s_tab[ncounters]);
}

}  // namespace sites
using namespace sites;

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

static SiteGeom geom_of(const lm_hip_seqset *set)
{
    SiteGeom g;
    g.data = set->seq->d_data;
    g.stride = set->seq->stride;
    g.rows = set->seq->rows;
    g.offsets = set->d_offsets;
    g.records = set->offsets.size() - 1;
    g.k = (unsigned)set->seq->k;
    return g;
}

static int upload_image(lm_hip_ctx *ctx, const std::vector<unsigned long long> &image, void *d_image)
{
    LM_HIP_TRY(hipMemcpyAsync(d_image, image.data(), image.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    return LM_HIP_OK;
}

static int run_windows(lm_hip_ctx *ctx, const lm_hip_seqset *set, const Request &r, const Plan &p, uint8_t *symbols, uint8_t *valid)
{
    if (p.max_units / (kSiteBlock * kWindowItems) >> 31)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_windows: a window of %llu symbols is beyond the grid", p.max_units);
    const size_t image_bytes = align256(p.max_image_words() * 8), window_bytes = align256((size_t)p.max_units);
    LM_TRY(ctx->scratch.reserve(image_bytes + window_bytes + align256(p.max_sites)));
    char *block = static_cast<char *>(ctx->scratch.ptr);
    unsigned long long *d_image = reinterpret_cast<unsigned long long *>(block);
    uint8_t *d_out = reinterpret_cast<uint8_t *>(block + image_bytes), *d_valid = d_out + window_bytes;
    const SiteGeom g = geom_of(set);
    std::vector<unsigned long long> image;
    std::vector<Run> runs;
    for (const Chunk &c : p.chunks) {
        build_image(r, p, c, &image);
        LM_TRY(upload_image(ctx, image, d_image));
        const unsigned nseg = (unsigned)(c.seg1 - c.seg0);
        const int in_lds = nseg + 1 <= kLdsPrefix;
        const unsigned grid = (unsigned)((c.units + kSiteBlock * kWindowItems - 1) / (kSiteBlock * kWindowItems));
        hipLaunchKernelGGL(site_windows, dim3(grid), dim3(kSiteBlock), in_lds ? (nseg + 1) * 8 : 0, ctx->stream, g, d_image, nseg, in_lds,
                           c.units, d_out, d_valid);
        LM_HIP_TRY(hipGetLastError());
        ctx->last_kernel = "site_windows";
        window_runs(r, p, c, &runs);
        for (const Run &x : runs) {
            LM_HIP_TRY(hipMemcpyAsync(symbols + x.host_byte, d_out + x.dev_byte, x.bytes, hipMemcpyDeviceToHost, ctx->stream));
            if (valid)
                LM_HIP_TRY(hipMemcpyAsync(valid + x.host_site, d_valid + x.dev_site, x.sites, hipMemcpyDeviceToHost, ctx->stream));
        }
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the image is rebuilt in place for the next chunk)
    }
    return LM_HIP_OK;
}

static int run_counts(lm_hip_ctx *ctx, const lm_hip_seqset *set, const Request &r, const Plan &p, uint64_t *tables, uint64_t *used)
{
    if (p.max_units >> 31 || p.max_segs >> 31)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_count_sites: %llu workgroups in one chunk are beyond the grid", p.max_units);
    // scratch: used u64[nlive] | tables u64[live_entries] | image
    const size_t head_bytes = align256((p.nlive + p.live_entries) * 8);
    LM_TRY(ctx->scratch.reserve(head_bytes + align256(p.max_image_words() * 8)));
    char *block = static_cast<char *>(ctx->scratch.ptr);
    unsigned long long *d_used = reinterpret_cast<unsigned long long *>(block), *d_tables = d_used + p.nlive;
    unsigned long long *d_image = reinterpret_cast<unsigned long long *>(block + head_bytes);
    LM_HIP_TRY(hipMemsetAsync(block, 0, head_bytes, ctx->stream));
    const SiteGeom g = geom_of(set);
    std::vector<unsigned long long> image;
    for (const Chunk &c : p.chunks) {
        build_image(r, p, c, &image);
        LM_TRY(upload_image(ctx, image, d_image));
        const unsigned nseg = (unsigned)(c.seg1 - c.seg0);
        if (c.direct) {
            hipLaunchKernelGGL(site_counts<false>, dim3((unsigned)c.units), dim3(kSiteBlock), 16, ctx->stream, g, d_image, nseg, d_tables, d_used);
            ctx->last_kernel = "site_counts_direct";
        } else {
            hipLaunchKernelGGL(site_counts<true>, dim3((unsigned)c.units), dim3(kSiteBlock), (size_t)c.counters * 4, ctx->stream, g, d_image,
                               nseg, d_tables, d_used);
            ctx->last_kernel = "site_counts_lds";
        }
        LM_HIP_TRY(hipGetLastError());
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    std::vector<uint64_t> host(p.nlive + p.live_entries);
    LM_HIP_TRY(hipMemcpyAsync(host.data(), block, host.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t k = set->seq->k;
    for (size_t i = 0; i < r.n; ++i)
        if (p.live[i] != kDead) {
            memcpy(tables + p.out_base[i], host.data() + p.nlive + p.table[p.live[i]], r.widths[i] * k * 8);
            if (used)
                used[i] = host[p.live[i]];
        }
    return LM_HIP_OK;
}

static int sites_call(const char *what, bool windows, lm_hip_ctx *ctx, const lm_hip_seqset *set, const Request &r, void *out, void *extra)
{
    if (!ctx || !set)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: null argument", what);
    const size_t k = set->seq->k;
    Totals t;
    std::string msg;
    const int status = sites::check(r, k, windows, &t, &msg);
    if (status != LM_HIP_OK)
        return fail(status, "%s: %s", what, msg.c_str());
    if (set->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: the set lives on device %d, the context on %d", what, set->device, ctx->device);
    if (r.n == 0)
        return LM_HIP_OK;
    // what no kernel writes: the windows of dead motifs read 0xFF and are invalid; tables start from zero
    Plan p;
    make_plan(r, k, windows, set->seq->rows ? set->seq->length : 0, ctx->site_chunk, kBlockBytes, &p);
    if (windows) {
        for (size_t i = 0; i < r.n; ++i)
            if (p.live[i] == kDead && r.counts[i]) {
                memset(static_cast<uint8_t *>(out) + p.out_base[i], 0xFF, r.counts[i] * r.widths[i]);
                if (extra)
                    memset(static_cast<uint8_t *>(extra) + p.site_base[i], 0, r.counts[i]);
            }
    } else {
        memset(out, 0, t.entries * sizeof(uint64_t));
        if (extra)
            memset(extra, 0, r.n * sizeof(uint64_t));
    }
    if (p.chunks.empty())
        return LM_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    return windows ? run_windows(ctx, set, r, p, static_cast<uint8_t *>(out), static_cast<uint8_t *>(extra))
                   : run_counts(ctx, set, r, p, static_cast<uint64_t *>(out), static_cast<uint64_t *>(extra));
}

}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_seqset_windows(lm_hip_ctx *ctx, const lm_hip_seqset *set, const size_t *counts, const size_t *widths, const int64_t *shifts,
                          size_t n, const void *sites, size_t site_stride_bytes, uint8_t *symbols, size_t capacity, uint8_t *valid)
{
    sites::Request r;
    r.counts = counts, r.widths = widths, r.shifts = shifts, r.n = n;
    r.sites = sites, r.stride = site_stride_bytes, r.out = symbols, r.capacity = capacity;
    return sites_call("seqset_windows", true, ctx, set, r, symbols, valid);
}

int lm_hip_seqset_count_sites(lm_hip_ctx *ctx, const lm_hip_seqset *set, const size_t *counts, const size_t *widths, const int64_t *shifts,
                              size_t n, const void *sites, size_t site_stride_bytes, uint64_t *tables, size_t capacity, uint64_t *used)
{
    sites::Request r;
    r.counts = counts, r.widths = widths, r.shifts = shifts, r.n = n;
    r.sites = sites, r.stride = site_stride_bytes, r.out = tables, r.capacity = capacity;
    return sites_call("seqset_count_sites", false, ctx, set, r, tables, used);
}

}  // extern "C"
