// regions.hip -- a sequence set cut out of a resident set, on the device: record i of the result is region i of the
// call, [start, end) of a source record clipped to it, as it stands or as its reverse complement (abc.rs:174-185).
//
// A genome is uploaded once as a set of contigs; every peak set, promoter set or variant neighbourhood is then a
// derived set and every set call takes it as it is.  The host half (regions_plan.hpp) settles everything that needs
// no device -- checks, clipping, the `taken` table, the offsets of the result -- and builds the image the kernel reads.
//
//   region_gather   DESTINATION-stationary over the joined text of the result.  A lane owns kRun = 16 consecutive
//                   destination bytes and issues one 16-byte store.  The workgroup finds the live regions its tile
//                   touches by two binary searches in global memory and stages that slab of destination offsets in
//                   LDS (up to kLdsSlab entries; a tile of single-symbol regions touches more, which are read from
//                   global memory); a lane finds the region of its first byte in the slab.  A source position q of the
//                   region sits at row q % rows, column q / rows of the source matrix (pli/mod.rs:178-200): the division
//                   is made once per run and once per region switch inside it, and from there the lane walks the rows --
//                   up for strand 0, down for strand 1, stepping to the neighbouring column at either end -- reading one
//                   byte per 32-byte row.  row < rows throughout: the wrap rows of the source are never read.
//
// The joined text then goes through launch_stripe_tile (StripeTile::None, pitch = rows) into a seq_alloc'd matrix and
// seqset_adopt takes over, as at the end of fasta.hip: fasta_ingest -- the padded cells and the layout are those of every
// other builder by construction.
//
// COST.  A source record is a column walk of the striped matrix, so a gathered byte costs a 32-byte sector of reads: fine
// for region sets that cover a few percent of the source, ~32 re-reads of it through L2 for a tiling of the whole source
// (tools/regions_bench.py measures both).
#include <new>
#include <string>
#include <vector>

#include "live_search.hpp"
#include "lm_internal.hpp"
#include "regions_plan.hpp"

namespace lm {

namespace regions {

__device__ __forceinline__ unsigned long long div_u64(unsigned long long a, unsigned long long b)
{
    return ((a | b) >> 32) ? a / b : (unsigned long long)((unsigned)a / (unsigned)b);
}

// Where a lane stands in the source matrix, and how it moves on to the next symbol of its region.
struct Cursor {
    const uint8_t *p;
    unsigned long long row;
    unsigned minus;
};

__global__ __launch_bounds__(kBlockLanes) void region_gather(const uint8_t *__restrict__ data, const unsigned long long stride,
                                                             const unsigned long long rows,
                                                             const unsigned long long *__restrict__ image,
                                                             const unsigned long long nlive, const unsigned long long total,
                                                             uint8_t *__restrict__ out)
{
    __shared__ unsigned long long s_dst[kLdsSlab];
    const unsigned long long *__restrict__ g_dst = image;
    const unsigned long long *__restrict__ live = image + nlive + 1;
    const unsigned long long b0 = (unsigned long long)blockIdx.x * kTile;  // < total: the grid is ceil(total / kTile)
    const unsigned long long b1 = min(total, b0 + kTile);
    auto global = [&](unsigned long long i) { return g_dst[i]; };
    const unsigned long long first = find_live(global, 0ull, nlive, b0);
    const unsigned long long last = find_live(global, first, nlive, b1 - 1);
    const unsigned staged = (unsigned)min(last - first + 2, (unsigned long long)kLdsSlab);  // dst[first .. last + 1]
    for (unsigned i = threadIdx.x; i < staged; i += kBlockLanes)
        s_dst[i] = g_dst[first + i];
    __syncthreads();
    auto dst = [&](unsigned long long i) {
        const unsigned long long j = i - first;
        return j < staged ? s_dst[(unsigned)j] : g_dst[i];
    };

    const unsigned long long d0 = b0 + (unsigned long long)threadIdx.x * kRun;
    if (d0 >= total)
        return;
    unsigned long long r = find_live(dst, first, last + 1, d0), next = 0;
    Cursor c{};
    // the symbol of region r that destination byte d holds: one division per call
    auto enter = [&](const unsigned long long d) {
        const unsigned long long base = dst(r);
        next = dst(r + 1);
        const unsigned long long local = d - base, src = live[r * kLiveWords];
        c.minus = (unsigned)live[r * kLiveWords + 1];
        const unsigned long long q = c.minus ? src + (next - base - 1 - local) : src + local;
        const unsigned long long col = div_u64(q, rows);
        c.row = q - col * rows;
        c.p = data + c.row * stride + col;
    };
    enter(d0);
    unsigned w[kRun / 4] = {0, 0, 0, 0};
#pragma unroll
    for (unsigned j = 0; j < kRun; ++j) {
        const unsigned long long d = d0 + j;
        if (d < total) {
            if (d == next) {  // (live regions hold at least one symbol: one step)
                ++r;
                enter(d);
            }
            unsigned b = *c.p;
            if (c.minus) {
                b = b < 4u ? b ^ 2u : b;  // abc.rs:174-185
                if (c.row == 0) {         // the symbol before row 0 of a column is the last row of the column before
                    c.row = rows - 1;
                    c.p += (rows - 1) * stride - 1;
                } else {
                    --c.row;
                    c.p -= stride;
                }
            } else {
                ++c.row;
                c.p += stride;
                if (c.row == rows) {
                    c.row = 0;
                    c.p -= rows * stride - 1;
                }
            }
            w[j / 4] |= b << (8 * (j % 4));
        }
    }
    // the text's allocation is padded to whole runs: the last run is stored whole as well
    *reinterpret_cast<uint4 *>(out + d0) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace regions
using namespace regions;

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

namespace {

// What the call made, released on every way out that does not hand it to the set.
struct Made {
    lm_hip_ctx *ctx;
    lm_hip_seq *seq = nullptr;
    unsigned long long *d_offsets = nullptr;
    explicit Made(lm_hip_ctx *c) : ctx(c) {}
    ~Made()
    {
        (void)hipStreamSynchronize(ctx->stream);
        if (d_offsets)
            (void)hipFree(d_offsets);
        if (seq)
            lm_hip_seq_destroy(seq);
    }
};

int gather(lm_hip_ctx *ctx, const lm_hip_seqset *src, Plan &p, size_t n, lm_hip_seqset **out)
{
    const lm_hip_seq *s = src->seq;
    if ((p.total + kTile - 1) / kTile >> 31)
        return fail(LM_HIP_ERR_CAPACITY, "seqset_from_regions: %llu symbols are beyond the grid", (unsigned long long)p.total);
    Made m(ctx);
    LM_HIP_TRY(hipMalloc(&m.d_offsets, (n + 1) * sizeof(unsigned long long)));
    LM_HIP_TRY(hipMemcpyAsync(m.d_offsets, p.offsets.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    LM_TRY(seq_alloc(ctx, (size_t)p.rows, s->stride, s->cols, (size_t)p.total, s->k, &m.seq));
    if (p.nlive) {
        // scratch: the image | the joined text, padded to whole runs
        const size_t image_bytes = align256(p.image.size() * 8), text_bytes = align256((size_t)p.total + kRun);
        LM_TRY(ctx->scratch.reserve(image_bytes + text_bytes));
        char *block = static_cast<char *>(ctx->scratch.ptr);
        unsigned long long *d_image = reinterpret_cast<unsigned long long *>(block);
        uint8_t *d_text = reinterpret_cast<uint8_t *>(block + image_bytes);
        LM_HIP_TRY(hipMemcpyAsync(d_image, p.image.data(), p.image.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = (unsigned)((p.total + kTile - 1) / kTile);
        hipLaunchKernelGGL(region_gather, dim3(grid), dim3(kBlockLanes), 0, ctx->stream, s->d_data, (unsigned long long)s->stride,
                           (unsigned long long)s->rows, d_image, (unsigned long long)p.nlive, (unsigned long long)p.total, d_text);
        LM_HIP_TRY(hipGetLastError());
        StripeTile t;
        t.d_src = d_text;
        t.pitch = (size_t)p.rows;
        t.len = (size_t)p.total;
        t.rows = (size_t)p.rows;
        t.rbase = 0;
        t.nrows = (size_t)p.rows;
        t.cols = s->cols;
        t.stride = s->stride;
        t.def = (uint8_t)(s->k - 1);
        t.d_data = m.seq->d_data;
        t.transform = StripeTile::None;
        t.k = s->k;
        LM_TRY(launch_stripe_tile(ctx, t));
        ctx->last_kernel = "region_gather";
    }
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    lm_hip_seq *seq = m.seq;
    unsigned long long *d_offsets = m.d_offsets;
    m.seq = nullptr, m.d_offsets = nullptr;  // the set owns them from here on
    return seqset_adopt(ctx, seq, std::move(p.offsets), d_offsets, out);
}

}  // namespace

}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_seqset_from_regions(lm_hip_ctx *ctx, const lm_hip_seqset *src, const lm_hip_region *regions, size_t n, lm_hip_seqset **out,
                               lm_hip_region_span *taken)
{
    if (out)
        *out = nullptr;
    regions::Args a;
    a.ctx = ctx != nullptr, a.src = src != nullptr, a.out = out != nullptr;
    a.ctx_device = ctx ? ctx->device : 0, a.src_device = src ? src->device : 0;
    a.k = src ? src->seq->k : 0;
    a.regions = regions, a.n = n;
    std::string msg;
    int status = regions::check(a, &msg);
    if (status != LM_HIP_OK)
        return fail(status, "seqset_from_regions: %s", msg.c_str());
    regions::Plan p;
    try {
        status = regions::make_plan(src->offsets.data(), src->offsets.size() - 1, src->seq->cols, regions, n, taken, &p, &msg);
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    if (status != LM_HIP_OK)
        return fail(status, "seqset_from_regions: %s", msg.c_str());
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    return gather(ctx, src, p, n, out);
}

}  // extern "C"
