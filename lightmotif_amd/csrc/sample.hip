// sample.hip -- a null sequence set drawn on the device: EncodedSequence::sample / StripedSequence::sample (seq.rs:131-143,
// seq.rs:315-328) for every record of a set in one call, i.i.d. from a Background (abc.rs:389-402) or from a first-order
// Markov chain.  The rule, the generator and everything that needs no device are in sample_plan.hpp.
//
// All kernels are DESTINATION-stationary over the joined text of the result, shaped like regions.hip: region_gather.  A
// lane owns kRun = 16 consecutive text bytes and issues one 16-byte store; the workgroup stages the slab of live-record
// offsets its tile touches in LDS and a lane finds the record of its first byte there (live_search.hpp).  One Philox block
// yields the uniforms of 4 positions of a record, so a lane computes 4 or 5 blocks per run (one more per record border).
//
//   sample_iid     order 0.  The thresholds of the shared model sit in LDS; per-record thresholds are a device table read
//                  when a run enters a record.
//   markov_tiles   order 1, first of three launches in stream order (no workgroup waits for another): the step of every
//                  position is a 15-bit map; a lane composes the maps of its run, the workgroup those of its tile.
//   markov_carry   one workgroup: the exclusive scan of the tile maps.  Position 0 is a record start, so every prefix is a
//                  constant map and the carry into a tile is one symbol.
//   markov_emit    the uniforms again; the per-position maps go to LDS, the run maps through a wave and LDS scan, the carry
//                  is applied, and each lane replays its 16 maps from its entering symbol.
//
// The text then goes through launch_stripe_tile (StripeTile::None, pitch = rows) into a seq_alloc'd matrix and seqset_adopt
// takes over, as at the end of regions.hip: gather.
#include <new>
#include <string>
#include <vector>

#define LM_SAMPLE_HD __host__ __device__
#include "live_search.hpp"
#include "lm_internal.hpp"
#include "sample_plan.hpp"

namespace lm {

namespace sample {

struct TextGeom {
    const unsigned long long *image;  // dst[nlive + 1] | record[nlive]
    unsigned long long nlive, total, seed, record_base;
};

// The records a workgroup's tile touches, staged: dst(i) for i in [first, last + 1].
struct Slab {
    const unsigned long long *g_dst;
    const unsigned long long *s_dst;
    unsigned long long first, last;
    unsigned staged;
    __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const
    {
        const unsigned long long j = i - first;
        return j < staged ? s_dst[(unsigned)j] : g_dst[i];
    }
};

// (every lane of the workgroup calls this: it synchronises)
__device__ __forceinline__ Slab stage_slab(const TextGeom &g, unsigned long long *s_dst)
{
    const unsigned long long b0 = (unsigned long long)blockIdx.x * kTile;  // < total: the grid is ceil(total / kTile)
    const unsigned long long b1 = min(g.total, b0 + kTile);
    const unsigned long long *g_dst = g.image;
    auto global = [&](unsigned long long i) { return g_dst[i]; };
    Slab s;
    s.g_dst = g_dst;
    s.s_dst = s_dst;
    s.first = find_live(global, 0ull, g.nlive, b0);
    s.last = find_live(global, s.first, g.nlive, b1 - 1);
    s.staged = (unsigned)min(s.last - s.first + 2, (unsigned long long)kLdsSlab);  // dst[first .. last + 1]
    for (unsigned i = threadIdx.x; i < s.staged; i += kBlockLanes)
        s_dst[i] = g_dst[s.first + i];
    __syncthreads();
    return s;
}

// The walk of one lane's run [d0, d0 + n) of the joined text: enter(live) when the run stands in a new live record, and
// at(i, first, u) for byte i of the run, `first` when it is position 0 of its record, u its uniform.  One Philox block per
// iteration: up to four positions of one record.
template <class Enter, class At>
__device__ __forceinline__ void walk_run(const TextGeom &g, const Slab &dst, const unsigned long long d0, const unsigned n, Enter enter,
                                         At at)
{
    const unsigned long long *__restrict__ record = g.image + g.nlive + 1;
    unsigned long long r = find_live(dst, dst.first, dst.last + 1, d0);
    unsigned long long next = dst(r + 1), j = d0 - dst(r), R = g.record_base + record[r];
    enter(r);
    unsigned i = 0;
    while (i < n) {
        if (d0 + i == next) {  // (live records hold at least one symbol: one step)
            ++r;
            next = dst(r + 1);
            j = 0;
            R = g.record_base + record[r];
            enter(r);
        }
        unsigned u[4];
        uniforms(g.seed, R, j >> 2, u);
        const unsigned w0 = (unsigned)j & 3u;
        const unsigned cnt = (unsigned)min((unsigned long long)min(4u - w0, n - i), next - (d0 + i));
#pragma unroll
        for (unsigned t = 0; t < 4; ++t)
            if (t >= w0 && t - w0 < cnt)
                at(i + t - w0, j == 0 && t == 0, u[t]);
        i += cnt;
        j += cnt;
    }
}

// byte i (< 16) of a run held in four words
struct RunBytes {
    unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    __device__ __forceinline__ void put(unsigned i, unsigned b)
    {
        const unsigned v = b << (8u * (i & 3u)), q = i >> 2;
        w0 |= q == 0 ? v : 0u;
        w1 |= q == 1 ? v : 0u;
        w2 |= q == 2 ? v : 0u;
        w3 |= q == 3 ? v : 0u;
    }
    // the text's allocation is padded to whole runs: the last run is stored whole as well
    __device__ __forceinline__ void store(uint8_t *out) const { *reinterpret_cast<uint4 *>(out) = make_uint4(w0, w1, w2, w3); }
};

template <unsigned K>
__global__ __launch_bounds__(kBlockLanes) void sample_iid(const TextGeom g, const unsigned *__restrict__ rows, const unsigned shared,
                                                          uint8_t *__restrict__ out)
{
    constexpr unsigned W = row_words(K);
    __shared__ unsigned long long s_dst[kLdsSlab];
    __shared__ unsigned s_row[W];
    if (threadIdx.x < W)
        s_row[threadIdx.x] = rows[threadIdx.x];
    const Slab dst = stage_slab(g, s_dst);  // (synchronises)
    const unsigned long long d0 = (unsigned long long)blockIdx.x * kTile + (unsigned long long)threadIdx.x * kRun;
    if (d0 >= g.total)
        return;
    const unsigned n = (unsigned)min((unsigned long long)kRun, g.total - d0);
    unsigned row[W];
#pragma unroll
    for (unsigned s = 0; s < W; ++s)
        row[s] = s_row[s];
    RunBytes bytes;
    walk_run(
        g, dst, d0, n,
        [&](unsigned long long live) {
            if (!shared) {
                const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(rows + live * W);
#pragma unroll
                for (unsigned s = 0; s < W / 4; ++s) {
                    const uint4 v = src[s];
                    row[4 * s] = v.x, row[4 * s + 1] = v.y, row[4 * s + 2] = v.z, row[4 * s + 3] = v.w;
                }
            }
        },
        [&](unsigned i, bool, unsigned u) {
            unsigned x = row[K - 1];
#pragma unroll
            for (unsigned s = 0; s + 1 < K; ++s)
                x += u > row[s] ? 1u : 0u;
            bytes.put(i, x);
        });
    bytes.store(out + d0);
}

// ---- order 1 -----------------------------------------------------------------------------------------------------------------

// the inclusive scan of one map per lane over the wavefront, in lane order
__device__ __forceinline__ unsigned wave_scan_maps(unsigned v)
{
    const unsigned lane = threadIdx.x & 63u;
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)v, off, 64);
        if (lane >= off)
            v = map_compose(t, v);
    }
    return v;
}

// The map of this lane's run; with s_maps, the map of byte i of the run goes to s_maps[i * kBlockLanes + lane] as well.
__device__ __forceinline__ unsigned run_map(const TextGeom &g, const Slab &dst, const MarkovModel &m, unsigned short *s_maps)
{
    const unsigned long long d0 = (unsigned long long)blockIdx.x * kTile + (unsigned long long)threadIdx.x * kRun;
    unsigned acc = kIdentityMap;
    if (d0 < g.total) {
        const unsigned n = (unsigned)min((unsigned long long)kRun, g.total - d0);
        walk_run(
            g, dst, d0, n, [](unsigned long long) {},
            [&](unsigned i, bool first, unsigned u) {
                const unsigned map = first ? markov_first(m, u) : markov_step(m, u);
                if (s_maps)
                    s_maps[i * kBlockLanes + threadIdx.x] = (unsigned short)map;
                acc = map_compose(acc, map);
            });
    }
    return acc;
}

__global__ __launch_bounds__(kBlockLanes) void markov_tiles(const TextGeom g, const MarkovModel m, unsigned *__restrict__ tile_maps)
{
    __shared__ unsigned long long s_dst[kLdsSlab];
    __shared__ unsigned s_wave[kBlockLanes / 64];
    const Slab dst = stage_slab(g, s_dst);
    const unsigned scanned = wave_scan_maps(run_map(g, dst, m, nullptr));
    if ((threadIdx.x & 63u) == 63u)
        s_wave[threadIdx.x >> 6] = scanned;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned acc = s_wave[0];
        for (unsigned w = 1; w < kBlockLanes / 64; ++w)
            acc = map_compose(acc, s_wave[w]);
        tile_maps[blockIdx.x] = acc;
    }
}

// carry[t] = the symbol in front of tile t: (tile 0, then ... tile t - 1)(anything), 0 for tile 0, which begins a record
__global__ __launch_bounds__(kBlockLanes) void markov_carry(const unsigned *__restrict__ tile_maps, const unsigned ntiles,
                                                            uint8_t *__restrict__ carry)
{
    __shared__ unsigned s_wave[kBlockLanes / 64];
    unsigned state = 0;  // what enters the chunk (uniform)
    for (unsigned t0 = 0; t0 < ntiles; t0 += kBlockLanes) {
        const unsigned t = t0 + threadIdx.x;
        const unsigned own = t < ntiles ? tile_maps[t] : kIdentityMap;
        const unsigned scanned = wave_scan_maps(own);
        if ((threadIdx.x & 63u) == 63u)
            s_wave[threadIdx.x >> 6] = scanned;
        __syncthreads();
        unsigned x = state, all = state;
        for (unsigned w = 0; w < kBlockLanes / 64; ++w) {
            if (w < (threadIdx.x >> 6))
                x = map_apply(s_wave[w], x);
            all = map_apply(s_wave[w], all);
        }
        unsigned before = (unsigned)__shfl_up((int)scanned, 1, 64);  // the exclusive prefix inside the wavefront
        if ((threadIdx.x & 63u) == 0)
            before = kIdentityMap;
        if (t < ntiles)
            carry[t] = (uint8_t)map_apply(before, x);
        state = all;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
}

__global__ __launch_bounds__(kBlockLanes) void markov_emit(const TextGeom g, const MarkovModel m, const uint8_t *__restrict__ carry,
                                                           uint8_t *__restrict__ out)
{
    __shared__ unsigned long long s_dst[kLdsSlab];
    __shared__ unsigned short s_maps[kRun * kBlockLanes];
    __shared__ unsigned s_wave[kBlockLanes / 64];
    const Slab dst = stage_slab(g, s_dst);
    const unsigned scanned = wave_scan_maps(run_map(g, dst, m, s_maps));
    if ((threadIdx.x & 63u) == 63u)
        s_wave[threadIdx.x >> 6] = scanned;
    __syncthreads();
    unsigned x = carry[blockIdx.x];
    for (unsigned w = 0; w < (threadIdx.x >> 6); ++w)
        x = map_apply(s_wave[w], x);
    unsigned before = (unsigned)__shfl_up((int)scanned, 1, 64);
    if ((threadIdx.x & 63u) == 0)
        before = kIdentityMap;
    x = map_apply(before, x);
    const unsigned long long d0 = (unsigned long long)blockIdx.x * kTile + (unsigned long long)threadIdx.x * kRun;
    if (d0 >= g.total)
        return;
    const unsigned n = (unsigned)min((unsigned long long)kRun, g.total - d0);
    unsigned w[kRun / 4] = {0, 0, 0, 0};
#pragma unroll
    for (unsigned i = 0; i < kRun; ++i)
        if (i < n) {  // (a lane reads the maps it wrote itself)
            x = map_apply(s_maps[i * kBlockLanes + threadIdx.x], x);
            w[i / 4] |= x << (8 * (i % 4));
        }
    *reinterpret_cast<uint4 *>(out + d0) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace sample
using namespace sample;

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

int draw_set(lm_hip_ctx *ctx, Plan &p, size_t n, size_t cols, uint64_t seed, uint64_t record_base, lm_hip_seqset **out)
{
    Made m(ctx);
    LM_HIP_TRY(hipMalloc(&m.d_offsets, (n + 1) * sizeof(unsigned long long)));
    LM_HIP_TRY(hipMemcpyAsync(m.d_offsets, p.offsets.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    const size_t stride = lm_hip_stride(cols, 1);
    LM_TRY(seq_alloc(ctx, (size_t)p.nrows, stride, cols, (size_t)p.total, p.k, &m.seq));
    if (p.nlive) {
        // scratch: the image | the threshold rows | the tile maps and carries (order 1) | the joined text, padded to whole runs
        const unsigned grid = (unsigned)((p.total + kTile - 1) / kTile);
        const size_t image_bytes = align256(p.image.size() * 8), rows_bytes = align256(p.rows.size() * 4 + 16);
        const size_t maps_bytes = p.order1 ? align256((size_t)grid * 4) : 0, carry_bytes = p.order1 ? align256(grid) : 0;
        const size_t text_bytes = align256((size_t)p.total + kRun);
        LM_TRY(ctx->scratch.reserve(image_bytes + rows_bytes + maps_bytes + carry_bytes + text_bytes));
        char *block = static_cast<char *>(ctx->scratch.ptr);
        unsigned long long *d_image = reinterpret_cast<unsigned long long *>(block);
        unsigned *d_rows = reinterpret_cast<unsigned *>(block + image_bytes);
        unsigned *d_maps = reinterpret_cast<unsigned *>(block + image_bytes + rows_bytes);
        uint8_t *d_carry = reinterpret_cast<uint8_t *>(block + image_bytes + rows_bytes + maps_bytes);
        uint8_t *d_text = reinterpret_cast<uint8_t *>(block + image_bytes + rows_bytes + maps_bytes + carry_bytes);
        LM_HIP_TRY(hipMemcpyAsync(d_image, p.image.data(), p.image.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        TextGeom g;
        g.image = d_image;
        g.nlive = p.nlive;
        g.total = p.total;
        g.seed = seed;
        g.record_base = record_base;
        // option "time_scan": the draw kernels between events (lm_hip_ctx_last_scan_kernel_ms; phase [1]: the stripe kernel)
        scan_timer_begin(ctx, ctx->stream);
        if (p.order1) {
            hipLaunchKernelGGL(markov_tiles, dim3(grid), dim3(kBlockLanes), 0, ctx->stream, g, p.chain, d_maps);
            hipLaunchKernelGGL(markov_carry, dim3(1), dim3(kBlockLanes), 0, ctx->stream, d_maps, grid, d_carry);
            hipLaunchKernelGGL(markov_emit, dim3(grid), dim3(kBlockLanes), 0, ctx->stream, g, p.chain, d_carry, d_text);
            ctx->last_kernel = "markov_emit";
        } else {
            LM_HIP_TRY(hipMemcpyAsync(d_rows, p.rows.data(), p.rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            if (p.k == kDna)
                hipLaunchKernelGGL(sample_iid<kDna>, dim3(grid), dim3(kBlockLanes), 0, ctx->stream, g, d_rows, p.shared ? 1u : 0u, d_text);
            else
                hipLaunchKernelGGL(sample_iid<kProtein>, dim3(grid), dim3(kBlockLanes), 0, ctx->stream, g, d_rows, p.shared ? 1u : 0u,
                                   d_text);
            ctx->last_kernel = "sample_iid";
        }
        LM_HIP_TRY(hipGetLastError());
        scan_timer_end(ctx, ctx->stream);
        StripeTile t;
        t.d_src = d_text;
        t.pitch = (size_t)p.nrows;
        t.len = (size_t)p.total;
        t.rows = (size_t)p.nrows;
        t.rbase = 0;
        t.nrows = (size_t)p.nrows;
        t.cols = cols;
        t.stride = stride;
        t.def = (uint8_t)(p.k - 1);
        t.d_data = m.seq->d_data;
        t.transform = StripeTile::None;
        t.k = p.k;
        const char *drew = ctx->last_kernel;
        LM_TRY(launch_stripe_tile(ctx, t));
        ctx->last_kernel = drew;
        scan_timer_mark(ctx, ctx->stream, 2);
    }
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    scan_timer_read(ctx);
    lm_hip_seq *seq = m.seq;
    unsigned long long *d_offsets = m.d_offsets;
    m.seq = nullptr, m.d_offsets = nullptr;  // the set owns them from here on
    return seqset_adopt(ctx, seq, std::move(p.offsets), d_offsets, out);
}

}  // namespace

}  // namespace lm

using namespace lm;

extern "C" {

size_t lm_hip_sample_tile_bytes(void) { return sample::kTile; }

int lm_hip_seqset_sample(lm_hip_ctx *ctx, char alphabet, const uint64_t *lengths, size_t n_records, const float *frequencies,
                         size_t n_models, const float *transitions, uint64_t seed, uint64_t record_base, size_t cols,
                         lm_hip_seqset **out)
{
    if (out)
        *out = nullptr;
    sample::Args a;
    a.ctx = ctx != nullptr, a.out = out != nullptr;
    a.alphabet = alphabet;
    a.lengths = lengths, a.n_records = n_records;
    a.frequencies = frequencies, a.n_models = n_models;
    a.transitions = transitions;
    a.cols = cols;
    std::string msg;
    int status = sample::check(a, &msg);
    if (status != LM_HIP_OK)
        return fail(status, "seqset_sample: %s", msg.c_str());
    sample::Plan p;
    try {
        status = sample::make_plan(a, &p, &msg);
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    if (status != LM_HIP_OK)
        return fail(status, "seqset_sample: %s", msg.c_str());
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    ScratchTrim trim(ctx);
    return draw_set(ctx, p, n_records, cols, seed, record_base, out);
}

}  // extern "C"
