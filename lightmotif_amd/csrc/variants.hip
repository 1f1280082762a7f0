// variants.hip -- what a single-symbol substitution does to the sites of every motif in a resident sequence set.
//
// A variant is (record, position p, alt symbol); for a motif of M rows the windows that cover p and lie inside the record
// start at s = max(0, p - M + 1) ... min(p, L - M).  Per (motif, variant) both alleles report their best window: the
// greatest score under f32 `>`, M sequential f32 adds from +0.0 in row order each (pli/mod.rs:96-105), NaN windows never
// competing, the LOWEST start among equals (the rule of seqset_best.hip).  This is no scan: at most M windows are scored
// twice over 2M - 1 symbols that are read once, so the record walk of seqset_walk.hpp is of no use here.
//
//   variant_gather          once per chunk of variants, split by OUTPUT byte as site_windows is: validates each variant
//                           and writes its clipped neighbourhood [p - W + 1, p + W - 1] (W = the longest live motif of the
//                           call, 0xFF outside the record) variant-major into scratch, the resident symbol at p (0xFF for
//                           an invalid variant) and how far the record reaches to either side (variants_plan.hpp: clip).
//                           Symbol q of the concatenation sits at row q % rows, column q / rows (pli/mod.rs:178-200); no
//                           address is formed from an invalid variant and nothing is read outside the record, so the
//                           wrap rows are never looked at.
//   variant_effects         one lane per variant; a workgroup loops over a GROUP of motifs whose transposed tables
//                           (table[s * ts + j], ts odd: the k symbol rows start on distinct banks) are staged in LDS from
//                           d_dense -- every matrix has that table, d_table exists only up to 36 rows.  The lanes'
//                           neighbourhoods sit in LDS byte-transposed (nb[j][lane], rows kNbPad bytes apart so that the
//                           transposing writes do not meet on one bank): a wavefront reads 64 consecutive bytes per step
//                           when its lanes are at the same window.  Windows are visited in ascending start with a
//                           strict `>`: the tie rule.  Both alleles add the SAME weights in the same order except at the
//                           variant's row, where the alt side adds the alt symbol's weight: one table read and two adds per
//                           step, never `ref - w + w'`.  (Forking the alt accumulator from the ref one at row p - s would
//                           save a quarter of the adds but makes the trip counts of a wavefront's lanes differ inside
//                           the window; the step is bound by its two LDS reads, which the fork does not save.)
//   variant_effects_global  the same kernel for ONE motif whose table exceeds the LDS budget: weights from d_dense.
//   variant_keep_count /    lm_hip_seqset_variant_hits: the dense block of a batch x chunk is compacted on the device, in
//   variant_keep_fill       (motif, variant) order; the host scans the per-tile counts in between (4 bytes per 256 cells).
// Motif length is a run-time value: one kernel, not a family per M.  Neighbourhoods too long for LDS (W > 241) are read
// from the scratch block instead.  The kernels are deliberately NOT in the kernel registry or the best-hit table.
// The host half (checks, rules, chunks, groups) is variants_plan.hpp.
#include <algorithm>
#include <cstring>

#include "lm_internal.hpp"
#include "variants_plan.hpp"

namespace lm {

namespace variants {

constexpr int kGatherBlock = 256;
constexpr int kGatherItems = 8;  // output bytes per lane of variant_gather
constexpr int kKeepBlock = 256;  // cells per tile of the compaction

struct SetGeom {
    const uint8_t *data;
    unsigned long long stride, rows;
    const unsigned long long *offsets;  // records + 1
    unsigned long long records;
    unsigned k;
};

struct MotifDesc {
    const float *dense;  // m x k row-major
    unsigned m;
    unsigned tab;        // first float of its LDS table
};

struct GroupDesc {
    unsigned first, count;
};

__device__ __forceinline__ unsigned long long div_u64(unsigned long long a, unsigned long long b)
{
    return ((a | b) >> 32) ? a / b : (unsigned long long)((unsigned)a / (unsigned)b);
}

__global__ __launch_bounds__(kGatherBlock) void variant_gather(const SetGeom g, const unsigned long long *__restrict__ vars,
                                                               const unsigned w, const unsigned long long nb,
                                                               const unsigned long long total, uint8_t *__restrict__ out,
                                                               uint8_t *__restrict__ ref_sym, uint2 *__restrict__ clips)
{
    const unsigned long long base = (unsigned long long)blockIdx.x * (kGatherBlock * kGatherItems) + threadIdx.x;
    const unsigned long long centre = (unsigned long long)w - 1;
#pragma unroll 2
    for (int it = 0; it < kGatherItems; ++it) {
        const unsigned long long o = base + (unsigned long long)it * kGatherBlock;
        if (o >= total)
            break;
        const unsigned long long v = div_u64(o, nb), j = o - v * nb;
        const unsigned long long rec = vars[3 * v], pos = vars[3 * v + 1];
        const unsigned alt = (unsigned)(vars[3 * v + 2] & 0xFFu);
        unsigned long long o0 = 0, len = 0;
        if (rec < g.records) {
            o0 = g.offsets[rec];
            len = g.offsets[rec + 1] - o0;
        }
        unsigned left = 0, right = 0;
        uint8_t byte = 0xFF;
        if (variant_valid(rec, pos, alt, g.records, len, g.k)) {
            clip(pos, len, w, &left, &right);
            if (j + left >= centre && j <= centre + right) {
                const unsigned long long q = o0 + (pos + j - centre);
                const unsigned long long col = div_u64(q, g.rows), row = q - col * g.rows;
                byte = g.data[row * g.stride + col];
            }
        }
        out[o] = byte;
        if (j == centre) {
            ref_sym[v] = byte;
            clips[v] = make_uint2(left, right);
        }
    }
}

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

template <bool TAB_LDS, bool NB_LDS>
__global__ __launch_bounds__(kWideBlock) void variant_effects(const MotifDesc *__restrict__ motifs, const GroupDesc *__restrict__ groups,
                                                              const unsigned tiles, const unsigned k, const unsigned w,
                                                              const unsigned long long *__restrict__ vars, const unsigned nv,
                                                              const uint8_t *__restrict__ nb_g, const uint8_t *__restrict__ ref_sym,
                                                              const uint2 *__restrict__ clips, const unsigned nb_lds_bytes,
                                                              lm_hip_variant_effect *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint8_t *s_nb = smem;
    float *s_tab = reinterpret_cast<float *>(smem + nb_lds_bytes);
    const unsigned bd = blockDim.x, tid = threadIdx.x;
    const unsigned group = blockIdx.x / tiles, tile = blockIdx.x - group * tiles;
    const GroupDesc G = groups[group];
    const unsigned v0 = tile * bd, v = v0 + tid;
    const unsigned nb = 2 * w - 1, pitch = bd + kNbPad;
    if (NB_LDS) {
        const unsigned here = min(bd, nv - v0), count = here * nb;
        const uint8_t *__restrict__ src = nb_g + (unsigned long long)v0 * nb;
        for (unsigned idx = tid; idx < count; idx += bd) {
            const unsigned vv = idx / nb, j = idx - vv * nb;
            s_nb[j * pitch + vv] = src[idx];
        }
    }
    if (TAB_LDS) {
        for (unsigned mi = 0; mi < G.count; ++mi) {
            const MotifDesc d = motifs[G.first + mi];
            const unsigned ts = d.m | 1u, cells = d.m * k;
            for (unsigned idx = tid; idx < cells; idx += bd) {
                const unsigned i = idx / k, s = idx - i * k;
                s_tab[d.tab + s * ts + i] = d.dense[idx];
            }
        }
    }
    __syncthreads();

    unsigned ref = 0xFF, alt = 0, left = 0, right = 0;
    if (v < nv) {
        ref = ref_sym[v];
        alt = (unsigned)(vars[3ull * v + 2] & 0xFFu);
        const uint2 c = clips[v];
        left = c.x;
        right = c.y;
    }
    const bool valid = ref != 0xFF;  // (what variant_gather wrote for an invalid variant)
    const uint8_t *__restrict__ my_nb = NB_LDS ? s_nb + tid : nb_g + (unsigned long long)(v < nv ? v : 0) * nb;
    const unsigned nb_step = NB_LDS ? pitch : 1u;

    for (unsigned mi = 0; mi < G.count; ++mi) {
        const MotifDesc d = motifs[G.first + mi];
        const unsigned M = d.m, ts = M | 1u;
        const float *__restrict__ tab = s_tab + d.tab;
        unsigned lo = 0;
        const unsigned count = valid ? windows(M, left, right, &lo) : 0u;
        float best_r = quiet_nan(), best_a = quiet_nan();
        unsigned back_r = LM_HIP_VARIANT_NONE, back_a = LM_HIP_VARIANT_NONE;
        for (unsigned t = 0; t < count; ++t) {
            const unsigned b = lo + count - 1 - t;  // ascending start = descending back
            const uint8_t *__restrict__ win = my_nb + (unsigned long long)(w - 1 - b) * nb_step;
            const float w_alt = TAB_LDS ? tab[alt * ts + b] : d.dense[(unsigned long long)b * k + alt];
            float r = 0.0f, a = 0.0f;
            for (unsigned i = 0; i < M; ++i) {
                const unsigned s = min((unsigned)win[(unsigned long long)i * nb_step], k - 1);
                const float x = TAB_LDS ? tab[s * ts + i] : d.dense[(unsigned long long)i * k + s];
                r += x;
                a += i == b ? w_alt : x;
            }
            if (r == r && !(r <= best_r)) {  // strictly greater, or the first: the lowest start of a tie stays
                best_r = r;
                back_r = b;
            }
            if (a == a && !(a <= best_a)) {
                best_a = a;
                back_a = b;
            }
        }
        if (v < nv) {
            lm_hip_variant_effect e;
            e.ref_score = best_r;
            e.alt_score = best_a;
            e.ref_back = back_r;
            e.alt_back = back_a;
            out[(unsigned long long)(G.first + mi) * nv + v] = e;
        }
    }
}

__device__ __forceinline__ bool kept(const lm_hip_variant_effect &e, float t) { return e.ref_score >= t || e.alt_score >= t; }

// counts[motif * tiles + tile]: the kept cells among the kKeepBlock cells of the tile
__global__ __launch_bounds__(kKeepBlock) void variant_keep_count(const lm_hip_variant_effect *__restrict__ dense, const float *__restrict__ ts,
                                                                 const unsigned nv, const unsigned tiles, unsigned *__restrict__ counts)
{
    const unsigned motif = blockIdx.x / tiles, tile = blockIdx.x - motif * tiles;
    const unsigned v = tile * kKeepBlock + threadIdx.x;
    const bool keep = v < nv && kept(dense[(unsigned long long)motif * nv + v], ts[motif]);
    const int total = __syncthreads_count(keep);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = (unsigned)total;
}

__global__ __launch_bounds__(kKeepBlock) void variant_keep_fill(const lm_hip_variant_effect *__restrict__ dense, const float *__restrict__ ts,
                                                                const unsigned nv, const unsigned tiles,
                                                                const unsigned long long *__restrict__ starts,
                                                                const unsigned long long variant0, lm_hip_variant_hit *__restrict__ out)
{
    __shared__ unsigned s_wave[kKeepBlock / 64];
    const unsigned motif = blockIdx.x / tiles, tile = blockIdx.x - motif * tiles;
    const unsigned v = tile * kKeepBlock + threadIdx.x;
    lm_hip_variant_effect e{};
    bool keep = false;
    if (v < nv) {
        e = dense[(unsigned long long)motif * nv + v];
        keep = kept(e, ts[motif]);
    }
    const unsigned long long mask = __ballot(keep);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
        s_wave[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned before = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    for (unsigned x = 0; x < wave; ++x)
        before += s_wave[x];
    if (keep) {
        lm_hip_variant_hit h;
        h.variant = variant0 + v;
        h.effect = e;
        out[starts[blockIdx.x] + before] = h;
    }
}

}  // namespace variants
using namespace variants;

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

namespace {

struct Call {
    const lm_hip_pssm *const *pssms = nullptr;
    size_t n = 0;
    const lm_hip_variant *vars = nullptr;
    size_t nv = 0;
    lm_hip_variant_effect *effects = nullptr;  // dense form
    const float *thresholds = nullptr;         // hits form
    std::vector<std::vector<lm_hip_variant_hit>> *kept = nullptr;
    uint8_t *ref_symbols = nullptr;
};

lm_hip_variant_effect none_effect()
{
    lm_hip_variant_effect e;
    const uint32_t nan_bits = 0x7FC00000u;
    memcpy(&e.ref_score, &nan_bits, 4);
    memcpy(&e.alt_score, &nan_bits, 4);
    e.ref_back = e.alt_back = LM_HIP_VARIANT_NONE;
    return e;
}

template <bool TAB_LDS>
int launch_effects(lm_hip_ctx *ctx, const Plan &p, unsigned ngroups, size_t lds, const MotifDesc *d_motifs, const GroupDesc *d_groups,
                   unsigned tiles, unsigned k, const unsigned long long *d_vars, unsigned nv, const uint8_t *d_nb, const uint8_t *d_ref,
                   const uint2 *d_clip, lm_hip_variant_effect *d_out)
{
    const dim3 grid(ngroups * tiles), block(p.block);
    if (p.nb_in_lds)
        hipLaunchKernelGGL((variant_effects<TAB_LDS, true>), grid, block, lds, ctx->stream, d_motifs, d_groups, tiles, k, p.w, d_vars, nv, d_nb,
                           d_ref, d_clip, p.nb_lds_bytes, d_out);
    else
        hipLaunchKernelGGL((variant_effects<TAB_LDS, false>), grid, block, lds, ctx->stream, d_motifs, d_groups, tiles, k, p.w, d_vars, nv, d_nb,
                           d_ref, d_clip, p.nb_lds_bytes, d_out);
    LM_HIP_TRY(hipGetLastError());
    ctx->last_kernel = TAB_LDS ? "variant_effects" : "variant_effects_global";
    return LM_HIP_OK;
}

int run(lm_hip_ctx *ctx, const lm_hip_seqset *set, const Call &c, const Plan &p)
{
    const size_t k = set->seq->k;
    const bool hits_form = c.kept != nullptr;
    // scratch: variants | resident symbols | clips | neighbourhoods | motifs | groups | thresholds | tile counts | tile starts | effects
    const size_t chunk = p.chunk, keep_tiles = (chunk + kKeepBlock - 1) / kKeepBlock;
    const size_t vars_bytes = align256(chunk * kVariantBytes), ref_bytes = align256(chunk), clip_bytes = align256(chunk * sizeof(uint2));
    const size_t nb_bytes = align256((size_t)(chunk * p.nb));
    const size_t motif_bytes = align256(p.max_batch * sizeof(MotifDesc)), group_bytes = align256(p.max_groups * sizeof(GroupDesc));
    const size_t ts_bytes = align256(p.max_batch * sizeof(float));
    const size_t cells = hits_form ? p.max_batch * keep_tiles : 0;
    const size_t count_bytes = align256(cells * sizeof(unsigned)), start_bytes = align256(cells * sizeof(unsigned long long));
    const size_t out_bytes = align256(p.max_batch * chunk * sizeof(lm_hip_variant_effect));
    LM_TRY(ctx->scratch.reserve(vars_bytes + ref_bytes + clip_bytes + nb_bytes + motif_bytes + group_bytes + ts_bytes + count_bytes +
                                start_bytes + out_bytes));
    char *at = static_cast<char *>(ctx->scratch.ptr);
    auto carve = [&](size_t bytes) {
        char *q = at;
        at += bytes;
        return q;
    };
    unsigned long long *d_vars = reinterpret_cast<unsigned long long *>(carve(vars_bytes));
    uint8_t *d_ref = reinterpret_cast<uint8_t *>(carve(ref_bytes));
    uint2 *d_clip = reinterpret_cast<uint2 *>(carve(clip_bytes));
    uint8_t *d_nb = reinterpret_cast<uint8_t *>(carve(nb_bytes));
    MotifDesc *d_motifs = reinterpret_cast<MotifDesc *>(carve(motif_bytes));
    GroupDesc *d_groups = reinterpret_cast<GroupDesc *>(carve(group_bytes));
    float *d_ts = reinterpret_cast<float *>(carve(ts_bytes));
    unsigned *d_counts = reinterpret_cast<unsigned *>(carve(count_bytes));
    unsigned long long *d_starts = reinterpret_cast<unsigned long long *>(carve(start_bytes));
    lm_hip_variant_effect *d_out = reinterpret_cast<lm_hip_variant_effect *>(carve(out_bytes));

    SetGeom g;
    g.data = set->seq->d_data;
    g.stride = set->seq->stride;
    g.rows = set->seq->rows;
    g.offsets = set->d_offsets;
    g.records = set->offsets.size() - 1;
    g.k = (unsigned)k;

    std::vector<MotifDesc> motifs;
    std::vector<GroupDesc> groups;  // the LDS groups of a batch, then the others
    std::vector<float> ts;
    std::vector<unsigned> counts;
    std::vector<unsigned long long> starts;
    std::vector<lm_hip_variant_hit> list;
    for (size_t ci = 0; ci < p.nchunks; ++ci) {
        const size_t v0 = ci * chunk, nv = std::min(chunk, c.nv - v0);
        LM_HIP_TRY(hipMemcpyAsync(d_vars, c.vars + v0, nv * kVariantBytes, hipMemcpyHostToDevice, ctx->stream));
        const unsigned long long total = (unsigned long long)nv * p.nb;
        const unsigned long long per_group = (unsigned long long)kGatherBlock * kGatherItems;
        if ((total + per_group - 1) / per_group >> 31)
            return fail(LM_HIP_ERR_CAPACITY, "seqset_variant_effects: a chunk of %llu neighbourhood bytes is beyond the grid", total);
        hipLaunchKernelGGL(variant_gather, dim3((unsigned)((total + per_group - 1) / per_group)), dim3(kGatherBlock), 0, ctx->stream, g, d_vars,
                           p.w, p.nb, total, d_nb, d_ref, d_clip);
        LM_HIP_TRY(hipGetLastError());
        ctx->last_kernel = "variant_gather";
        if (c.ref_symbols)
            LM_HIP_TRY(hipMemcpyAsync(c.ref_symbols + v0, d_ref, nv, hipMemcpyDeviceToHost, ctx->stream));
        const unsigned tiles = (unsigned)((nv + p.block - 1) / p.block);
        for (const Batch &b : p.batches) {
            const size_t nlive = b.live1 - b.live0;
            motifs.resize(nlive);
            ts.resize(nlive);
            for (size_t li = 0; li < nlive; ++li) {
                const size_t i = p.live[b.live0 + li];
                motifs[li] = MotifDesc{c.pssms[i]->d_dense, (unsigned)c.pssms[i]->m, p.tab[b.live0 + li]};
                ts[li] = hits_form ? c.thresholds[i] : 0.0f;
            }
            groups.clear();
            for (int lds = 1; lds >= 0; --lds)
                for (size_t gi = b.group0; gi < b.group1; ++gi)
                    if (p.groups[gi].lds == (lds != 0))
                        groups.push_back(GroupDesc{p.groups[gi].first, p.groups[gi].count});
            // (pageable sources: the copies have read them when they return)
            LM_HIP_TRY(hipMemcpyAsync(d_motifs, motifs.data(), nlive * sizeof(MotifDesc), hipMemcpyHostToDevice, ctx->stream));
            LM_HIP_TRY(hipMemcpyAsync(d_groups, groups.data(), groups.size() * sizeof(GroupDesc), hipMemcpyHostToDevice, ctx->stream));
            const unsigned nglobal = (unsigned)groups.size() - b.lds_groups;
            if (b.lds_groups)
                LM_TRY(launch_effects<true>(ctx, p, b.lds_groups, p.nb_lds_bytes + (size_t)b.table_floats * sizeof(float), d_motifs, d_groups, tiles,
                                            (unsigned)k, d_vars, (unsigned)nv, d_nb, d_ref, d_clip, d_out));
            if (nglobal)
                LM_TRY(launch_effects<false>(ctx, p, nglobal, p.nb_lds_bytes, d_motifs, d_groups + b.lds_groups, tiles, (unsigned)k, d_vars,
                                             (unsigned)nv, d_nb, d_ref, d_clip, d_out));
            if (!hits_form) {
                // row li of the block is motif p.live[b.live0 + li] of the call: runs of consecutive motifs go in one copy
                for (size_t li = 0; li < nlive;) {
                    size_t run = 1;
                    while (li + run < nlive && p.live[b.live0 + li + run] == p.live[b.live0 + li] + run)
                        ++run;
                    lm_hip_variant_effect *dst = c.effects + p.live[b.live0 + li] * c.nv + v0;
                    if (nv == c.nv)  // one chunk: the rows lie end to end on both sides
                        LM_HIP_TRY(hipMemcpyAsync(dst, d_out + li * nv, run * nv * sizeof(lm_hip_variant_effect), hipMemcpyDeviceToHost, ctx->stream));
                    else
                        LM_HIP_TRY(hipMemcpy2DAsync(dst, c.nv * sizeof(lm_hip_variant_effect), d_out + li * nv, nv * sizeof(lm_hip_variant_effect),
                                                    nv * sizeof(lm_hip_variant_effect), run, hipMemcpyDeviceToHost, ctx->stream));
                    li += run;
                }
                LM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the block is rewritten by the next batch)
                continue;
            }
            const unsigned ktiles = (unsigned)((nv + kKeepBlock - 1) / kKeepBlock);
            const size_t ncells = nlive * ktiles;
            LM_HIP_TRY(hipMemcpyAsync(d_ts, ts.data(), nlive * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(variant_keep_count, dim3((unsigned)ncells), dim3(kKeepBlock), 0, ctx->stream, d_out, d_ts, (unsigned)nv, ktiles,
                               d_counts);
            LM_HIP_TRY(hipGetLastError());
            counts.resize(ncells);
            LM_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, ncells * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
            LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
            starts.resize(ncells);
            unsigned long long total_kept = 0;
            for (size_t x = 0; x < ncells; ++x) {
                starts[x] = total_kept;
                total_kept += counts[x];
            }
            if (total_kept == 0)
                continue;
            LM_TRY(ctx->scratch2.reserve((size_t)total_kept * sizeof(lm_hip_variant_hit)));
            lm_hip_variant_hit *d_list = static_cast<lm_hip_variant_hit *>(ctx->scratch2.ptr);
            LM_HIP_TRY(hipMemcpyAsync(d_starts, starts.data(), ncells * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(variant_keep_fill, dim3((unsigned)ncells), dim3(kKeepBlock), 0, ctx->stream, d_out, d_ts, (unsigned)nv, ktiles,
                               d_starts, (unsigned long long)v0, d_list);
            LM_HIP_TRY(hipGetLastError());
            list.resize((size_t)total_kept);
            LM_HIP_TRY(hipMemcpyAsync(list.data(), d_list, (size_t)total_kept * sizeof(lm_hip_variant_hit), hipMemcpyDeviceToHost, ctx->stream));
            LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (size_t li = 0; li < nlive; ++li) {
                const unsigned long long a = starts[li * ktiles];
                const unsigned long long e = li + 1 < nlive ? starts[(li + 1) * ktiles] : total_kept;
                std::vector<lm_hip_variant_hit> &dst = (*c.kept)[p.live[b.live0 + li]];
                dst.insert(dst.end(), list.begin() + a, list.begin() + e);
            }
        }
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the chunk's variants are replaced by the next one's)
    }
    return LM_HIP_OK;
}

int variants_call(const char *what, lm_hip_ctx *ctx, const lm_hip_seqset *set, Call &c, size_t *counts, lm_hip_variant_hit **hits)
{
    const bool hits_form = counts != nullptr || hits != nullptr || c.thresholds != nullptr;
    std::string msg;
    int status = LM_HIP_OK;
    const size_t k = set->seq->k;
    {
        std::vector<size_t> ms(c.n), ks(c.n);
        for (size_t i = 0; i < c.n; ++i) {
            if (!c.pssms[i])
                return fail(LM_HIP_ERR_BAD_ARGS, "%s: matrix %zu is null", what, i);
            ms[i] = c.pssms[i]->m;
            ks[i] = c.pssms[i]->k;
        }
        status = check_motifs(ms.data(), ks.data(), c.n, k, c.nv, !hits_form, &msg);
        if (status != LM_HIP_OK)
            return fail(status, "%s: %s", what, msg.c_str());
        if (set->device != ctx->device)
            return fail(LM_HIP_ERR_BAD_ARGS, "%s: the set lives on device %d, the context on %d", what, set->device, ctx->device);
        if (hits_form && c.n) {
            for (size_t i = 0; i < c.n; ++i)
                counts[i] = 0;
            *hits = nullptr;
        }
        if (c.n == 0 || c.nv == 0)
            return LM_HIP_OK;
        unsigned long long max_len = 0;
        for (size_t r = 0; r + 1 < set->offsets.size(); ++r)
            max_len = std::max<unsigned long long>(max_len, set->offsets[r + 1] - set->offsets[r]);
        Plan p;
        make_plan(ms.data(), c.n, k, max_len, c.nv, ctx->variant_chunk, ctx->variant_lds_bytes, kBlockBytes, &p);
        // what no kernel writes: the cells of dead motifs
        if (!hits_form) {
            const lm_hip_variant_effect none = none_effect();
            for (size_t i = 0; i < c.n; ++i)
                if (p.live_of[i] == kDead)
                    std::fill(c.effects + i * c.nv, c.effects + (i + 1) * c.nv, none);
        }
        std::vector<std::vector<lm_hip_variant_hit>> kept(hits_form ? c.n : 0);
        if (hits_form)
            c.kept = &kept;
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            DeviceGuard guard(ctx->device);
            ScratchTrim trim(ctx);
            LM_TRY(run(ctx, set, c, p));
        }
        if (!hits_form)
            return LM_HIP_OK;
        size_t total = 0;
        for (size_t i = 0; i < c.n; ++i)
            total += kept[i].size();
        if (total == 0)
            return LM_HIP_OK;
        ResultArray<lm_hip_variant_hit> host(total);
        if (!host.p)
            return fail(LM_HIP_ERR_OOM, "%s: cannot allocate %zu entries on the host", what, total);
        size_t at = 0;
        for (size_t i = 0; i < c.n; ++i) {
            counts[i] = kept[i].size();
            if (counts[i])
                memcpy(host.p + at, kept[i].data(), counts[i] * sizeof(lm_hip_variant_hit));
            at += counts[i];
        }
        *hits = host.release();
    }
    return LM_HIP_OK;
}

}  // namespace

}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_seqset_variant_effects(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const lm_hip_seqset *set,
                                  const lm_hip_variant *variants, size_t n_variants, lm_hip_variant_effect *effects, uint8_t *ref_symbols)
{
    variants::Pointers ptrs;
    ptrs.ctx = ctx, ptrs.set = set, ptrs.pssms = pssms, ptrs.variants = variants, ptrs.effects = effects;
    ptrs.n = n, ptrs.n_variants = n_variants;
    std::string msg;
    const int status = variants::check_pointers(ptrs, &msg);
    if (status != LM_HIP_OK)
        return fail(status, "seqset_variant_effects: %s", msg.c_str());
    Call c;
    c.pssms = pssms, c.n = n, c.vars = variants, c.nv = n_variants, c.effects = effects, c.ref_symbols = ref_symbols;
    return variants_call("seqset_variant_effects", ctx, set, c, nullptr, nullptr);
}

int lm_hip_seqset_variant_hits(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *thresholds, size_t n, const lm_hip_seqset *set,
                               const lm_hip_variant *variants, size_t n_variants, size_t *counts, lm_hip_variant_hit **hits,
                               uint8_t *ref_symbols)
{
    variants::Pointers ptrs;
    ptrs.ctx = ctx, ptrs.set = set, ptrs.pssms = pssms, ptrs.variants = variants, ptrs.hits_form = true;
    ptrs.thresholds = thresholds, ptrs.counts = counts, ptrs.hits = hits;
    ptrs.n = n, ptrs.n_variants = n_variants;
    std::string msg;
    const int status = variants::check_pointers(ptrs, &msg);
    if (status != LM_HIP_OK)
        return fail(status, "seqset_variant_hits: %s", msg.c_str());
    if (n == 0) {  // (nothing to zero: counts has n entries)
        if (hits)
            *hits = nullptr;
        if (set->device != ctx->device)
            return fail(LM_HIP_ERR_BAD_ARGS, "seqset_variant_hits: the set lives on device %d, the context on %d", set->device, ctx->device);
        return LM_HIP_OK;
    }
    Call c;
    c.pssms = pssms, c.n = n, c.vars = variants, c.nv = n_variants, c.thresholds = thresholds, c.ref_symbols = ref_symbols;
    return variants_call("seqset_variant_hits", ctx, set, c, counts, hits);
}

}  // extern "C"
