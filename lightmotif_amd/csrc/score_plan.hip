// score_plan.hip -- kernel registry, the stream geometry every launch shares, scan planner and launcher of the fused routes.
#include <cstdio>
#include <cstring>
#include <mutex>

#include "score_launch.hpp"

namespace lm {

// ---- registry of the unrolled kernels (score_registry.hpp) ------------------------------------------------

static ScoreC32Launcher g_c32[kMaxStoreM + 1][kRegistrySlots];  // rows kMaxFastM + 1 ..: the long family (M % 4 == 0); beyond kMaxLongM: store only (M % 8 == 0)
static ScoreC32Launcher g_c32w[kMaxStoreM + 1][kRegistrySlots];  // wide alphabets (lds_wide(K))
static PrefilterLauncher g_prew[kMaxFastM + 1];
static PrefilterLauncher g_preblk[kMaxFastM + 1];
static ScoreU8Launcher g_u8w[kMaxFastM + 1];
static PrefilterLauncher g_pre[kMaxFastM + 1];
static PrefilterLauncher g_pre2[kMaxPairM + 1];  // DNA pair scan: every length up to kMaxPairM
static PrefilterLauncher g_pre2_protein[kMaxFastM + 1];
static ScoreU8Launcher g_u8[kMaxFastM + 1];
static ScoreU8Launcher g_u8_pairs[kMaxFastM + 1];
static PrefilterMultiLauncher g_pre2_multi[kMaxFastM + 1];
static char g_c32_names[kMaxStoreM + 1][3][32];
static char g_hole[96];  // "" = every promised row is filled
static std::once_flag g_c32_once;

// what LM_REGISTERING_UNITS promises: the store kernel for every M up to kMaxFastM and the padded lengths of the long
// (M % 4 == 0) and very long (M % 8 == 0) families; the DNA pair scan from 2 to kMaxPairM; one-symbol scan and u8 kernels
static void find_hole()
{
    auto check = [](bool filled, const char *row, int m) {
        if (!filled && !g_hole[0])
            snprintf(g_hole, sizeof g_hole, "kernel registry: no %s kernel for M = %d (a unit of the build is not registered)", row, m);
    };
    static const char *const slot_names[kRegistrySlots] = {"store", "fused argmax", "fused threshold", "dword-load store",
                                                           "store + block maxima", "continue", "16-column store", "tracked store"};
    for (int m = 1; m <= kMaxStoreM; ++m) {
        const bool fast = m <= kMaxFastM, lng = !fast && m <= kMaxLongM && m % 4 == 0, xlong = m > kMaxLongM && m % 8 == 0;
        if (!fast && !lng && !xlong)
            continue;
        for (int slot = 0; slot < kRegistrySlots; ++slot) {
            const bool quad = slot == SLOT_STORE_QL || slot == SLOT_STORE_TRACK;  // the members that need M % 4 == 0
            const bool promised = xlong ? (slot == SLOT_STORE || slot == SLOT_STORE_QL)
                                  : slot == SLOT_STORE_C16 ? fast && m % 4 == 0
                                  : quad ? m % 4 == 0
                                         : true;
            if (promised)
                check(g_c32[m][slot] && g_c32w[m][slot], slot_names[slot], m);
        }
    }
    for (int m = 2; m <= kMaxPairM; ++m)
        check(g_pre2[m], "pair scan", m);
    for (int m = 1; m <= kMaxFastM; ++m) {
        check(g_pre[m] && g_prew[m], "one-symbol scan", m);
        check(g_preblk[m], "block scan", m);
        check(g_u8[m] && g_u8w[m], "u8", m);
        if (m >= 2) {  // (the pair kernels start at two rows)
            check(g_pre2_protein[m], "protein pair scan", m);
            check(g_u8_pairs[m], "u8 pair", m);
            if (prefilter2_multi(m) > 1)
                check(g_pre2_multi[m], "multi-motif pair scan", m);
        }
        check(seqset_best_fused_row(m), "best-hit", m);
    }
}

// every non-null cell of the tables above and of seqset_best.hip's, in table order (lm_hip_registry_rows)
static std::vector<lm_hip_registry_row> registered_rows()
{
    std::vector<lm_hip_registry_row> rows;
    auto put = [&](int family, int wide, int m, int slot, const void *fn) {
        if (fn)
            rows.push_back(lm_hip_registry_row{family, wide, m, slot, (unsigned long long)reinterpret_cast<uintptr_t>(fn)});
    };
    for (int wide = 0; wide < 2; ++wide)
        for (int m = 0; m <= kMaxStoreM; ++m)
            for (int slot = 0; slot < kRegistrySlots; ++slot)
                put(LM_HIP_FAMILY_C32, wide, m, slot, reinterpret_cast<const void *>((wide ? g_c32w : g_c32)[m][slot]));
    for (int m = 0; m <= kMaxPairM; ++m)
        put(LM_HIP_FAMILY_PRE2, 0, m, 0, reinterpret_cast<const void *>(g_pre2[m]));
    for (int m = 0; m <= kMaxFastM; ++m) {
        put(LM_HIP_FAMILY_PRE, 0, m, 0, reinterpret_cast<const void *>(g_pre[m]));
        put(LM_HIP_FAMILY_PRE, 1, m, 0, reinterpret_cast<const void *>(g_prew[m]));
        put(LM_HIP_FAMILY_PREBLK, 1, m, 0, reinterpret_cast<const void *>(g_preblk[m]));
        put(LM_HIP_FAMILY_PRE2_PROTEIN, 1, m, 0, reinterpret_cast<const void *>(g_pre2_protein[m]));
        put(LM_HIP_FAMILY_PRE2_MULTI, 0, m, 0, reinterpret_cast<const void *>(g_pre2_multi[m]));
        put(LM_HIP_FAMILY_U8, 0, m, 0, reinterpret_cast<const void *>(g_u8[m]));
        put(LM_HIP_FAMILY_U8, 1, m, 0, reinterpret_cast<const void *>(g_u8w[m]));
        put(LM_HIP_FAMILY_U8_PAIRS, 0, m, 0, reinterpret_cast<const void *>(g_u8_pairs[m]));
        put(LM_HIP_FAMILY_BEST_FUSED, 0, m, 0, seqset_best_fused_row(m));
    }
    return rows;
}

static void init_registry()
{
    const KernelRegistry r{g_c32, g_pre, g_pre2, g_pre2_protein, g_u8, g_u8_pairs, g_pre2_multi, g_c32w, g_prew, g_u8w, g_preblk};
#define LM_CALL_UNIT(f) f(r);
    LM_REGISTERING_UNITS(LM_CALL_UNIT)
#undef LM_CALL_UNIT
    find_hole();
    for (int m = 0; m <= kMaxStoreM; ++m)
        for (int mode = 0; mode < 3; ++mode)
            snprintf(g_c32_names[m][mode], sizeof g_c32_names[m][mode], "score_c32<%d,%d>", m, mode);
}

const char *score_registry_hole()
{
    std::call_once(g_c32_once, init_registry);
    return g_hole[0] ? g_hole : nullptr;
}

ScoreC32Launcher score_c32_lookup(int M, int slot, bool wide)
{
    std::call_once(g_c32_once, init_registry);
    if (M < 1 || M > kMaxStoreM || slot < 0 || slot >= kRegistrySlots)
        return nullptr;
    if (slot == SLOT_STORE_C16 && M > kMaxFastM)
        return nullptr;  // the C = 16 kernel is a member of the short family only
    return (wide ? g_c32w : g_c32)[M][slot];
}

PrefilterLauncher score_c32_prefilter_lookup(int M, bool wide, bool blocks)
{
    std::call_once(g_c32_once, init_registry);
    return (M >= 1 && M <= kMaxFastM) ? (wide ? (blocks ? g_preblk[M] : g_prew[M]) : g_pre[M]) : nullptr;
}

PrefilterLauncher score_c32_prefilter2_lookup(int M, int K)
{
    std::call_once(g_c32_once, init_registry);
    if (M < 1 || M > (K == 5 ? kMaxPairM : kMaxFastM))
        return nullptr;
    return K == 5 ? g_pre2[M] : K == 21 ? g_pre2_protein[M] : nullptr;
}

PrefilterMultiLauncher score_c32_prefilter2_multi_lookup(int M)
{
    std::call_once(g_c32_once, init_registry);
    return (M >= 1 && M <= kMaxFastM) ? g_pre2_multi[M] : nullptr;
}

ScoreU8Launcher score_c32_lookup_u8(int M, bool pairs, bool wide)
{
    std::call_once(g_c32_once, init_registry);
    if (M < 1 || M > kMaxFastM)
        return nullptr;
    return pairs ? g_u8_pairs[M] : wide ? g_u8w[M] : g_u8[M];
}

}  // namespace lm

extern "C" int lm_hip_registry_rows(lm_hip_registry_row *rows, size_t cap, size_t *count)
{
    if (!count || (cap && !rows))
        return lm::fail(LM_HIP_ERR_BAD_ARGS, "registry_rows: null argument");
    std::call_once(lm::g_c32_once, lm::init_registry);
    const std::vector<lm_hip_registry_row> all = lm::registered_rows();
    *count = all.size();
    std::copy(all.begin(), all.begin() + std::min(cap, all.size()), rows);
    return LM_HIP_OK;
}

namespace lm {

const char *score_c32_name(int M, int mode)
{
    std::call_once(g_c32_once, init_registry);
    return (M >= 0 && M <= kMaxStoreM && mode >= 0 && mode < 3) ? g_c32_names[M][mode] : "score_c32";
}

// ---- stream geometry ---------------------------------------------------------------

ExactMotif exact_motif(const lm_hip_pssm *p, const uint8_t *d_seq)
{
    if (p->m <= (size_t)kMaxFastM)
        return ExactMotif{p->m, p->d_table, 0u};
    if (p->parts.size() == 1 && p->parts[0].m <= (size_t)kMaxLongM && reinterpret_cast<uintptr_t>(d_seq) % 4 == 0)
        return ExactMotif{p->parts[0].m, p->parts[0].d_table, (unsigned)p->parts[0].lead};
    return ExactMotif{};
}

C32Plan plan_c32(const lm_hip_ctx *ctx, const ScoreArgs &a, bool store, int prefilter, size_t batch)
{
    const size_t m = prefilter == 0 ? exact_motif(a.pssm, a.d_seq).m : a.pssm->m;
    const MotifShape ms{m, a.pssm->k, a.pssm->d_image2 != nullptr};
    return plan_c32(ctx, ms, a, store, prefilter, batch);
}

// `allow16`: the caller also has a kernel for C = 16 (plain store, score rows of 16 floats; a
// wavefront then carries four streams)
C32Plan plan_c32(const lm_hip_ctx *ctx, const MotifShape &ms, const ScoreArgs &a, bool store,
                        int prefilter, size_t batch, unsigned long long default_rows, bool allow16, bool plain_store)
{
    C32Plan p;
    const size_t K = ms.k;
    // rows per unrolled group and rows completed by a stream's first group: the discrete scans' from the StreamGeom
    // their kernels count groups with (scan_stream.hpp); the exact kernels step by the motif length
    const StreamGeom geom = prefilter == 2   ? pair_geom((int)ms.m)
                            : prefilter == 1 ? one_symbol_geom((int)ms.m, lds_wide((int)K))
                                             : StreamGeom{(int)ms.m, 1};
    const size_t M = (size_t)geom.step;
    const unsigned long long n = a.row_end - a.row_begin;
    const bool c16 = allow16 && store && prefilter == 0 && a.cols == 16;
    // the kernel stores rows in pairs: R full steps more per stream, which makes every stream length even
    const bool pairs = plain_store && store && prefilter == 0 && !c16 && store_pairs((int)ms.m, MODE_STORE, 32, 1, lds_wide((int)K) ? 1 : 0);
    const size_t extra = (size_t)geom.first + (pairs ? (size_t)store_extra_rows((int)ms.m) : 0);  // rows of a stream beyond q groups
    if ((a.cols != 32 && !c16) || a.seq_stride != 32 || (store && a.out_stride != a.cols))
        return p;
    if (ms.m < 1 || ms.m > (size_t)(prefilter == 0 ? (store ? kMaxStoreM : kMaxLongM) : (prefilter == 2 && K == 5) ? kMaxPairM : kMaxFastM) || n < M + extra)
        return p;
    if (prefilter == 0 && ms.m > (size_t)kMaxFastM && (ms.m % 4 != 0 || reinterpret_cast<uintptr_t>(a.d_seq) % 4 != 0))
        return p;  // the long family: padded lengths, dword symbol loads
    // (the pair-symbol kernel fetches symbols with dword loads: 4-byte aligned matrix)
    if (prefilter == 2 && ((K != 5 && !(K == 21 && ctx->pair_prefilter_protein)) || !ms.pair_table || ms.m < 2 ||
                           reinterpret_cast<uintptr_t>(a.d_seq) % 4 != 0))
        return p;
    const size_t lds = prefilter == 2   ? (size_t)prefilter2_image_dw((int)ms.m, (int)K) * 4
                       : prefilter == 1 ? (size_t)prefilter_image_dw((int)ms.m, (int)K) * 4
                                        : std::max<size_t>(K * table_stride((int)M, lds_wide((int)K)) * sizeof(float), 64);
    if (lds > 60 * 1024)
        return p;
    // The fused kernels write nothing, so they are LDS/VALU-bound and prefer long
    // streams (fewer fill steps): T=1001 0.69 ms vs T=61 0.79 ms on the same input.
    // Store kernel: three groups per stream (T = 3M + 1) up to M = 26, where the write pattern
    // binds and short streams keep the window of rows in flight compact (M = 12: T = 37 0.872 ms,
    // T = 73 0.894; M = 20: T = 61 0.940, T = 121 0.970; M = 24: T = 73 1.001, T = 145 1.024);
    // longer motifs are bound by the LDS gather and want the fill / drain groups amortised over
    // six groups (M = 28: T = 57 1.29 ms, T = 169 1.08; M = 33: T = 67 1.30, T = 199 1.22;
    // profiles/r02_edge_ab.txt).  Very short motifs keep ~24 rows per stream.
    // Paired stores (even M, plain store): T = q*M + 1 + R with R = 63 % M, so up to M = 26 the default stream is
    // q = 63 / M groups = 64 rows = 8 KB of score rows, every stream starts 256-byte aligned and no pair of rows
    // straddles two streams; a requested length goes to the nearest q.
    unsigned long long target = ctx->rows_per_stream ? ctx->rows_per_stream
                                : default_rows         ? default_rows
                                : !store               ? 1024
                                : prefilter != 0       ? 64
                                : ms.m > 26            ? 6 * M
                                : pairs                ? 64
                                                       : std::max<size_t>(3 * M, 24);
    // keep at least ~4 streams per SIMD lane-half in flight on small inputs
    // Enough workgroups for several rounds of the chip's resident capacity (6 x 256 CUs
    // of 8-stream workgroups), so the last partial round costs little; the fused
    // kernels run back to back per motif, where that tail is paid every launch.
    // (a multi-job launch brings `batch` times as many workgroups, so each job needs fewer)
    const unsigned long long want_streams =
        std::max<unsigned long long>((unsigned long long)ctx->num_cus * (store ? 64 : 128) / batch, 64);
    if (n / target < want_streams)
        target = std::max<unsigned long long>(n / want_streams, 1);
    target = std::min<unsigned long long>(target, 1ull << 30);  // step indices are 32-bit
    unsigned long long q = std::max<unsigned long long>(((pairs ? target - std::min<unsigned long long>(target, extra) : target) + M / 2) / M, 1);
    if (q * M + extra > n)
        q = (n - extra) / M;
    if (q < 1)
        return p;
    p.T = q * M + extra;
    p.nstreams = (n + p.T - 1) / p.T;
    const unsigned long long per_block = c16 ? 2 * kStreamsPerBlock : kStreamsPerBlock;
    p.grid = dim3((unsigned)((p.nstreams + per_block - 1) / per_block));
    p.lds = lds;
    p.ok = true;
    return p;
}

dim3 generic_grid(const lm_hip_ctx *ctx, unsigned long long ncells)
{
    unsigned long long blocks = (ncells + kBlock - 1) / kBlock;
    const unsigned long long cap = (unsigned long long)ctx->num_cus * 32;
    return dim3((unsigned)std::max<unsigned long long>(std::min(blocks, cap), 1));
}

size_t generic_lds(const lm_hip_pssm *p, int *use_lds)
{
    const size_t bytes = p->m * p->k * sizeof(float);
    *use_lds = bytes <= 48 * 1024 && bytes > 0;
    return std::max<size_t>(*use_lds ? bytes : 0, 64);
}

// ---- batches ---------------------------------------------------------------------------

int BatchStreams::fork()
{
    if (!two)
        return LM_HIP_OK;
    if (!ctx->aux_stream) {
        LM_HIP_TRY(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
        LM_HIP_TRY(hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming));
        LM_HIP_TRY(hipEventCreateWithFlags(&ctx->join_event, hipEventDisableTiming));
    }
    LM_HIP_TRY(hipEventRecord(ctx->fork_event, ctx->stream));
    LM_HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->fork_event, 0));
    return LM_HIP_OK;
}

int BatchStreams::join()
{
    if (!two)
        return LM_HIP_OK;
    LM_HIP_TRY(hipEventRecord(ctx->join_event, ctx->aux_stream));
    LM_HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->join_event, 0));
    return LM_HIP_OK;
}

// ---- the scans of a batch, hit lists and the head of a call (score_launch.hpp) -------------------------------

ScanPlan plan_scans(const lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, const std::vector<JobGroup> &groups, bool allow_drop)
{
    ScanPlan sp;
    sp.groups.resize(groups.size());
    sp.order.reserve(n + 4 * groups.size());
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const JobGroup &g = groups[gi];
        ScanGroup &sg = sp.groups[gi];
        sg.pos = sp.order.size();
        const lm_hip_pssm *p0 = jobs[g.idx[0]].pssm;
        sg.multi = g.kind == KIND_PREFILTER2 && ctx->multi_motif && g.idx.size() >= 2 && p0->k == 5 &&
                   score_c32_prefilter2_multi_lookup((int)p0->m);
        for (size_t i : g.idx) {
            sg.multi = sg.multi && jobs[i].pssm->d_image2_multi != nullptr;
            sp.order.push_back(ScanPlan::Pos{i, false});
        }
        if (sg.multi) {
            sg.per_pass = prefilter2_multi((int)p0->m);
            while ((sp.order.size() - sg.pos) % sg.per_pass)
                sp.order.push_back(ScanPlan::Pos{g.idx.back(), true});
        }
    }
    const lm_hip_pssm *p = jobs[0].pssm;
    if (allow_drop && n == 1 && groups.size() == 1 && groups[0].kind == KIND_PREFILTER2 && ctx->drop_last && p->d_image2_drop &&
        score_c32_prefilter2_lookup((int)p->m - 1, (int)p->k))
        sp.drop = plan_c32(ctx, MotifShape{p->m - 1, p->k, true}, jobs[0], false, 2, 1);
    return sp;
}

const void *scan_table(const ScanPlan &sp, size_t gi, int kind, const ScoreArgs &a)
{
    const lm_hip_pssm *p = a.pssm;
    return sp.drop.ok                ? (const void *)p->d_image2_drop
           : sp.groups[gi].multi     ? (const void *)p->d_image2_multi
           : kind == KIND_PREFILTER2 ? (const void *)p->d_image2
           : kind == KIND_PREFILTER  ? (const void *)p->d_image
           : kind == KIND_EXACT      ? (const void *)exact_motif(p, a.d_seq).table
                                     : (const void *)p->d_table;
}

void record_scan_shape(lm_hip_ctx *ctx, const ScanPlan &sp, const std::vector<JobGroup> &groups, const ScoreArgs *jobs, size_t n)
{
    ctx->last_scan_rows = ctx->last_scan_lds_bytes = 0;
    if (n != 1 || groups.size() != 1)
        return;
    const size_t scanned = jobs[0].pssm->m - (sp.drop.ok ? 1 : 0);
    const size_t em = groups[0].kind == KIND_EXACT ? exact_motif(jobs[0].pssm, jobs[0].d_seq).m : scanned;
    ctx->last_scan_lds_bytes = scan_lds_bytes(groups[0].kind, em, jobs[0].pssm->k);
    ctx->last_scan_rows = ctx->last_scan_lds_bytes ? (unsigned)scanned : 0u;
}

int launch_prefilter_scan(lm_hip_ctx *ctx, int kind, size_t m, size_t k, bool blocks, const C32Plan &plan, hipStream_t st,
                          const uint8_t *d_seq, size_t row_begin, size_t row_end, const unsigned *image, unsigned td,
                          const FusedOut &fo)
{
    const bool pairs = kind == KIND_PREFILTER2;
    ctx->last_kernel = pairs ? "score_c32_prefilter2" : blocks ? "score_c32_prefilter_blk" : "score_c32_prefilter";
    PrefilterLauncher fn = pairs ? score_c32_prefilter2_lookup((int)m, (int)k) : score_c32_prefilter_lookup((int)m, lds_wide((int)k), blocks);
    if (!fn)
        return fail(LM_HIP_ERR_HIP, "no %s kernel for M = %zu, K = %zu", ctx->last_kernel, m, k);
    tally_launch(ctx, pairs ? (k == 5 ? LM_HIP_FAMILY_PRE2 : LM_HIP_FAMILY_PRE2_PROTEIN) : blocks ? LM_HIP_FAMILY_PREBLK : LM_HIP_FAMILY_PRE,
                 lds_wide((int)k), m);
    LM_HIP_TRY(fn(plan.grid, plan.lds, st, d_seq, image, (int)k, row_begin, row_end, plan.T, plan.nstreams, td, fo));
    return LM_HIP_OK;
}

int launch_group_scan(lm_hip_ctx *ctx, const ScanPlan &sp, size_t gi, const JobGroup &g, const ScoreArgs &a, int mode, unsigned td,
                      hipStream_t st, const FusedOut &fo)
{
    const lm_hip_pssm *p = a.pssm;
    const ScanGroup &sg = sp.groups[gi];
    if (sg.multi) {  // several motifs of this length per pass over the sequence
        dim3 grid = g.plan.grid;
        grid.y = (unsigned)((g.idx.size() + sg.per_pass - 1) / sg.per_pass);
        ctx->last_kernel = "score_c32_prefilter2_multi";
        tally_launch(ctx, LM_HIP_FAMILY_PRE2_MULTI, false, p->m);
        LM_HIP_TRY(score_c32_prefilter2_multi_lookup((int)p->m)(grid, st, a.d_seq, a.row_begin, a.row_end, g.plan.T, g.plan.nstreams, fo));
        return LM_HIP_OK;
    }
    if (g.kind == KIND_PREFILTER2 && sp.drop.ok)
        return launch_prefilter_scan(ctx, g.kind, p->m - 1, p->k, false, sp.drop, st, a.d_seq, a.row_begin, a.row_end,
                                     p->d_image2_drop, td, fo);
    if (g.kind == KIND_PREFILTER || g.kind == KIND_PREFILTER2)
        return launch_prefilter_scan(ctx, g.kind, p->m, p->k, block_scan(ctx, a), g.plan, st, a.d_seq, a.row_begin, a.row_end,
                                     g.kind == KIND_PREFILTER2 ? p->d_image2 : p->d_image, td, fo);
    if (g.kind != KIND_EXACT || (mode != MODE_ARGMAX && mode != MODE_THRESHOLD))  // (a mode is a registry slot only up to MODE_THRESHOLD)
        return fail(LM_HIP_ERR_BAD_ARGS, "launch_group_scan: no fused kernel for kind %d in mode %d", g.kind, mode);
    const ExactMotif em = exact_motif(p, a.d_seq);  // (a group shares length, hence padding)
    FusedOut efo = fo;
    efo.lead_rows = em.lead;
    ScoreC32Launcher fn = score_c32_lookup((int)em.m, mode, lds_wide((int)p->k));
    ctx->last_kernel = score_c32_name((int)em.m, mode);
    if (!fn)
        return fail(LM_HIP_ERR_HIP, "no %s kernel", ctx->last_kernel);
    tally_launch(ctx, LM_HIP_FAMILY_C32, lds_wide((int)p->k), em.m, mode);
    LM_HIP_TRY(fn(g.plan.grid, g.plan.lds, st, a.d_seq, em.table, (int)p->k, a.row_begin, a.row_end, g.plan.T, g.plan.nstreams,
                  nullptr, efo));
    return LM_HIP_OK;
}

int reserve_hit_lists(lm_hip_ctx *ctx, size_t head_bytes, unsigned long long cap, unsigned long long ccap, size_t tail_bytes,
                      FusedOut *fo, char **base)
{
    const size_t off_cands = head_bytes + cap * sizeof(HitRecord);
    LM_TRY(ctx->scratch.reserve(off_cands + ccap * sizeof(Candidate) + tail_bytes));
    char *b = static_cast<char *>(ctx->scratch.ptr);
    fo->hit_count = reinterpret_cast<unsigned long long *>(b);
    fo->cand_count = fo->hit_count + 1;
    fo->hits = reinterpret_cast<HitRecord *>(b + head_bytes);
    fo->hit_capacity = cap;
    fo->cands = reinterpret_cast<Candidate *>(b + off_cands);
    fo->cand_capacity = ccap;
    *base = b;
    return LM_HIP_OK;
}

int upload_head(lm_hip_ctx *ctx, hipStream_t st, char *base, size_t head_bytes, size_t zero_bytes, const HeadPart *parts, size_t nparts)
{
    if (char *head = pinned_at<char>(ctx, kPinUploadHead, head_bytes)) {
        memset(head, 0, zero_bytes);
        for (size_t i = 0; i < nparts; ++i)
            if (parts[i].src)
                memcpy(head + parts[i].off, parts[i].src, parts[i].bytes);
            else
                std::fill_n(reinterpret_cast<unsigned *>(head + parts[i].off), parts[i].bytes / 4, parts[i].fill);
        LM_HIP_TRY(hipMemcpyAsync(base, head, head_bytes, hipMemcpyHostToDevice, st));
        return LM_HIP_OK;
    }
    LM_HIP_TRY(hipMemsetAsync(base, 0, 16, st));
    for (size_t i = 0; i < nparts; ++i)
        if (parts[i].src)
            LM_HIP_TRY(hipMemcpyAsync(base + parts[i].off, parts[i].src, parts[i].bytes, hipMemcpyHostToDevice, st));
        else
            LM_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(base + parts[i].off), (int)parts[i].fill, parts[i].bytes / 4, st));
    return LM_HIP_OK;
}

float best_kmer_score(const lm_hip_pssm *p)
{
    float b = 0.0f;
    for (size_t j = 0; j < p->m; ++j) {
        float best = p->host[j * p->k];
        for (size_t s = 1; s < p->k; ++s)
            best = p->host[j * p->k + s] > best ? p->host[j * p->k + s] : best;
        b = b + best;
    }
    return b;
}

bool chunked_ok(const lm_hip_ctx *ctx, const ScoreArgs &a)
{
    if (!ctx->chunked_fused)
        return false;
    const unsigned long long n = a.row_end - a.row_begin;
    if (a.cols == 32)
        return !a.pssm->parts.empty() && a.seq_stride == 32 && reinterpret_cast<uintptr_t>(a.d_seq) % 4 == 0 &&
               n > (unsigned long long)a.pssm->parts[0].m;
    return a.cols >= 1 && a.cols <= 4096 && n * a.cols >= (1ull << 16) && n > a.pssm->m;
}

// rows per chunk: ctx->chunk_rows is quoted for C = 32; other column counts keep the chunk's cell count
unsigned long long chunk_rows_for(const lm_hip_ctx *ctx, const ScoreArgs &a)
{
    return std::max<unsigned long long>((unsigned long long)ctx->chunk_rows * 32 / a.cols, 1);
}

unsigned long long chunk_count(const lm_hip_ctx *ctx, const ScoreArgs &a)
{
    const unsigned long long n = a.row_end - a.row_begin, per = chunk_rows_for(ctx, a);
    return (n + per - 1) / per;
}

// Workgroups of the per-chunk argmax (a full chunk is 2^25 cells)
unsigned chunk_argmax_grid(const lm_hip_ctx *ctx)
{
    return (unsigned)ctx->num_cus * 8;
}

}  // namespace lm
