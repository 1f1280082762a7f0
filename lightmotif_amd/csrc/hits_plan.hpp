// hits_plan.hpp -- the host arithmetic of hits.hip: which of the three ordering forms a hit list takes, the bucket geometry,
// the layout of the device scratch block (ctx->scratch2) and of the pinned staging block, and the layout of ctx->d_short.
// Pure functions, no HIP include: a host-only program compiles them (tests/cpp/test_hits_plan.cpp).  hits.hip launches and
// copies by a Plan and computes none of this itself.
//
// Planning takes two steps, because the radix sort's temporary size is rocPRIM's to tell:
//     Geometry g = choose_form(request);          // form, bucket geometry, n_sort, end_bit, grids
//     (hits.hip: Form::Sorted -> rocprim::radix_sort_pairs(nullptr, sort_temp, ... g.n_sort, 0, g.end_bit))
//     Plan p = lay_out(request, g, sort_temp);    // every region of both blocks
#pragma once

#include <algorithm>
#include <cstddef>

#include "lightmotif_hip.h"

namespace lm {
namespace hits {

constexpr unsigned long long kLowMask = (1ull << 40) - 1;  // key = (job << 40) | low
constexpr int kPlanBlock = 256;      // = kBlock, threads per workgroup of the ordering kernels (hits.hip asserts it)
constexpr int kPlanScanTile = 1024;  // = kScanTile (reduce.hip)
constexpr size_t kRecordBytes = 16;  // = sizeof(HitRecord)

constexpr unsigned long long kShortRecords = 40960;  // expected records (the previous call's count + 25 %) up to which a list is "short"
constexpr int kShortBuckets = 10496;                 // >= kShortRecords / 4 + 1 (bucket_geometry), a multiple of kBlock; 41 KB of LDS
constexpr size_t kShortTiles = kShortBuckets / kPlanScanTile + 1;
constexpr unsigned long long kSortFrom = 1ull << 17;  // expected records from which the list is radix-sorted
constexpr unsigned long long kPrefix = 12800;         // head of the list mirrored into the staging block; x 20 B = 256 KB
// ctx->d_short: counts | cursors | tiles (zero for ever: one "tile" per kScanTile buckets, see bucket_start) | offsets |
// the list's counters (zero between calls) | their copy for the ranking kernel, which clears the originals
constexpr size_t kShortOffCursors = kShortBuckets * 4, kShortOffTiles = 2 * kShortOffCursors,
                 kShortOffOffsets = kShortOffTiles + 128,
                 kShortOffCounters = (kShortOffOffsets + (kShortBuckets + 1) * 8 + 255) / 256 * 256,  // {hits, candidates}: a line of their own
                 kShortOffCopy = kShortOffCounters + 256, kShortOffTicket = kShortOffCopy + 128,  // (the ticket of hits_rank_emit's last workgroup)
                 kShortBytes = kShortOffCopy + 256;
static_assert(kShortTiles * 8 <= 128 && kShortBuckets % kPlanBlock == 0 && kShortRecords / 4 + 1 <= kShortBuckets, "layout of the short form");

// bucket geometry for `sized_for` expected records (one place: the re-scoring kernel counts with it)
inline void bucket_geometry(unsigned long long sized_for, size_t njobs, unsigned long long max_low, int *shift_out,
                            unsigned long long *nb_out)
{
    // ~1 record per bucket on average; at most 2^26 buckets.  (Ranking is quadratic in the bucket
    // size and the density is far from uniform across jobs: in the JASPAR batch a length-4 motif
    // has 150 x the average hit density; at 8 records per average bucket its buckets held 2 800
    // records and hits_rank_emit took 7 ms of the batch's 47.)
    int shift = 5;
    const long double universe = (long double)max_low * (long double)njobs;
    while (shift < 40 && ((long double)(1ull << shift) * (long double)sized_for < 1.0L * universe))
        ++shift;
    while (shift < 40 && (((max_low - 1) >> shift) + 1) * njobs > (1ull << 26))
        ++shift;
    // short lists (one motif at p = 1e-5 leaves ~10^4 hits per Gbp): four records per bucket keep the histogram small
    // (<= kShortBuckets: the short form; three tiles of the single-launch scan otherwise), and ranking 4 x 4 keys
    // costs nothing
    if (sized_for <= kShortRecords && njobs == 1 && shift + 2 < 40)
        shift += 2;
    *shift_out = shift;
    *nb_out = ((max_low - 1) >> shift) + 1;
}

// records a speculative ordering is sized for when `expected` were announced
inline unsigned long long speculative_size(unsigned long long expected) { return std::max<unsigned long long>(expected, 4096); }

// Short:   one job, a short list expected; the re-scoring kernel has counted per bucket (ShortOrder): scatter, rank
// Buckets: histogram, scan, scatter, rank
// Sorted:  split, radix sort, emit, starts
enum class Form { Short, Buckets, Sorted };
// Coords:  lm_hip_coords {low / cols, low % cols} + score      (Threshold, pli/mod.rs:215)
// Hits:    lm_hip_hit {low, score}                             (Scanner: low is the sequence position)
// Records: the record itself, key included, for the segment pass of seqset.hip, whose lm_hip_set_hit list is the result
enum class Output { Coords, Hits, Records };

inline const char *form_name(Form f) { return f == Form::Short ? "short" : f == Form::Buckets ? "buckets" : "sorted"; }

struct ShortGeometry {  // what short_order_begin handed to the re-scoring kernel
    bool on = false;
    int shift = 0;
    unsigned long long nb = 0;
};

// Form::Short is for a speculative ordering of ONE job whose list is expected short and whose histogram fits the LDS of
// hits_short_scatter; `on` = false otherwise (short_order_begin, hits.hip, sets the context's buffers up for it)
inline ShortGeometry short_geometry(unsigned long long expected, size_t njobs, unsigned long long max_low)
{
    ShortGeometry s;
    const unsigned long long sized_for = speculative_size(expected);
    if (njobs != 1 || sized_for > kShortRecords || max_low == 0 || max_low > kLowMask + 1)
        return s;
    bucket_geometry(sized_for, njobs, max_low, &s.shift, &s.nb);
    s.on = s.nb <= (unsigned long long)kShortBuckets;
    return s;
}

struct Request {
    bool speculative = false;      // the host has not read the count: sized for `count` EXPECTED records, room for `cap`
    unsigned long long count = 0;  // counted: the records of the list (> 0); speculative: the expected count
    unsigned long long cap = 0;    // capacity of the list
    size_t njobs = 1;
    unsigned long long max_low = 1;  // the keys' low parts are below it; 1 ... 2^40
    Output output = Output::Coords;
    bool sort_hits = true;         // context option: long lists by radix sort
    unsigned num_cus = 1;
    ShortGeometry short_geom;      // on: Form::Short, if the geometry is this plan's own
    unsigned seg_waves_per_group = 0;  // Output::Records: wave_counts entries per workgroup of the segment pass
    size_t staging_cap = 0, readback_cap = 0;  // bytes of kPinHitStaging / kPinHitReadback
};

struct Geometry {
    Form form = Form::Buckets;
    bool short_matches = true;  // false: Form::Short was begun with another geometry, or for a counted ordering
    unsigned long long sized_for = 0, room = 0;  // records the geometry expects / the arrays hold
    int shift = 0;
    unsigned long long nb = 0, nbuckets = 0, ntiles = 0;  // buckets per job, of the batch, scan tiles over them
    unsigned long long n_sort = 0;  // Sorted: keys sorted (unused slots hold a sentinel); 0 otherwise
    int end_bit = 41;               // keys are below njobs << 40; one spare bit keeps the all-ones sentinel strictly behind them
    unsigned long long pre = 0;        // speculative: records of the head of the RESULT mirrored into the staging block
    unsigned long long order_pre = 0;  // ... of them by the ordering's own emit (0 with a segment pass: the head of ITS output is mirrored)
    // a guess that is off by orders of magnitude (first call of a context: 4 096 expected, millions found) leaves hundreds
    // of records per bucket and a quadratic ranking pass (23 ms on the JASPAR batch): give up early, the counted form
    // costs a fraction of a millisecond
    unsigned long long max_bucket = ~0ull;
    bool inline_starts = true;  // Short / Buckets: one workgroup of hits_rank_emit writes the job starts (no hits_job_starts launch)
    unsigned grid = 1, starts_grid = 1, seg_grid = 1;  // ordering kernels | hits_job_starts, hits_sorted_starts (256 threads) | segment pass
};

inline Geometry choose_form(const Request &r)
{
    Geometry g;
    g.sized_for = r.speculative ? speculative_size(r.count) : r.count;
    g.room = r.speculative ? r.cap : r.count;
    bucket_geometry(g.sized_for, r.njobs, r.max_low, &g.shift, &g.nb);
    g.nbuckets = g.nb * r.njobs;
    g.ntiles = (g.nbuckets + kPlanScanTile - 1) / kPlanScanTile;
    // long lists: radix sort (see the head of hits.hip).  Speculative: the arrays hold the expected count with a quarter of
    // headroom; a longer list raises the abort flag and the counted form sorts the true count.
    const bool sorted = r.sort_hits && g.sized_for >= kSortFrom && r.njobs < (1ull << 22);
    g.form = r.short_geom.on ? Form::Short : sorted ? Form::Sorted : Form::Buckets;
    g.short_matches = !r.short_geom.on || (r.speculative && r.short_geom.shift == g.shift && r.short_geom.nb == g.nb && r.njobs == 1);
    g.n_sort = !sorted ? 0 : r.speculative ? std::min(g.room, g.sized_for + g.sized_for / 4 + 4096) : r.count;
    while ((1ull << (g.end_bit - 41)) < r.njobs)
        ++g.end_bit;
    // the previous call's length with headroom, bounded so that the staging copy stays a small pinned transfer
    g.pre = r.speculative ? std::min(g.room, std::min<unsigned long long>(std::max<unsigned long long>(g.sized_for, 2048), kPrefix)) : 0;
    g.order_pre = r.output == Output::Records ? 0 : g.pre;
    g.max_bucket = r.speculative ? 256 : ~0ull;
    g.inline_starts = r.njobs <= 1024;
    g.grid = (unsigned)std::max<unsigned long long>(
        std::min<unsigned long long>((g.sized_for + kPlanBlock - 1) / kPlanBlock, (unsigned long long)r.num_cus * 32), 1);
    g.starts_grid = (unsigned)((r.njobs + 1 + 255) / 256);
    g.seg_grid = (unsigned)std::max<unsigned long long>(
        std::min<unsigned long long>((g.sized_for + 1023) / 1024, (unsigned long long)r.num_cus * 4), 1);
    return g;
}

struct Region {
    size_t off = 0, bytes = 0, align = 16;  // `bytes` in use; `align` of the element type
    size_t end() const { return off + bytes; }
};

inline size_t align16(size_t x) { return (x + 15) / 16 * 16; }

struct Plan : Geometry {
    // ---- ctx->scratch2 ----
    // The ordering's work area starts the block.  Its two uses OVERLAY each other: `sort` is live in Form::Sorted alone,
    // `buckets` in the other two (Form::Short reads `grouped` only -- histogram, offsets and tiles live in ctx->d_short --
    // but the block keeps the room).  Everything below `work_end` is disjoint from both.
    struct {
        Region keys_in, keys_out, vals_in, vals_out, temp;
    } sort;
    struct {
        Region grouped, counts, offsets, tiles;
    } buckets;
    Region total;  // the scan's grand total
    // the result; counted form: starts | out | values come back as ONE copy (`readback_bytes`)
    Region starts, out, values;
    Region seg_counts, seg_starts, seg_out;  // Output::Records: survivors per wavefront | the jobs' new starts | the lm_hip_set_hit list
    size_t bytes = 0;
    // ---- pinned staging block (speculative): counters [0, 16) | abort flag | done word | starts | head of the list ----
    static constexpr size_t p_abort = 16, p_done = 24, p_starts = 32, p_head_zeroed = 32;
    size_t p_out = 0, p_values = 0, p_bytes = 0;
    bool staging_fits = false;
    // ---- counted read-back ----
    size_t rec_bytes = 0;        // of one entry of `out`
    size_t readback_bytes = 0;   // starts.off ... end of the values of `count` records
    bool readback_pinned = false;  // it fits kPinHitReadback: one copy into the pinned block
};

inline Plan lay_out(const Request &r, const Geometry &g, size_t sort_temp)
{
    Plan p;
    static_cast<Geometry &>(p) = g;
    const size_t njobs = r.njobs;
    p.rec_bytes = r.output == Output::Coords ? sizeof(lm_hip_coords) : sizeof(lm_hip_hit);
    // work area, use 1: the radix sort (all empty unless Form::Sorted, where n_sort > 0)
    p.sort.keys_in = {0, (size_t)g.n_sort * 8, 8};
    p.sort.keys_out = {p.sort.keys_in.off + align16(g.n_sort * 8), (size_t)g.n_sort * 8, 8};
    p.sort.vals_in = {p.sort.keys_out.off + align16(g.n_sort * 8), (size_t)g.n_sort * 4, 4};
    p.sort.vals_out = {p.sort.vals_in.off + align16(g.n_sort * 4), (size_t)g.n_sort * 4, 4};
    p.sort.temp = {p.sort.vals_out.off + align16(g.n_sort * 4), sort_temp, 16};
    // work area, use 2: the bucket passes
    p.buckets.grouped = {0, (size_t)g.room * kRecordBytes, 16};
    p.buckets.counts = {p.buckets.grouped.off + align16(g.room * kRecordBytes), (size_t)(g.nbuckets * 4 + 255) / 256 * 256, 4};  // whole 256-B units: one fill kernel
    p.buckets.offsets = {p.buckets.counts.end(), (size_t)g.nbuckets * 8, 8};
    p.buckets.tiles = {p.buckets.offsets.off + align16(g.nbuckets * 8), (size_t)g.ntiles * 8, 8};
    const size_t work_end = g.form == Form::Sorted ? (p.sort.temp.off + sort_temp + 255) / 256 * 256 : p.buckets.tiles.off + align16(g.ntiles * 8);
    p.total = {work_end, 8, 8};
    p.starts = {work_end + 16, (njobs + 1) * 8, 8};
    p.out = {p.starts.off + align16((njobs + 1) * 8), (size_t)g.room * p.rec_bytes, 16};
    p.values = {p.out.off + align16(g.room * p.rec_bytes), (size_t)g.room * sizeof(float), 4};
    const bool cut = r.output == Output::Records;
    p.seg_counts = {p.values.off + align16(g.room * sizeof(float)), cut ? (size_t)g.seg_grid * r.seg_waves_per_group * 4 : 0, 4};
    p.seg_starts = {p.seg_counts.off + (cut ? align16((size_t)g.seg_grid * r.seg_waves_per_group * 4) : 0), cut ? (njobs + 1) * 8 : 0, 8};
    p.seg_out = {p.seg_starts.off + (cut ? align16((njobs + 1) * 8) : 0), cut ? (size_t)g.room * sizeof(lm_hip_set_hit) : 0, 8};
    p.bytes = p.seg_out.off + (cut ? align16(g.room * sizeof(lm_hip_set_hit)) : 0);
    // the staging block lives in the context's pinned host buffer and the kernels write it THERE (posted writes over PCIe,
    // visible after the stream synchronisation): no copy command, no memset
    p.p_out = Plan::p_starts + align16((njobs + 1) * 8);
    p.p_values = p.p_out + align16(g.pre * (cut ? sizeof(lm_hip_set_hit) : p.rec_bytes));
    p.p_bytes = p.p_values + align16(g.pre * sizeof(float));
    p.staging_fits = p.p_bytes <= r.staging_cap;
    // counted form: small results come back as ONE copy into the pinned buffer (a copy into pageable memory costs ~15 us
    // each), large ones go straight into the arrays handed to the caller
    p.readback_bytes = r.speculative ? 0 : p.values.off + (size_t)r.count * sizeof(float) - p.starts.off;
    p.readback_pinned = !r.speculative && p.readback_bytes <= r.readback_cap;
    return p;
}

// the regions of ctx->scratch2 a plan's kernels and copies touch (the live use of the work area only); returns how many
inline int live_regions(const Plan &p, Output output, const Region *out[16])
{
    int n = 0;
    if (p.form == Form::Sorted)
        for (const Region *r : {&p.sort.keys_in, &p.sort.keys_out, &p.sort.vals_in, &p.sort.vals_out, &p.sort.temp})
            out[n++] = r;
    else
        for (const Region *r : {&p.buckets.grouped, &p.buckets.counts, &p.buckets.offsets, &p.buckets.tiles, &p.total})
            out[n++] = r;
    for (const Region *r : {&p.starts, &p.out, &p.values})
        out[n++] = r;
    if (output == Output::Records)
        for (const Region *r : {&p.seg_counts, &p.seg_starts, &p.seg_out})
            out[n++] = r;
    return n;
}

// ---- count -> scan -> fill (launch_scan_u32's arrays: reduce.hip, discrete.hip, composition.hip) -------------------------
// counts u32[n] | offsets u64[n] | tile totals u64[ntiles] | total u64; `bytes` = the end of the 16 bytes kept for the total
struct ScanLayout {
    size_t off_counts = 0, off_offsets = 0, off_tiles = 0, off_total = 0, bytes = 0;
};
inline ScanLayout scan_layout(unsigned long long n)
{
    ScanLayout s;
    const unsigned long long ntiles = (n + kPlanScanTile - 1) / kPlanScanTile;
    s.off_offsets = (size_t)((n * 4 + 15) / 16 * 16);
    s.off_tiles = s.off_offsets + (size_t)n * 8;
    s.off_total = s.off_tiles + (size_t)ntiles * 8;
    s.bytes = s.off_total + 16;
    return s;
}

}  // namespace hits
}  // namespace lm
