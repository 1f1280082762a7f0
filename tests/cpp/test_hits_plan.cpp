// The host arithmetic of the hit-list ordering (lightmotif_amd/csrc/hits_plan.hpp): form choice, bucket geometry, the
// layout of the device scratch block and of the pinned staging block, the counted form's read-back block, and the layout
// of launch_scan_u32's arrays.  A stand-alone program (no device, no HIP call), built by tests/test_cpp_hits_plan.py with
// the address and undefined-behaviour sanitizers.
//
// (a) holds the plan against `Restated`: the offset chain, the staging chain, the grids and the bucket geometry as the
//     single 360-line order_hits computed them before the plan existed, restated here expression by expression with its
//     own constants -- a plan that moves one byte for one input of the sweep fails.
// (b) checks what that function never checked: alignment, containment, disjointness outside the declared overlay, and
//     that the counted read-back block is contiguous.
// (c) form choice at each boundary, inline_starts at 1024 / 1025;  (d) the staging request and the pinned read-back on
//     both sides of their capacities;  (e) the scan arrays against the three sites' old formulas.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "hits_plan.hpp"

using namespace lm::hits;

static long g_checks = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        ++g_checks;                                                  \
        if (!(cond)) {                                               \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                            \
            fprintf(stderr, "\n");                                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// ---- the arithmetic restated ----------------------------------------------------------------------------------------------

static void geometry_restated(unsigned long long sized_for, size_t njobs, unsigned long long max_low, int *shift_out,
                              unsigned long long *nb_out)
{
    int shift = 5;
    const long double universe = (long double)max_low * (long double)njobs;
    while (shift < 40 && ((long double)(1ull << shift) * (long double)sized_for < 1.0L * universe))
        ++shift;
    while (shift < 40 && (((max_low - 1) >> shift) + 1) * njobs > (1ull << 26))
        ++shift;
    if (sized_for <= 40960 && njobs == 1 && shift + 2 < 40)
        shift += 2;
    *shift_out = shift;
    *nb_out = ((max_low - 1) >> shift) + 1;
}

static size_t a16(size_t x) { return (x + 15) / 16 * 16; }

struct Restated {
    bool short_error;
    unsigned long long sized_for, room, nb, nbuckets, ntiles, n_sort, pre, order_pre, max_bucket;
    int shift, end_bit;
    bool sorted, inline_starts;
    size_t off_keys_in, off_keys_out, off_vals_in, off_vals_out, off_sort_temp, off_grouped, off_counts, off_offsets, off_tiles,
        off_total, off_starts, off_out, off_values, off_seg_counts, off_seg_starts, off_seg_out, bytes;
    size_t p_abort, p_done, p_starts, p_out, p_values, p_bytes;
    unsigned grid, seg_grid, starts_grid;
    size_t block_bytes, counts_fill;
};

// `emit`: 0 coords, 1 hits; `cut`: the segment pass (emit 1).  count == ~0: speculative.  sort_temp(n_sort, end_bit) stands
// for rocPRIM's answer.
static Restated restate(unsigned long long count, unsigned long long cap, unsigned long long expected, size_t njobs,
                        unsigned long long max_low, int emit, bool cut, bool sort_hits, unsigned num_cus, bool so_on, int so_shift,
                        unsigned long long so_nb, unsigned seg_waves, size_t (*sort_temp_of)(unsigned long long, int))
{
    Restated r{};
    const bool speculative = count == ~0ull;
    const unsigned long long sized_for = speculative ? std::max<unsigned long long>(expected, 4096) : count;
    const unsigned long long room = speculative ? cap : count;
    int shift = 0;
    unsigned long long nb = 0;
    geometry_restated(sized_for, njobs, max_low, &shift, &nb);
    const bool short_form = so_on;
    r.short_error = short_form && (!speculative || so_shift != shift || so_nb != nb || njobs != 1);
    const unsigned long long nbuckets = nb * njobs;
    const unsigned long long ntiles = (nbuckets + 1024 - 1) / 1024;
    const size_t rec_bytes = emit == 0 ? sizeof(lm_hip_coords) : sizeof(lm_hip_hit);
    const bool sorted = sort_hits && sized_for >= (1ull << 17) && njobs < (1ull << 22);
    const unsigned long long n_sort = !sorted ? 0 : speculative ? std::min(room, sized_for + sized_for / 4 + 4096) : count;
    int end_bit = 41;
    while ((1ull << (end_bit - 41)) < njobs)
        ++end_bit;
    size_t sort_temp = 0;
    if (sorted)
        sort_temp = sort_temp_of(n_sort, end_bit);
    const size_t off_keys_in = 0, off_keys_out = off_keys_in + a16(n_sort * 8);
    const size_t off_vals_in = off_keys_out + a16(n_sort * 8), off_vals_out = off_vals_in + a16(n_sort * 4);
    const size_t off_sort_temp = off_vals_out + a16(n_sort * 4);
    const size_t off_grouped = 0;
    const size_t off_counts = off_grouped + a16(room * 16);
    const size_t off_offsets = off_counts + (nbuckets * 4 + 255) / 256 * 256;
    const size_t off_tiles = off_offsets + a16(nbuckets * 8);
    const size_t off_total = sorted ? (off_sort_temp + sort_temp + 255) / 256 * 256 : off_tiles + a16(ntiles * 8);
    const unsigned long long pre =
        speculative ? std::min(room, std::min<unsigned long long>(std::max<unsigned long long>(sized_for, 2048), 12800)) : 0;
    const unsigned long long order_pre = cut ? 0 : pre;
    const size_t off_starts = off_total + 16;
    const size_t off_out = off_starts + a16((njobs + 1) * 8);
    const size_t off_values = off_out + a16(room * rec_bytes);
    const unsigned seg_grid = (unsigned)std::max<unsigned long long>(
        std::min<unsigned long long>((sized_for + 1023) / 1024, (unsigned long long)num_cus * 4), 1);
    const size_t off_seg_counts = off_values + a16(room * sizeof(float));
    const size_t off_seg_starts = off_seg_counts + (cut ? a16((size_t)seg_grid * seg_waves * 4) : 0);
    const size_t off_seg_out = off_seg_starts + (cut ? a16((njobs + 1) * 8) : 0);
    const size_t bytes = off_seg_out + (cut ? a16(room * sizeof(lm_hip_set_hit)) : 0);
    const size_t p_abort = 16, p_done = 24, p_starts = 32;
    const size_t p_out = p_starts + a16((njobs + 1) * 8);
    const size_t p_values = p_out + a16(pre * (cut ? sizeof(lm_hip_set_hit) : rec_bytes));
    const size_t p_bytes = p_values + a16(pre * sizeof(float));
    const unsigned long long max_bucket = speculative ? 256 : ~0ull;
    const unsigned grid = (unsigned)std::max<unsigned long long>(
        std::min<unsigned long long>((sized_for + 256 - 1) / 256, (unsigned long long)num_cus * 32), 1);
    r.sized_for = sized_for, r.room = room, r.nb = nb, r.nbuckets = nbuckets, r.ntiles = ntiles, r.n_sort = n_sort, r.pre = pre;
    r.order_pre = order_pre, r.max_bucket = max_bucket, r.shift = shift, r.end_bit = end_bit, r.sorted = sorted;
    r.inline_starts = njobs <= 1024;
    r.off_keys_in = off_keys_in, r.off_keys_out = off_keys_out, r.off_vals_in = off_vals_in, r.off_vals_out = off_vals_out;
    r.off_sort_temp = off_sort_temp, r.off_grouped = off_grouped, r.off_counts = off_counts, r.off_offsets = off_offsets;
    r.off_tiles = off_tiles, r.off_total = off_total, r.off_starts = off_starts, r.off_out = off_out, r.off_values = off_values;
    r.off_seg_counts = off_seg_counts, r.off_seg_starts = off_seg_starts, r.off_seg_out = off_seg_out, r.bytes = bytes;
    r.p_abort = p_abort, r.p_done = p_done, r.p_starts = p_starts, r.p_out = p_out, r.p_values = p_values, r.p_bytes = p_bytes;
    r.grid = grid, r.seg_grid = seg_grid, r.starts_grid = (unsigned)((njobs + 1 + 255) / 256);
    r.block_bytes = speculative ? 0 : off_values + count * sizeof(float) - off_starts;
    r.counts_fill = (nbuckets * 4 + 255) / 256 * 256;
    return r;
}

static size_t fake_sort_temp(unsigned long long n_sort, int end_bit) { return (size_t)(n_sort / 7 * 3 + 777 + (size_t)end_bit); }

constexpr size_t kStagingCap = 2u << 20, kReadbackCap = 256u << 10;  // kPinHitStaging, kPinHitReadback
constexpr unsigned kSegWaves = 4;

static Request request(bool speculative, unsigned long long count, unsigned long long cap, size_t njobs, unsigned long long max_low,
                       Output output, bool sort_hits, unsigned num_cus, ShortGeometry sg)
{
    Request q;
    q.speculative = speculative;
    q.count = count;
    q.cap = cap;
    q.njobs = njobs;
    q.max_low = max_low;
    q.output = output;
    q.sort_hits = sort_hits;
    q.num_cus = num_cus;
    q.short_geom = sg;
    q.seg_waves_per_group = kSegWaves;
    q.staging_cap = kStagingCap;
    q.readback_cap = kReadbackCap;
    return q;
}

static Plan plan(const Request &q)
{
    const Geometry g = choose_form(q);
    return lay_out(q, g, g.form == Form::Sorted ? fake_sort_temp(g.n_sort, g.end_bit) : 0);
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------

static void check_invariants(const Plan &p, const Request &q)
{
    const Region *live[16];
    const int n = live_regions(p, q.output, live);
    CHECK(n <= 16, "%d regions", n);
    for (int i = 0; i < n; ++i) {
        CHECK(live[i]->off % live[i]->align == 0, "region %d at %zu is not aligned to %zu", i, live[i]->off, live[i]->align);
        CHECK(live[i]->end() <= p.bytes, "region %d ends at %zu of %zu bytes", i, live[i]->end(), p.bytes);
        for (int j = 0; j < i; ++j)
            CHECK(live[j]->bytes == 0 || live[i]->bytes == 0 || live[j]->end() <= live[i]->off || live[i]->end() <= live[j]->off,
                  "regions %d [%zu, %zu) and %d [%zu, %zu) overlap", j, live[j]->off, live[j]->end(), i, live[i]->off, live[i]->end());
    }
    // the one declared overlay: both uses of the work area begin the block, and everything else lies behind BOTH of them when
    // it lies behind the live one -- the dead use's regions are never touched, so only the live one has to end before `total`
    CHECK(p.sort.keys_in.off == 0 && p.buckets.grouped.off == 0, "the work area begins the block");
    CHECK((p.form == Form::Sorted ? p.sort.temp.end() : p.buckets.tiles.end()) <= p.total.off, "the work area runs into the results");
    CHECK(p.form == Form::Sorted || p.n_sort == 0, "sort arrays outside the sorted form");
    // the staging block: head | starts | records | values, in that order, inside p_bytes
    CHECK(Plan::p_abort + 4 <= Plan::p_done && Plan::p_done + 4 <= Plan::p_starts && Plan::p_head_zeroed == Plan::p_starts, "staging head");
    CHECK(Plan::p_starts + (q.njobs + 1) * 8 <= p.p_out && p.p_out % 16 == 0 && p.p_values % 16 == 0, "staging starts");
    const size_t head_rec = q.output == Output::Records ? sizeof(lm_hip_set_hit) : p.rec_bytes;
    CHECK(p.p_out + p.pre * head_rec <= p.p_values && p.p_values + p.pre * sizeof(float) <= p.p_bytes, "staging head of the list");
    CHECK(p.pre <= p.room && p.order_pre <= p.pre, "more mirrored than there is room for");
    if (!q.speculative) {
        // contiguous: starts, records and values follow one another with nothing of another region between them
        CHECK(p.starts.off < p.out.off && p.out.off < p.values.off, "read-back block out of order");
        CHECK(p.out.off - p.starts.end() < 16 && p.values.off - p.out.end() < 16, "a gap in the read-back block");
        CHECK(p.readback_bytes == p.values.off + q.count * 4 - p.starts.off && p.starts.off + p.readback_bytes <= p.values.end(),
              "read-back block of %zu bytes", p.readback_bytes);
        CHECK(p.readback_pinned == (p.readback_bytes <= kReadbackCap), "pinned read-back of %zu bytes", p.readback_bytes);
    }
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------

static long g_plans = 0, g_forms[3] = {0, 0, 0}, g_mismatch = 0;

static void compare(bool speculative, unsigned long long count, unsigned long long cap, size_t njobs, unsigned long long max_low,
                    Output output, bool sort_hits, unsigned num_cus, ShortGeometry sg)
{
    const Request q = request(speculative, count, cap, njobs, max_low, output, sort_hits, num_cus, sg);
    const Restated r = restate(speculative ? ~0ull : count, cap, count, njobs, max_low, output == Output::Coords ? 0 : 1,
                               output == Output::Records, sort_hits, num_cus, sg.on, sg.shift, sg.nb, kSegWaves, fake_sort_temp);
    const Geometry g = choose_form(q);
    CHECK(g.short_matches == !r.short_error, "short geometry %d/%llu against %d/%llu", sg.shift, sg.nb, r.shift, r.nb);
    if (r.short_error) {  // (the ordering is refused: nothing is laid out)
        ++g_mismatch;
        return;
    }
    const Plan p = plan(q);
    ++g_plans;
    ++g_forms[(int)p.form];
#define SAME(field, want) CHECK((unsigned long long)(p.field) == (unsigned long long)(want), #field " %llu, was %llu (%s count %llu cap %llu njobs %zu max_low %llu output %d sort %d short %d)", \
                                (unsigned long long)(p.field), (unsigned long long)(want), speculative ? "speculative" : "counted", count, cap, njobs, max_low, (int)output, (int)sort_hits, (int)sg.on)
    CHECK(p.form == (sg.on ? Form::Short : r.sorted ? Form::Sorted : Form::Buckets), "form");
    SAME(sized_for, r.sized_for);
    SAME(room, r.room);
    SAME(shift, r.shift);
    SAME(nb, r.nb);
    SAME(nbuckets, r.nbuckets);
    SAME(ntiles, r.ntiles);
    SAME(n_sort, r.n_sort);
    SAME(end_bit, r.end_bit);
    SAME(pre, r.pre);
    SAME(order_pre, r.order_pre);
    SAME(max_bucket, r.max_bucket);
    SAME(inline_starts, r.inline_starts);
    SAME(grid, r.grid);
    SAME(seg_grid, r.seg_grid);
    SAME(starts_grid, r.starts_grid);
    SAME(sort.keys_in.off, r.off_keys_in);
    SAME(sort.keys_out.off, r.off_keys_out);
    SAME(sort.vals_in.off, r.off_vals_in);
    SAME(sort.vals_out.off, r.off_vals_out);
    SAME(sort.temp.off, r.off_sort_temp);
    SAME(buckets.grouped.off, r.off_grouped);
    SAME(buckets.counts.off, r.off_counts);
    SAME(buckets.counts.bytes, r.counts_fill);
    SAME(buckets.offsets.off, r.off_offsets);
    SAME(buckets.tiles.off, r.off_tiles);
    SAME(total.off, r.off_total);
    SAME(starts.off, r.off_starts);
    SAME(out.off, r.off_out);
    SAME(values.off, r.off_values);
    SAME(seg_counts.off, r.off_seg_counts);
    SAME(seg_starts.off, r.off_seg_starts);
    SAME(seg_out.off, r.off_seg_out);
    SAME(bytes, r.bytes);
    CHECK(Plan::p_abort == r.p_abort && Plan::p_done == r.p_done && Plan::p_starts == r.p_starts, "staging head");
    SAME(p_out, r.p_out);
    SAME(p_values, r.p_values);
    SAME(p_bytes, r.p_bytes);
    SAME(staging_fits, r.p_bytes <= kStagingCap);
    SAME(readback_bytes, r.block_bytes);
#undef SAME
    check_invariants(p, q);
}

static void test_sweep()
{
    const size_t jobs[] = {1, 2, 1024, 1025, 2346, (1u << 22) - 1, 1u << 22};
    const unsigned long long counts[] = {0, 1, 2047, 2048, 4095, 4096, 4097, 12800, 12801, 40960, 40961, 65536, (1ull << 17) - 1, 1ull << 17,
                                         (1ull << 17) + 1, 2600000, 1ull << 27};
    const unsigned long long lows[] = {1, 32, 1000000, 32000000, 1ull << 40};
    for (int speculative = 0; speculative < 2; ++speculative)
        for (size_t njobs : jobs)
            for (unsigned long long count : counts)
                for (unsigned long long max_low : lows)
                    for (Output output : {Output::Coords, Output::Hits, Output::Records})
                        for (int sort_hits = 0; sort_hits < 2; ++sort_hits)
                            for (unsigned num_cus : {256u, 8u}) {
                                if (!speculative && count == 0)
                                    continue;  // (an empty list is answered before anything is planned)
                                // capacities: the floor of a call (2^16), the expected count with the caller's half of headroom, a long list's
                                const unsigned long long caps[] = {1ull << 16, count + count / 2 + 1, (1ull << 27) + 64};
                                for (unsigned long long cap : caps) {
                                    if (!speculative && cap != caps[0])
                                        continue;  // (a counted plan does not read the capacity)
                                    compare(speculative, count, cap, njobs, max_low, output, sort_hits, num_cus, ShortGeometry{});
                                    if (output == Output::Records)
                                        continue;  // (a segment pass with a short ordering is refused before anything is planned)
                                    // a short geometry that is this plan's own, wherever one exists ...
                                    const ShortGeometry own = short_geometry(count, njobs, max_low);
                                    if (own.on && speculative)
                                        compare(true, count, cap, njobs, max_low, output, sort_hits, num_cus, own);
                                    // ... and one that is not: begun for another count, another shape, or for a counted ordering
                                    ShortGeometry other = own;
                                    other.on = true;
                                    other.shift = own.shift + 1;
                                    compare(speculative, count, cap, njobs, max_low, output, sort_hits, num_cus, other);
                                    other = short_geometry(count, 1, max_low);
                                    if (other.on && (njobs != 1 || !speculative))
                                        compare(speculative, count, cap, njobs, max_low, output, sort_hits, num_cus, other);
                                }
                            }
    CHECK(g_forms[0] > 100 && g_forms[1] > 1000 && g_forms[2] > 1000 && g_mismatch > 1000, "the sweep reached %ld short, %ld bucket, %ld sorted plans, %ld refusals",
          g_forms[0], g_forms[1], g_forms[2], g_mismatch);
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------

static Form form_of(bool speculative, unsigned long long count, size_t njobs, bool sort_hits = true, ShortGeometry sg = ShortGeometry{})
{
    return choose_form(request(speculative, count, 1u << 20, njobs, 32000000, Output::Hits, sort_hits, 256, sg)).form;
}

static void test_form_boundaries()
{
    // the sort from 2^17 records on, expected or counted
    CHECK(form_of(false, (1ull << 17) - 1, 1) == Form::Buckets && form_of(false, 1ull << 17, 1) == Form::Sorted, "counted, 2^17");
    CHECK(form_of(true, (1ull << 17) - 1, 1) == Form::Buckets && form_of(true, 1ull << 17, 1) == Form::Sorted, "speculative, 2^17");
    CHECK(form_of(false, 1ull << 17, 1, false) == Form::Buckets && form_of(true, 1ull << 20, 7, false) == Form::Buckets, "option sort_hits = 0");
    CHECK(form_of(false, 1ull << 20, (1u << 22) - 1) == Form::Sorted && form_of(false, 1ull << 20, 1u << 22) == Form::Buckets, "2^22 jobs");
    // a speculative ordering is never sized for fewer than 4 096 records
    CHECK(choose_form(request(true, 0, 1u << 16, 1, 32000000, Output::Hits, true, 256, ShortGeometry{})).sized_for == 4096, "floor of the guess");
    CHECK(choose_form(request(true, 4097, 1u << 16, 1, 32000000, Output::Hits, true, 256, ShortGeometry{})).sized_for == 4097, "above the floor");
    // the short form: one job, at most 40 960 records expected, a histogram of at most 10 496 buckets
    CHECK(short_geometry(40960, 1, 32000000).on && !short_geometry(40961, 1, 32000000).on, "kShortRecords");
    CHECK(!short_geometry(100, 2, 32000000).on && !short_geometry(100, 1, 0).on && !short_geometry(100, 1, (1ull << 40) + 1).on, "one job, a key space");
    CHECK(short_geometry(100, 1, 1ull << 40).on, "the whole key space");
    for (unsigned long long expected : {0ull, 4096ull, 10000ull, 40960ull})
        for (unsigned long long max_low : {1ull, 32ull, 1000000ull, 32000000ull, 1ull << 33, 1ull << 40}) {
            const ShortGeometry s = short_geometry(expected, 1, max_low);
            CHECK(s.on && s.nb <= (unsigned long long)kShortBuckets, "%llu buckets for %llu records over %llu cells", s.nb, expected, max_low);
            CHECK(form_of(true, expected, 1, true, s) == Form::Short, "short");
            const Geometry g = choose_form(request(true, expected, 1u << 16, 1, max_low, Output::Hits, true, 256, s));
            CHECK(g.short_matches && g.shift == s.shift && g.nb == s.nb, "the ordering recomputes the geometry the scan counted with");
            CHECK(!choose_form(request(false, 5000, 1u << 16, 1, max_low, Output::Hits, true, 256, s)).short_matches, "never counted");
        }
    // four records per bucket in the short range, one beyond it
    int s1, s2;
    unsigned long long nb;
    bucket_geometry(40960, 1, 1ull << 30, &s1, &nb);
    bucket_geometry(40961, 1, 1ull << 30, &s2, &nb);
    CHECK(s1 == s2 + 2, "shift %d at 40 960 records, %d at 40 961", s1, s2);
    // job starts: written by the ranking kernel up to 1 024 jobs, by a launch of their own beyond
    CHECK(choose_form(request(true, 5000, 1u << 16, 1024, 1000, Output::Coords, true, 256, ShortGeometry{})).inline_starts, "1024 jobs");
    CHECK(!choose_form(request(true, 5000, 1u << 16, 1025, 1000, Output::Coords, true, 256, ShortGeometry{})).inline_starts, "1025 jobs");
    CHECK(choose_form(request(true, 5000, 1u << 16, 1025, 1000, Output::Coords, true, 256, ShortGeometry{})).starts_grid == 5, "1026 starts");
    // layout of ctx->d_short
    CHECK(kShortOffCursors == 41984 && kShortOffTiles == 83968 && kShortOffOffsets == 84096 && kShortOffCounters == 168192 &&
              kShortOffCopy == 168448 && kShortOffTicket == 168576 && kShortBytes == 168704, "ctx->d_short");
}

// ---- (d) ----------------------------------------------------------------------------------------------------------------

static void test_staging_and_readback()
{
    // 2 MB of staging: 32 bytes of head, the starts, 12 800 x (16 + 4) bytes of list -> (2 MB - 32 - 256 000) / 8 - 1 jobs
    const size_t most = (kStagingCap - 32 - 12800 * 20) / 8 - 1;
    CHECK(most > 220000 && most < 240000, "%zu jobs", most);
    for (size_t njobs : {most - 1, most})
        CHECK(plan(request(true, 100000, 1u << 20, njobs, 1000, Output::Coords, true, 256, ShortGeometry{})).staging_fits, "%zu jobs fit", njobs);
    for (size_t njobs : {most + 1, most + 2, (size_t)1 << 22})
        CHECK(!plan(request(true, 100000, 1u << 20, njobs, 1000, Output::Coords, true, 256, ShortGeometry{})).staging_fits, "%zu jobs do not fit", njobs);
    CHECK(plan(request(true, 100, 1u << 16, 1, 1000, Output::Hits, true, 256, ShortGeometry{})).p_bytes == 32 + 16 + 4096 * 16 + 4096 * 4, "a first call");
    // a set's head is 24-byte entries
    CHECK(plan(request(true, 100, 1u << 16, 1, 1000, Output::Records, true, 256, ShortGeometry{})).p_values == 32 + 16 + 4096 * 24, "set hits");
    // counted read-back, one job: 16 bytes of starts + count x (16 + 4) -> 256 KB holds 13 106 records
    const unsigned long long most_records = (kReadbackCap - 16) / 20;
    for (Output output : {Output::Coords, Output::Hits}) {
        const Plan below = plan(request(false, most_records, 1u << 20, 1, 32000000, output, true, 256, ShortGeometry{}));
        const Plan above = plan(request(false, most_records + 1, 1u << 20, 1, 32000000, output, true, 256, ShortGeometry{}));
        CHECK(below.readback_pinned && below.readback_bytes <= kReadbackCap, "%zu bytes", below.readback_bytes);
        CHECK(!above.readback_pinned && above.readback_bytes > kReadbackCap, "%zu bytes", above.readback_bytes);
    }
    CHECK(!plan(request(true, 100, 1u << 16, 1, 1000, Output::Hits, true, 256, ShortGeometry{})).readback_pinned, "speculative: no block copy");
}

// ---- (e) ----------------------------------------------------------------------------------------------------------------

static void test_scan_layout()
{
    for (unsigned long long n : {1ull, 2ull, 3ull, 4ull, 5ull, 1023ull, 1024ull, 1025ull, 3072ull, 3073ull, 244141ull, 1ull << 20, (1ull << 31) + 3}) {
        const ScanLayout s = scan_layout(n);
        const unsigned long long ntiles = (n + 1024 - 1) / 1024;
        // reduce.hip launch_threshold and discrete.hip launch_threshold_u8 (nchunks = n)
        const size_t off_counts = 0;
        const size_t off_offsets = (n * 4 + 15) / 16 * 16;
        const size_t off_tiles = off_offsets + n * 8;
        const size_t off_total = off_tiles + ntiles * 8;
        CHECK(s.off_counts == off_counts && s.off_offsets == off_offsets && s.off_tiles == off_tiles && s.off_total == off_total &&
                  s.bytes == off_total + 16, "threshold, %llu chunks", n);
        // composition.hip launch_count_symbols (table | scanned | tiles | total | prefix ...)
        const size_t c_scanned = (size_t)((n * 4 + 15) / 16 * 16);
        const size_t c_tiles = c_scanned + (size_t)n * 8;
        const size_t c_total = c_tiles + (size_t)ntiles * 8;
        const size_t c_prefix = c_total + 16;
        CHECK(s.off_offsets == c_scanned && s.off_tiles == c_tiles && s.off_total == c_total && s.bytes == c_prefix, "composition, %llu counters", n);
        CHECK(s.off_offsets % 8 == 0 && s.off_tiles % 8 == 0 && s.off_total % 8 == 0 && n * 4 <= s.off_offsets, "alignment, %llu", n);
    }
}

int main()
{
    test_sweep();
    test_form_boundaries();
    test_staging_and_readback();
    test_scan_layout();
    printf("test_hits_plan: all checks passed (%ld checks, %ld plans against the restated chain)\n", g_checks, g_plans);
    return 0;
}
