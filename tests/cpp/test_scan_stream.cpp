// The stream geometry of the discrete scans (lightmotif_amd/csrc/scan_stream.hpp) on the host: group counts, notes, the
// rows of a flagged note and the flag field.  A stand-alone program (no device, no HIP call), built by
// tests/test_cpp_scan_stream.py with the address and undefined-behaviour sanitizers.
//
// Geometries {MP, 1} for MP = 2, 4 ... 36 (one-symbol scans) and {RING, 2} for RING = 4, 8 ... 132 (pair scans); streams of
// q = 1, 2, 3, 62, 63, 64, 65, 127, 128, 129, 1000 and 2^30 / step groups beyond the first.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "scan_stream.hpp"

using namespace lm;
typedef unsigned long long u64;
typedef long long i64;

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

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()  // xorshift64*
{
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}

// the group that completes output row i of a stream, worked out from the kernels' description and not from note_rows: the
// FIRST group (0) completes rows 0 .. FIRST - 1, every later group STEP rows
template <int STEP, int FIRST>
static u64 completing_group(u64 i)
{
    return i < (u64)FIRST ? 0 : (i - FIRST) / STEP + 1;
}

// The counter every threshold scan spells out (score_prefilter.hpp, score_prefilter_blk.hpp, score_prefilter2.hpp): one
// step per group, then the tail.  -> notes taken.
static unsigned count_notes(unsigned ngroups, unsigned G)
{
    unsigned gleft = G, nnotes = 0;
    for (unsigned g = 0; g < ngroups; ++g)
        if (--gleft == 0) {
            gleft = G;
            ++nnotes;
        }
    if (gleft != G)  // the last, partly filled note
        ++nnotes;
    return nnotes;
}

template <int STEP, int FIRST>
static void check_stream(const StreamGeom geom, const u64 q)
{
    CHECK(geom.step == STEP && geom.first == FIRST, "geometry {%d, %d}", geom.step, geom.first);
    const u64 T = geom.rows(q);
    CHECK(T == q * STEP + FIRST && T <= (1ull << 30) + FIRST, "T = %llu", T);
    // group count: the shared function in both widths, and the kernels' 32-bit spellings of it
    CHECK((stream_groups<STEP, FIRST>(T)) == q + 1, "step %d q %llu", STEP, q);
    const unsigned ngroups = stream_groups<STEP, FIRST>((unsigned)T);
    CHECK(ngroups == q + 1, "step %d q %llu: %u", STEP, q, ngroups);
    CHECK(((unsigned)T - (unsigned)FIRST) / (unsigned)STEP + 1u == ngroups, "score_c32_prefilter_blk / _prefilter2 spelling");
    if (FIRST == 1)
        CHECK(((unsigned)T + (unsigned)STEP - 1u) / (unsigned)STEP == ngroups, "score_c32_prefilter spelling");
    // notes
    const unsigned G = groups_per_note(ngroups), nn = notes(ngroups);
    CHECK(G == (ngroups + 63u) / 64u, "the kernels' spelling of G");
    CHECK(nn >= 1 && nn <= 64, "%u notes", nn);
    CHECK((u64)nn * G >= ngroups && (u64)(nn - 1) * G < ngroups, "notes = ceil(groups / G): %u notes of %u for %u", nn, G, ngroups);
    CHECK(count_notes(ngroups, G) == nn, "counter: %u, notes() %u", count_notes(ngroups, G), nn);

    // an unshifted stream: the notes' ranges are in order, disjoint and tile its rows
    const i64 first_row = 12345;
    std::vector<std::pair<i64, i64>> whole(nn);
    i64 cursor = first_row;
    for (unsigned b = 0; b < nn; ++b) {
        i64 r0, r1;
        note_rows<STEP, FIRST>((int)b, G, ngroups, T, first_row, first_row, r0, r1);
        CHECK(r0 == cursor && r1 > r0, "bit %u: [%lld, %lld) after %lld", b, r0, r1, cursor);
        whole[b] = {r0, r1};
        cursor = r1;
    }
    CHECK(cursor == first_row + (i64)T, "the notes end at %lld, the stream at %lld", cursor, first_row + (i64)T);

    // the shifted last stream: only the rows from own_row on, every one once
    const u64 shifts[] = {1, (u64)STEP - 1, (u64)STEP, (u64)STEP + 1, T - 1};
    for (const u64 d : shifts) {
        if (d < 1 || d > T - 1)
            continue;
        const i64 own_row = first_row + (i64)d;
        cursor = own_row;
        for (unsigned b = 0; b < nn; ++b) {
            i64 r0, r1;
            note_rows<STEP, FIRST>((int)b, G, ngroups, T, first_row, own_row, r0, r1);
            if (r1 > r0) {
                CHECK(r0 == cursor, "shift %llu bit %u: [%lld, %lld) after %lld", d, b, r0, r1, cursor);
                cursor = r1;
            } else {
                CHECK(whole[b].second <= own_row, "shift %llu bit %u: empty, but its rows end at %lld", d, b, whole[b].second);
            }
        }
        CHECK(cursor == first_row + (i64)T, "shift %llu: ends at %lld", d, cursor);
    }

    // independently: the group that completes row i lies in the note whose range contains i
    auto check_row = [&](u64 i) {
        const u64 note = completing_group<STEP, FIRST>(i) / G;
        CHECK(note < nn, "row %llu: note %llu of %u", i, note, nn);
        CHECK(whole[note].first <= first_row + (i64)i && first_row + (i64)i < whole[note].second,
              "row %llu completes in note %llu = [%lld, %lld)", i, note, whole[note].first - first_row, whole[note].second - first_row);
    };
    if (T <= 20000) {
        for (u64 i = 0; i < T; ++i)
            check_row(i);
    } else {
        for (u64 i = 0; i < 64; ++i) {
            check_row(i);
            check_row(T - 1 - i);
        }
        for (unsigned b = 0; b < nn; ++b)
            for (i64 e = -3; e <= 3; ++e) {
                const i64 i = whole[b].second - first_row + e;
                if (i >= 0 && (u64)i < T)
                    check_row((u64)i);
            }
        for (int k = 0; k < 2000; ++k)
            check_row(rnd() % T);
    }
}

template <int STEP, int FIRST>
static void check_geometry(const StreamGeom geom)
{
    const u64 qs[] = {1, 2, 3, 62, 63, 64, 65, 127, 128, 129, 1000, (1ull << 30) / STEP};
    for (const u64 q : qs)
        check_stream<STEP, FIRST>(geom, q);
}

template <int... I>
static void check_one_symbol(std::integer_sequence<int, I...>)
{
    (check_geometry<2 * (I + 1), 1>(StreamGeom{2 * (I + 1), 1}), ...);  // MP = 2, 4 ... 36
}
template <int... I>
static void check_pairs(std::integer_sequence<int, I...>)
{
    (check_geometry<4 * (I + 1), 2>(StreamGeom{4 * (I + 1), 2}), ...);  // RING = 4, 8 ... 132 (M = 128: M' = 131)
}

// the families' geometries are among the ones checked above
static void check_family_geometries()
{
    for (int m = 1; m <= 36; ++m)
        for (int wide = 0; wide < 2; ++wide) {
            const StreamGeom g = one_symbol_geom(m, wide);
            CHECK(g.first == 1 && g.step >= m && g.step <= 36 && g.step % (wide ? 4 : 2) == 0 && g.step - m < (wide ? 4 : 2),
                  "one_symbol_geom(%d, %d) = {%d, %d}", m, wide, g.step, g.first);
        }
    for (int m = 2; m <= 128; ++m) {
        const StreamGeom g = pair_geom(m);
        CHECK(g.first == 2 && g.step > m && g.step <= 132 && g.step % 4 == 0 && g.step - m <= 4, "pair_geom(%d) = {%d, %d}", m, g.step, g.first);
    }
}

// GroupNotes::finish(n) against a plain 64-bit shift: after n notes the field's top n bits, oldest lowest
static void check_group_notes()
{
    for (unsigned n = 1; n <= 64; ++n)
        for (int trial = 0; trial < 50; ++trial) {
            GroupNotes notes;
            u64 ref = 0;
            for (unsigned k = 0; k < n; ++k) {
                const uint64_t r = rnd();
                const bool flag = (r & 3) == 0 || trial == 0;  // trial 0: every note flagged
                if (r & 4) {
                    notes.push((flag ? 0x80000000u : 0u) | (unsigned)(r >> 33));  // only bit 31 counts
                } else {
                    // note(): bit 15 of either half
                    unsigned mx = (unsigned)(r >> 32) & ~0x80008000u;
                    if (flag)
                        mx |= (r & 8) ? 0x8000u : 0x80000000u;
                    notes.note(mx);
                    CHECK(mx == 0, "note() clears the flags");
                }
                ref = (ref >> 1) | ((u64)flag << 63);
            }
            const u64 want = ref >> (64 - n);
            CHECK(notes.finish(n) == want, "n = %u: %016llx, plain shift %016llx", n, notes.finish(n), want);
        }
}

int main()
{
    check_one_symbol(std::make_integer_sequence<int, 18>());
    check_pairs(std::make_integer_sequence<int, 33>());
    check_family_geometries();
    check_group_notes();
    printf("test_scan_stream: all checks passed (%ld checks)\n", g_checks);
    return 0;
}
