// The host half of csrc/variants.hip alone (csrc/variants_plan.hpp: no HIP, no device): the argument checks, the validity
// and clipping rules against 128-bit arithmetic, the window range against brute force, and the chunk / batch / group plans
// of random calls against what they must cover.  Needs nothing but a C++ compiler; meant to be built with
// -fsanitize=address,undefined as well.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "variants_plan.hpp"

using namespace lm::variants;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static unsigned long long rnd(unsigned long long &s)
{
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

static void check_arguments()
{
    std::string msg;
    Pointers p;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS && !msg.empty());  // the all-zero call
    p.ctx = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);
    p.set = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_OK);                            // n == 0, no variants: nothing else is needed
    p.n = 2;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);
    p.pssms = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);                  // no output
    p.effects = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_OK);
    p.n_variants = 3;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);
    p.variants = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_OK);
    p.hits_form = true;                                                     // the dense output is not what the hits form needs
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);
    p.thresholds = p.counts = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_ERR_BAD_ARGS);
    p.hits = true;
    CHECK(check_pointers(p, &msg) == LM_HIP_OK);
    p.n = 0, p.thresholds = p.counts = p.hits = p.pssms = false;            // n == 0 asks for none of them
    CHECK(check_pointers(p, &msg) == LM_HIP_OK);

    const size_t ms[] = {4, 12, 0}, ks[] = {5, 5, 5}, other[] = {5, 21, 5};
    CHECK(check_motifs(ms, ks, 3, 5, 10, true, &msg) == LM_HIP_OK);
    CHECK(check_motifs(ms, other, 3, 5, 10, true, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("matrix 1") != std::string::npos);
    CHECK(check_motifs(ms, ks, 3, 21, 10, true, &msg) == LM_HIP_ERR_BAD_ARGS);
    const size_t huge[] = {4, (size_t)1 << 32}, last[] = {4, ((size_t)1 << 32) - 1};
    CHECK(check_motifs(huge, ks, 2, 5, 10, true, &msg) == LM_HIP_ERR_CAPACITY && msg.find("matrix 1") != std::string::npos);
    CHECK(check_motifs(last, ks, 2, 5, 10, false, &msg) == LM_HIP_OK);
    CHECK(check_motifs(ms, ks, 3, 5, ~(size_t)0 / 8, true, &msg) == LM_HIP_ERR_CAPACITY);   // n * V * 16 overflows
    CHECK(check_motifs(ms, ks, 3, 5, ~(size_t)0 / 8, false, &msg) == LM_HIP_OK);            // (no dense block on the host)
}

static void check_rules()
{
    const unsigned long long edge[] = {0, 1, 2, 5, 9, 10, 11, 1ull << 31, 1ull << 32, (1ull << 63) - 1, 1ull << 63, (1ull << 63) + 3,
                                       ~0ull - 10, ~0ull - 1, ~0ull};
    const unsigned long long lens[] = {0, 1, 2, 10, 11, 1ull << 33, (1ull << 63) + 5, ~0ull};
    const unsigned ws[] = {1, 2, 3, 10, 11, 130, 0xFFFFFFFFu};
    for (unsigned long long records : {0ull, 1ull, 10ull, ~0ull})
        for (unsigned long long rec : edge)
            for (unsigned long long len : lens)
                for (unsigned long long pos : edge)
                    for (unsigned alt : {0u, 4u, 5u, 255u})
                        CHECK(variant_valid(rec, pos, alt, records, len, 5) == (rec < records && pos < len && alt < 5));
    for (unsigned long long len : lens)
        for (unsigned long long pos : edge) {
            if (pos >= len)
                continue;
            for (unsigned w : ws) {
                unsigned left = 77, right = 77;
                clip(pos, len, w, &left, &right);
                // lo = max(0, p - W + 1), hi = min(L - 1, p + W - 1), on 128 bits
                const __int128 lo = (__int128)pos - (w - 1) < 0 ? 0 : (__int128)pos - (w - 1);
                const __int128 hi = (__int128)pos + (w - 1) > (__int128)len - 1 ? (__int128)len - 1 : (__int128)pos + (w - 1);
                CHECK((__int128)pos - left == lo && (__int128)pos + right == hi);
                CHECK(left <= w - 1 && right <= w - 1);
            }
        }
    // the windows of a motif of m rows, from the clip of a neighbourhood of w >= m: brute force over small records
    for (unsigned len = 1; len <= 12; ++len)
        for (unsigned pos = 0; pos < len; ++pos)
            for (unsigned w = 1; w <= 14; ++w) {
                unsigned left, right;
                clip(pos, len, w, &left, &right);
                for (unsigned m = 0; m <= w; ++m) {
                    std::vector<unsigned> want;  // back = p - s over the starts s, descending start
                    for (long long s = (long long)len - (long long)m; m && s >= 0; --s)
                        if (s <= (long long)pos && pos < s + m)
                            want.push_back(pos - (unsigned)s);
                    unsigned lo = 99;
                    const unsigned count = windows(m, left, right, &lo);
                    CHECK(count == want.size());
                    for (unsigned t = 0; t < count && t < want.size(); ++t)
                        CHECK(lo + t == want[t]);
                }
            }
}

static void check_plan(unsigned long long seed)
{
    const size_t k = rnd(seed) % 2 ? 5 : 21;
    const size_t n = rnd(seed) % 200;
    const unsigned long long max_len = rnd(seed) % 4 == 0 ? rnd(seed) % 3 : 1 + rnd(seed) % 400;
    std::vector<size_t> ms(n);
    for (size_t &m : ms)
        m = rnd(seed) % 8 == 0 ? rnd(seed) % 500 : rnd(seed) % 40;
    const size_t nv = 1 + rnd(seed) % 5000;
    const size_t variant_chunk = rnd(seed) % 3 == 0 ? 0 : 1 + rnd(seed) % 300;
    const size_t lds = rnd(seed) % 3 == 0 ? 0 : 16 + rnd(seed) % 4000;
    const size_t block = rnd(seed) % 2 ? kBlockBytes : 4096 + rnd(seed) % 200000;
    Plan p;
    make_plan(ms.data(), n, k, max_len, nv, variant_chunk, lds, block, &p);

    // live motifs: those with rows that fit some record, in caller order
    size_t nlive = 0, w = 1;
    for (size_t i = 0; i < n; ++i) {
        const bool live = ms[i] && ms[i] <= max_len;
        CHECK((p.live_of[i] != kDead) == live);
        if (live) {
            CHECK(p.live_of[i] == nlive && p.live[nlive] == i);
            ++nlive;
            w = ms[i] > w ? ms[i] : w;
        }
    }
    CHECK(p.live.size() == nlive && p.w == w && p.nb == 2 * w - 1);
    // chunks cover the variants; a chunk respects the option and, beyond one variant / one motif, the block
    CHECK(p.chunk >= 1 && p.chunk <= nv && p.nchunks == (nv + p.chunk - 1) / p.chunk);
    CHECK(!variant_chunk || p.chunk <= variant_chunk);
    CHECK(variant_chunk || p.chunk <= kDefaultChunk);
    CHECK(p.chunk == 1 || p.chunk * (kVariantBytes + 9 + p.nb) <= block);
    CHECK(p.chunk == 1 || p.chunk * sizeof(lm_hip_variant_effect) <= block);
    CHECK(p.batch_motifs >= 1 && (p.batch_motifs == 1 || p.batch_motifs * p.chunk * sizeof(lm_hip_variant_effect) <= block));
    // LDS
    if (p.nb_in_lds) {
        CHECK((p.block == kWideBlock || p.block == kNarrowBlock) && p.nb * (p.block + kNbPad) <= kLdsNeighbourBytes);
        CHECK(p.nb_lds_bytes % 16 == 0 && p.nb_lds_bytes >= p.nb * (p.block + kNbPad));
        CHECK(p.block == kWideBlock || p.nb * (kWideBlock + kNbPad) > kLdsNeighbourBytes);
    } else {
        CHECK(p.nb * (kNarrowBlock + kNbPad) > kLdsNeighbourBytes && p.nb_lds_bytes == 0);
    }
    // batches and groups tile the live motifs in order
    const unsigned long long budget = (lds ? lds : kLdsTableBytes) / 4;
    size_t at = 0, group_at = 0, max_batch = 0, max_groups = 0;
    for (const Batch &b : p.batches) {
        CHECK(b.live0 == at && b.live1 > b.live0 && b.live1 - b.live0 <= p.batch_motifs);
        CHECK(b.group0 == group_at && b.group1 > b.group0);
        unsigned first = 0, lds_groups = 0;
        unsigned long long widest = 0;
        for (size_t gi = b.group0; gi < b.group1; ++gi) {
            const Group &g = p.groups[gi];
            CHECK(g.first == first && g.count >= 1 && g.count <= kGroupMotifs);
            unsigned long long floats = 0;
            for (unsigned x = 0; x < g.count; ++x) {
                const size_t li = b.live0 + g.first + x;
                const unsigned long long mine = table_floats(ms[p.live[li]], k);
                CHECK((mine <= budget) == g.lds);
                if (g.lds)
                    CHECK(p.tab[li] == floats);
                floats += mine;
            }
            CHECK(g.lds ? floats <= budget : g.count == 1);
            lds_groups += g.lds;
            widest = g.lds && floats > widest ? floats : widest;
            first += g.count;
        }
        CHECK(first == b.live1 - b.live0 && lds_groups == b.lds_groups && widest == b.table_floats);
        at = b.live1;
        group_at = b.group1;
        max_batch = b.live1 - b.live0 > max_batch ? b.live1 - b.live0 : max_batch;
        max_groups = b.group1 - b.group0 > max_groups ? b.group1 - b.group0 : max_groups;
    }
    CHECK(at == nlive && group_at == p.groups.size() && max_batch == p.max_batch && max_groups == p.max_groups);
}

int main()
{
    check_arguments();
    check_rules();
    for (unsigned long long seed = 1; seed <= 3000; ++seed)
        check_plan(seed * 0x9E3779B97F4A7C15ull);
    // the option: 10 variants at variant_chunk = 3 are four chunks; 70 short motifs cross a group boundary
    std::vector<size_t> ms(70, 8);
    Plan p;
    make_plan(ms.data(), ms.size(), 5, 100, 10, 3, 0, kBlockBytes, &p);
    CHECK(p.chunk == 3 && p.nchunks == 4 && p.batches.size() == 1 && p.groups.size() == 2 && p.groups[0].count == 64 && p.groups[1].count == 6);
    make_plan(ms.data(), ms.size(), 5, 100, 10, 0, 64, kBlockBytes, &p);   // 9 * 5 floats > 16: every motif on its own, from global memory
    CHECK(p.chunk == 10 && p.nchunks == 1 && p.groups.size() == 70 && !p.groups[0].lds && p.batches[0].lds_groups == 0);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_variants_plan: all checks passed\n");
    return 0;
}
