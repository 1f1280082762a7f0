// The host half of csrc/sample.hip alone (csrc/sample_plan.hpp: no HIP, no device): the generator's known answers, the
// thresholds of a frequency row with their edges T = 0 and T = 2^32, row validity and the zero-row fallback, the offsets
// prefix, every refusal, the small vectors of the rule and the composition of packed maps against brute force.  Needs
// nothing but a C++ compiler; meant to be built with -fsanitize=address,undefined as well.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "sample_plan.hpp"

using namespace lm::sample;

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

static void check_known_answers()
{
    const unsigned cases[3][10] = {
        {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u},
    };
    for (const auto &c : cases) {
        unsigned v[4] = {c[0], c[1], c[2], c[3]};
        philox4x32_10(v, c[4], c[5]);
        for (int i = 0; i < 4; ++i)
            CHECK(v[i] == c[6 + i]);
    }
    // the counter of a position: (lo32(q), lo32(R), hi32(R), hi32(q)), key (lo32(seed), hi32(seed))
    unsigned a[4], b[4] = {0x85a308d3u, 0x13198a2eu, 0x03707344u, 0x243f6a88u};
    uniforms(0x299f31d0a4093822ull, 0x0370734413198a2eull, 0x243f6a8885a308d3ull, a);
    philox4x32_10(b, 0xa4093822u, 0x299f31d0u);
    for (int i = 0; i < 4; ++i)
        CHECK(a[i] == b[i]);
}

static void check_thresholds()
{
    const float f[5] = {0.3f, 0.2f, 0.15f, 0.35f, 0.0f};
    uint64_t T[4];
    thresholds(f, 5, T);
    CHECK(T[0] < T[1] && T[1] < T[2] && T[2] < T[3] && T[3] == 1ull << 32);
    CHECK(T[0] == (uint64_t)std::floor((double)f[0] / ((double)f[0] + (double)f[1] + (double)f[2] + (double)f[3] + (double)f[4]) * 4294967296.0));
    unsigned row[8];
    pack_row(f, 5, row);
    CHECK(row[4] == 0 && row[3] == kNever && row[0] == (unsigned)(T[0] - 1));
    // the packed draw is the rule's draw, at every threshold and next to it
    const float edge[5] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f};  // T = 0, 0, 2^32, 2^32
    uint64_t E[4];
    thresholds(edge, 5, E);
    CHECK(E[0] == 0 && E[1] == 0 && E[2] == 1ull << 32 && E[3] == 1ull << 32);
    unsigned erow[8];
    pack_row(edge, 5, erow);
    CHECK(erow[4] == 2);
    const unsigned probes[] = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (unsigned u : probes) {
        CHECK(draw(E, 5, u) == 2 && draw_packed(erow, 5, u) == 2);
        CHECK(draw(T, 5, u) == draw_packed(row, 5, u));
    }
    for (int s = 0; s < 3; ++s)
        for (int d = -1; d <= 1; ++d) {
            const unsigned u = (unsigned)(T[s] + d);
            CHECK(draw(T, 5, u) == draw_packed(row, 5, u));
            CHECK(draw(T, 5, u) == (unsigned)(s + (d >= 0)));
        }
    // random rows, protein included, random uniforms
    unsigned long long s = 88172645463325252ull;
    for (int it = 0; it < 2000; ++it) {
        const unsigned k = it & 1 ? 21 : 5;
        float g[21];
        for (unsigned i = 0; i < k; ++i)
            g[i] = rnd(s) % 4 == 0 ? 0.0f : (float)(rnd(s) % 1000) / 7.0f;
        g[rnd(s) % k] = 1.0f;
        uint64_t G[20];
        unsigned grow[24];
        thresholds(g, k, G);
        pack_row(g, k, grow);
        for (int q = 0; q < 50; ++q) {
            const unsigned u = q < 20 ? (unsigned)(G[q % (k - 1)] + (uint64_t)(q / 20)) : (unsigned)rnd(s);
            const unsigned x = draw(G, k, u);
            CHECK(x == draw_packed(grow, k, u));
            CHECK(x < k && g[x] > 0);  // a symbol without mass is never drawn
        }
    }
}

static void check_rows()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float ok[5] = {1, 0, 0, 0, 0}, zero[5] = {0, 0, 0, 0, 0}, neg[5] = {1, -1, 1, 1, 1}, bad[5] = {1, nan, 0, 0, 0};
    const float big[5] = {inf, 0, 0, 0, 0}, negzero[5] = {-0.0f, 0, 0, 0, 0};
    CHECK(row_valid(ok, 5) && !row_zero(ok, 5));
    CHECK(!row_valid(zero, 5) && row_zero(zero, 5));
    CHECK(!row_valid(neg, 5) && !row_zero(neg, 5));
    CHECK(!row_valid(bad, 5) && !row_zero(bad, 5));
    CHECK(!row_valid(big, 5) && !row_zero(big, 5));
    CHECK(!row_valid(negzero, 5) && row_zero(negzero, 5));
}

static Args args(char alphabet, const std::vector<uint64_t> &lengths, const float *f, size_t n_models, const float *t = nullptr,
                 size_t cols = 32)
{
    Args a;
    a.ctx = a.out = true;
    a.alphabet = alphabet;
    a.lengths = lengths.data(), a.n_records = lengths.size();
    a.frequencies = f, a.n_models = n_models;
    a.transitions = t;
    a.cols = cols;
    return a;
}

static void check_refusals_and_plan()
{
    const float f[5] = {0.3f, 0.2f, 0.15f, 0.35f, 0.0f};
    const std::vector<uint64_t> lengths = {0, 3, 0, 0, 5, 1, 0};
    std::string msg;
    Args a = args('D', lengths, f, 1);
    CHECK(check(a, &msg) == LM_HIP_OK);
    Args b = a;
    b.ctx = false;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && !msg.empty());
    b = a, b.out = false;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = a, b.frequencies = nullptr;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = a, b.lengths = nullptr;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b.n_records = 0, b.n_models = 1;
    CHECK(check(b, &msg) == LM_HIP_OK);  // null lengths with no records
    b = a, b.cols = 0;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = a, b.alphabet = 'X';
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = a, b.n_models = 2;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = a, b.n_models = 0;
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    float t[25] = {0};
    b = a, b.transitions = t, b.alphabet = 'P';
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);
    std::vector<float> per(lengths.size() * 5, 0.2f);
    b = args('D', lengths, per.data(), lengths.size(), t);
    CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS);

    // the offsets prefix, the live image, the shared row
    Plan p;
    CHECK(make_plan(a, &p, &msg) == LM_HIP_OK);
    const std::vector<uint64_t> want = {0, 0, 3, 3, 3, 8, 9, 9};
    CHECK(p.offsets == want && p.total == 9 && p.nrows == 1 && p.nlive == 3 && p.k == 5 && p.shared && !p.order1);
    CHECK(p.image.size() == 7 && p.dst()[0] == 0 && p.dst()[1] == 3 && p.dst()[2] == 8 && p.dst()[3] == 9);
    CHECK(p.record()[0] == 1 && p.record()[1] == 4 && p.record()[2] == 5);
    CHECK(p.rows.size() == 8);
    // per-record models: rows of live records only, an invalid row of an EMPTY record is no error, of a live one it is
    per[0] = -1.0f;                      // record 0 is empty
    Args c = args('D', lengths, per.data(), lengths.size());
    CHECK(make_plan(c, &p, &msg) == LM_HIP_OK && p.rows.size() == 3 * 8 && !p.shared);
    per[4 * 5 + 2] = std::numeric_limits<float>::quiet_NaN();
    CHECK(make_plan(c, &p, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("record 4") != std::string::npos);
    // an invalid shared row: an error with live records, none without
    const float zero[5] = {0, 0, 0, 0, 0};
    Args d = args('D', lengths, zero, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("row 0") != std::string::npos);
    const std::vector<uint64_t> empties = {0, 0, 0}, none;
    d = args('D', empties, zero, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_OK && p.nlive == 0 && p.total == 0 && p.offsets.size() == 4 && p.image.empty());
    d = args('P', none, zero, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_OK && p.offsets.size() == 1 && p.k == 21);
    // capacity: the sum passes 2^40, terms that would wrap 64 bits, and rows x columns past 2^40
    const std::vector<uint64_t> huge = {1ull << 39, 1ull << 39, 1}, wrap = {~0ull, ~0ull, 2}, edge = {1ull << 40};
    d = args('D', huge, f, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_ERR_CAPACITY && !msg.empty());
    d = args('D', wrap, f, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_ERR_CAPACITY);
    d = args('D', edge, f, 1);
    CHECK(make_plan(d, &p, &msg) == LM_HIP_OK && p.total == 1ull << 40 && p.nrows == 1ull << 35);
    const std::vector<uint64_t> pad = {(1ull << 40) - 1};
    d = args('D', pad, f, 1, nullptr, 7);  // ceil(total / 7) * 7 > 2^40
    CHECK(make_plan(d, &p, &msg) == LM_HIP_ERR_CAPACITY);

    // order 1: the zero row stands for `initial`, any other invalid row is an error -- once a record holds two symbols
    float tr[25] = {.1f, .2f, .3f, .4f, 0, .4f, .3f, .2f, .1f, 0, .25f, .25f, .25f, .25f, 0, .7f, .1f, .1f, .1f, 0, 0, 0, 0, 0, 0};
    Args m = args('D', lengths, f, 1, tr);
    CHECK(make_plan(m, &p, &msg) == LM_HIP_OK && p.order1 && p.rows.empty());
    for (unsigned s = 0; s < 8; ++s)
        CHECK(p.chain.row[5][s] == p.chain.row[0][s]);
    CHECK(p.chain.row[1][0] != p.chain.row[0][0]);
    tr[7] = -0.5f;
    CHECK(make_plan(m, &p, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("row 1") != std::string::npos);
    const std::vector<uint64_t> singles = {1, 0, 1};
    m = args('D', singles, f, 1, tr);
    CHECK(make_plan(m, &p, &msg) == LM_HIP_OK);  // no transition is taken
    m = args('D', lengths, zero, 1, tr);
    CHECK(make_plan(m, &p, &msg) == LM_HIP_ERR_BAD_ARGS);  // `initial` itself
}

static void check_small_vectors()
{
    const float f[5] = {0.3f, 0.2f, 0.15f, 0.35f, 0.0f};
    const uint8_t want[3][8] = {{3, 3, 2, 3, 3, 3, 1, 3}, {2, 0, 0, 0, 3, 3, 0, 0}, {1, 1, 3, 1, 0, 0, 3, 1}};
    const uint64_t seeds[3] = {1, 1, 2};
    const size_t records[3] = {0, 1, 0};
    const std::vector<uint64_t> lengths = {8, 8};
    std::string msg;
    Args a = args('D', lengths, f, 1);
    Plan p;
    CHECK(make_plan(a, &p, &msg) == LM_HIP_OK);
    for (int c = 0; c < 3; ++c) {
        const std::vector<uint8_t> got = host_record(a, p, seeds[c], 0, records[c]);
        CHECK(got.size() == 8);
        for (size_t j = 0; j < got.size(); ++j)
            CHECK(got[j] == want[c][j]);
    }
    // record_base shifts the record number
    const std::vector<uint8_t> shifted = host_record(a, p, 1, 1, 0);
    for (size_t j = 0; j < 8; ++j)
        CHECK(shifted[j] == want[1][j]);
}

static void check_maps()
{
    CHECK(map_compose(kIdentityMap, kIdentityMap) == kIdentityMap);
    for (unsigned x = 0; x < 5; ++x) {
        CHECK(map_apply(kIdentityMap, x) == x);
        for (unsigned a = 0; a < 5; ++a)
            CHECK(map_apply(map_constant(x), a) == x);
    }
    unsigned long long s = 2463534242ull;
    auto random_map = [&]() {
        unsigned m = 0;
        for (unsigned a = 0; a < 5; ++a)
            m |= (unsigned)(rnd(s) % 5) << (3 * a);
        return m;
    };
    for (int it = 0; it < 5000; ++it) {
        const unsigned f = random_map(), g = random_map(), h = random_map();
        const unsigned fg = map_compose(f, g);
        CHECK(fg < (1u << 15));
        for (unsigned a = 0; a < 5; ++a) {
            CHECK(map_apply(fg, a) == map_apply(g, map_apply(f, a)));
            CHECK(map_apply(map_compose(fg, h), a) == map_apply(map_compose(f, map_compose(g, h)), a));  // associative
        }
        // a constant map absorbs what stands in front of it: composition resets itself at a record start
        const unsigned c = map_constant((unsigned)(rnd(s) % 5));
        CHECK(map_compose(f, c) == c);
    }
    // a chain of steps composed equals the chain walked
    const float f[5] = {0.3f, 0.2f, 0.15f, 0.35f, 0.0f};
    const float tr[25] = {.1f, .2f, .3f, .4f, 0, .4f, .3f, .2f, .1f, 0, .25f, .25f, .25f, .25f, 0, .7f, .1f, .1f, .1f, 0, 0, 0, 0, 0, 0};
    const std::vector<uint64_t> lengths = {200};
    std::string msg;
    Args a = args('D', lengths, f, 1, tr);
    Plan p;
    CHECK(make_plan(a, &p, &msg) == LM_HIP_OK);
    const std::vector<uint8_t> text = host_record(a, p, 99, 0, 0);
    unsigned acc = kIdentityMap;
    for (uint64_t j = 0; j < 200; ++j) {
        unsigned u[4];
        uniforms(99, 0, j >> 2, u);
        acc = map_compose(acc, j ? markov_step(p.chain, u[j & 3]) : markov_first(p.chain, u[j & 3]));
        CHECK(map_apply(acc, 0) == text[(size_t)j] && map_apply(acc, 4) == text[(size_t)j]);
        CHECK(text[(size_t)j] < 4);
    }
}

int main()
{
    check_known_answers();
    check_thresholds();
    check_rows();
    check_refusals_and_plan();
    check_small_vectors();
    check_maps();
    if (failures) {
        std::fprintf(stderr, "test_sample_plan: %d checks failed\n", failures);
        return 1;
    }
    std::printf("test_sample_plan: all checks passed\n");
    return 0;
}
