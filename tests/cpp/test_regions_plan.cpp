// The host half of csrc/regions.hip alone (csrc/regions_plan.hpp: no HIP, no device): the clipping rule against 128-bit
// arithmetic, the argument checks, the offsets prefix, the capacity refusal and the device image of random requests
// against plain slices.  Needs nothing but a C++ compiler; meant to be built with -fsanitize=address,undefined as well.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "regions_plan.hpp"

using namespace lm::regions;

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

static lm_hip_region region(size_t record, int64_t start, int64_t end, uint8_t strand = 0)
{
    lm_hip_region r{};
    r.record = record, r.start = start, r.end = end, r.strand = strand;
    return r;
}

static void check_clip_rule()
{
    const int64_t edge[] = {INT64_MIN, INT64_MIN + 1, -(1ll << 62), -11, -10, -1, 0, 1, 2, 9, 10, 11, 1ll << 31, 1ll << 32, 1ll << 40,
                            (1ll << 62), INT64_MAX - 1, INT64_MAX};
    const uint64_t lens[] = {0, 1, 10, 1ull << 33, (1ull << 63) - 1, 1ull << 63, ~0ull};
    for (uint64_t len : lens)
        for (int64_t start : edge)
            for (int64_t end : edge) {
                const __int128 s = start < 0 ? 0 : (__int128)start;
                const __int128 e = (__int128)end < (__int128)len ? (__int128)end : (__int128)len;
                const bool want = s < e;
                uint64_t gs = 12345, ge = 54321;
                const bool got = clip(start, end, len, &gs, &ge);
                CHECK(got == want);
                if (want)
                    CHECK((__int128)gs == s && (__int128)ge == e);
                else
                    CHECK(gs == 0 && ge == 0);
            }
    for (unsigned b = 0; b < 256; ++b) {
        const uint8_t want = b == 0 ? 2 : b == 2 ? 0 : b == 1 ? 3 : b == 3 ? 1 : (uint8_t)b;  // abc.rs:174-185
        CHECK(complement((uint8_t)b) == want);
    }
}

static void check_arguments()
{
    const lm_hip_region two[] = {region(0, 0, 4), region(1, 2, 3, 1)};
    Args a;
    a.ctx = a.src = a.out = true;
    a.k = 5, a.regions = two, a.n = 2;
    std::string msg;
    CHECK(check(a, &msg) == LM_HIP_OK);
    for (int which = 0; which < 3; ++which) {  // a null ctx, src, out
        Args b = a;
        (which == 0 ? b.ctx : which == 1 ? b.src : b.out) = false;
        msg.clear();
        CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && !msg.empty());
    }
    {
        Args b = a;
        b.regions = nullptr;  // null regions with n > 0
        msg.clear();
        CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && !msg.empty());
        b.n = 0;              // ... and with n == 0: fine
        CHECK(check(b, &msg) == LM_HIP_OK);
    }
    for (unsigned strand : {2u, 3u, 43u, 45u, 255u}) {  // ('+' and '-' are not strands either)
        lm_hip_region bad[] = {region(0, 0, 4), region(0, 0, 4, (uint8_t)strand)};
        Args b = a;
        b.regions = bad;
        msg.clear();
        CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("region 1") != std::string::npos);
    }
    {
        Args b = a;
        b.k = 21;  // the reverse complement of a protein set
        msg.clear();
        CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("region 1") != std::string::npos);
        b.n = 1;   // strand 0 alone is fine there
        CHECK(check(b, &msg) == LM_HIP_OK);
    }
    {
        Args b = a;
        b.src_device = 1;  // a set on another device than the context
        msg.clear();
        CHECK(check(b, &msg) == LM_HIP_ERR_BAD_ARGS && msg.find("device") != std::string::npos);
    }
}

static void check_edges()
{
    // records of 0, 10, 0 and 7 symbols
    const uint64_t off[] = {0, 0, 10, 10, 17};
    const lm_hip_region regs[] = {
        region(1, INT64_MIN, INT64_MAX),     // the whole record, from both extremes
        region(1, -5, 3),                    // clipped at the front
        region(1, 8, 100, 1),                // clipped at the back
        region(1, 5, 5),                     // start == end
        region(1, 7, 2),                     // start > end
        region(1, INT64_MAX, INT64_MIN),     // ... at the extremes
        region(1, 10, 20),                   // wholly behind the record
        region(1, -20, 0),                   // wholly in front of it
        region(4, 0, 5),                     // one past the last record
        region(~(size_t)0, 0, 5),
        region(0, 0, 5),                     // empty source records
        region(2, INT64_MIN, INT64_MAX, 1),
        region(3, 6, 7),                     // the last symbol of the last record
        region(3, 0, 7, 1),
    };
    const size_t n = sizeof regs / sizeof regs[0];
    const uint64_t want[][2] = {{0, 10}, {0, 3}, {8, 10}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {6, 7}, {0, 7}};
    std::vector<lm_hip_region_span> taken(n, lm_hip_region_span{99, 99});
    Plan p;
    std::string msg;
    CHECK(make_plan(off, 4, 32, regs, n, taken.data(), &p, &msg) == LM_HIP_OK);
    CHECK(p.offsets.size() == n + 1 && p.offsets[0] == 0);
    uint64_t sum = 0;
    size_t live = 0;
    for (size_t i = 0; i < n; ++i) {
        CHECK(taken[i].start == want[i][0] && taken[i].end == want[i][1]);
        CHECK(p.offsets[i] == sum);
        sum += want[i][1] - want[i][0];
        live += want[i][1] > want[i][0];
    }
    CHECK(p.offsets[n] == sum && p.total == sum && p.rows == (sum + 31) / 32);
    CHECK(p.nlive == live && live == 5 && p.image.size() == live + 1 + live * kLiveWords);
    // the image: whole record | front | back (minus) | last symbol | last record (minus)
    const unsigned long long dst[] = {0, 10, 13, 15, 16, 23}, src[] = {0, 0, 8, 16, 10}, strand[] = {0, 0, 1, 0, 1};
    for (size_t j = 0; j < live; ++j)
        CHECK(p.dst()[j] == dst[j] && p.live(j)[0] == src[j] && p.live(j)[1] == strand[j]);
    CHECK(p.dst()[live] == dst[live]);
    // no taken table; no regions; nothing but empty regions
    CHECK(make_plan(off, 4, 32, regs, n, nullptr, &p, &msg) == LM_HIP_OK && p.total == sum);
    CHECK(make_plan(off, 4, 32, nullptr, 0, nullptr, &p, &msg) == LM_HIP_OK);
    CHECK(p.offsets.size() == 1 && p.offsets[0] == 0 && p.nlive == 0 && p.image.empty() && p.total == 0 && p.rows == 0);
    CHECK(make_plan(off, 4, 32, regs + 3, 9, taken.data(), &p, &msg) == LM_HIP_OK);
    CHECK(p.offsets == std::vector<uint64_t>(10, 0) && p.nlive == 0 && p.image.empty() && p.rows == 0);
    // a source without records
    const uint64_t none[] = {0};
    CHECK(make_plan(none, 0, 32, regs, n, taken.data(), &p, &msg) == LM_HIP_OK && p.total == 0 && p.nlive == 0);
}

// 2^40 cells: fabricated offsets, nothing of that size is allocated
static void check_capacity()
{
    const uint64_t off[] = {0, 1ull << 39, (1ull << 39) + 5, (1ull << 63) + 5};
    Plan p;
    std::string msg;
    const lm_hip_region two[] = {region(0, 0, INT64_MAX), region(0, 0, INT64_MAX, 1)};
    CHECK(make_plan(off, 3, 32, two, 2, nullptr, &p, &msg) == LM_HIP_OK && p.total == 1ull << 40 && p.rows == 1ull << 35);
    CHECK(make_plan(off, 3, 1, two, 2, nullptr, &p, &msg) == LM_HIP_OK && p.rows == 1ull << 40);
    const lm_hip_region more[] = {region(0, 0, INT64_MAX), region(0, 0, INT64_MAX), region(1, 0, 1)};  // 2^40 + 1
    msg.clear();
    CHECK(make_plan(off, 3, 32, more, 3, nullptr, &p, &msg) == LM_HIP_ERR_CAPACITY && !msg.empty());
    CHECK(make_plan(off, 3, 1, more, 3, nullptr, &p, &msg) == LM_HIP_ERR_CAPACITY);
    // columns that do not divide: 2^40 - 1 symbols are 3 full columns' worth, but at 7 columns their last row passes 2^40 cells
    const lm_hip_region odd[] = {region(0, 0, INT64_MAX), region(0, 1, INT64_MAX)};
    CHECK(make_plan(off, 3, 32, odd, 2, nullptr, &p, &msg) == LM_HIP_OK && p.total == (1ull << 40) - 1);
    CHECK(make_plan(off, 3, 3, odd, 2, nullptr, &p, &msg) == LM_HIP_OK);
    CHECK(make_plan(off, 3, 7, odd, 2, nullptr, &p, &msg) == LM_HIP_ERR_CAPACITY);
    // one region of 2^63 symbols, many times: the sum is refused long before it wraps
    std::vector<lm_hip_region> huge(64, region(2, 0, INT64_MAX));
    std::vector<lm_hip_region_span> taken(64);
    CHECK(make_plan(off, 3, 32, huge.data(), huge.size(), taken.data(), &p, &msg) == LM_HIP_ERR_CAPACITY);
    CHECK(taken[0].start == 0 && taken[0].end == off[3] - off[2]);
}

// random requests against plain slices of host records
static void check_random()
{
    unsigned long long seed = 0x9E3779B97F4A7C15ull;
    for (int round = 0; round < 200; ++round) {
        const size_t records = rnd(seed) % 6;
        std::vector<uint64_t> off(records + 1, 0);
        std::vector<uint8_t> text;
        for (size_t r = 0; r < records; ++r) {
            const size_t len = rnd(seed) % 4 ? rnd(seed) % 60 : 0;
            for (size_t i = 0; i < len; ++i)
                text.push_back((uint8_t)(rnd(seed) % 5));
            off[r + 1] = text.size();
        }
        const size_t n = rnd(seed) % 40, cols = 1 + rnd(seed) % 40;
        std::vector<lm_hip_region> regs;
        for (size_t i = 0; i < n; ++i)
            regs.push_back(region(rnd(seed) % (records + 2), (int64_t)(rnd(seed) % 90) - 15, (int64_t)(rnd(seed) % 90) - 15, rnd(seed) % 2));
        std::vector<lm_hip_region_span> taken(n);
        Plan p;
        std::string msg;
        CHECK(make_plan(off.data(), records, cols, regs.data(), n, taken.data(), &p, &msg) == LM_HIP_OK);
        // the joined text by the rule ...
        std::vector<uint8_t> want;
        for (size_t i = 0; i < n; ++i) {
            CHECK(p.offsets[i] == want.size());
            if (regs[i].record >= records)
                continue;
            const int64_t len = (int64_t)(off[regs[i].record + 1] - off[regs[i].record]);
            const int64_t s = regs[i].start < 0 ? 0 : regs[i].start, e = regs[i].end > len ? len : regs[i].end;
            if (s >= e) {
                CHECK(taken[i].start == 0 && taken[i].end == 0);
                continue;
            }
            CHECK(taken[i].start == (uint64_t)s && taken[i].end == (uint64_t)e);
            const uint8_t *rec = text.data() + off[regs[i].record];
            for (int64_t j = 0; j < e - s; ++j)
                want.push_back(regs[i].strand ? complement(rec[e - 1 - j]) : rec[s + j]);
        }
        CHECK(p.offsets[n] == want.size() && p.total == want.size() && p.rows == (want.size() + cols - 1) / cols);
        // ... and as the image describes it, byte by byte as the kernel reads it
        std::vector<uint8_t> got(want.size(), 0xEE);
        for (size_t j = 0; j < p.nlive; ++j) {
            const unsigned long long d0 = p.dst()[j], d1 = p.dst()[j + 1], src = p.live(j)[0];
            CHECK(d0 < d1 && d1 <= want.size() && src + (d1 - d0) <= text.size());
            for (unsigned long long d = d0; d < d1 && d < got.size(); ++d)
                got[d] = p.live(j)[1] ? complement(text[src + (d1 - d0 - 1 - (d - d0))]) : text[src + (d - d0)];
        }
        if (p.nlive)
            CHECK(p.dst()[0] == 0 && p.dst()[p.nlive] == want.size());
        CHECK(got == want);
    }
}

int main()
{
    check_clip_rule();
    check_arguments();
    check_edges();
    check_capacity();
    check_random();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_regions_plan: all checks passed\n");
    return 0;
}
