// The host half of csrc/sites.hip alone (csrc/sites_plan.hpp: no HIP, no device): the window rule against 128-bit
// arithmetic, the argument checks, and the chunk plans and device images of random requests against what they must
// cover.  Needs nothing but a C++ compiler; meant to be built with -fsanitize=address,undefined as well.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sites_plan.hpp"

using namespace lm::sites;

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

static void check_window_rule()
{
    const unsigned long long edge[] = {0, 1, 2, 5, 9, 10, 11, 1ull << 31, 1ull << 32, (1ull << 62) - 1, 1ull << 62, (1ull << 63) - 1, 1ull << 63,
                                       (1ull << 63) + 1, ~0ull - 10, ~0ull - 1, ~0ull};
    const long long shifts[] = {0, 1, -1, 3, -3, 10, -10, 11, -11, 1ll << 62, -(1ll << 62), INT64_MAX, INT64_MIN, INT64_MIN + 1, INT64_MAX - 1};
    const unsigned long long lens[] = {0, 1, 10, 1ull << 33, (1ull << 63) - 1};
    for (unsigned long long len : lens)
        for (unsigned long long pos : edge)
            for (long long shift : shifts)
                for (unsigned long long width : edge) {
                    if (width == 0)
                        continue;
                    const __int128 start = (__int128)pos + (__int128)shift;
                    const bool want = start >= 0 && start + (__int128)width <= (__int128)len;
                    unsigned long long got_start = 12345;
                    const bool got = window_start(pos, shift, width, len, &got_start);
                    CHECK(got == want);
                    if (got && want)
                        CHECK((__int128)got_start == start);
                    if (!got)
                        CHECK(got_start == 12345);
                }
}

static void check_arguments()
{
    const size_t counts[] = {2, 0, 1}, widths[] = {3, 4, 2}, zero[] = {3, 0, 2};
    unsigned long long sites[6] = {0, 0, 0, 1, 1, 0};
    unsigned char out[64];
    Request r;
    r.counts = counts, r.widths = widths, r.n = 3, r.sites = sites, r.stride = 16, r.out = out, r.capacity = 8;
    Totals t;
    std::string msg;
    CHECK(check(r, 5, true, &t, &msg) == LM_HIP_OK && t.sites == 3 && t.window_bytes == 8 && t.width_sum == 9 && t.entries == 45);
    r.capacity = 7;
    CHECK(check(r, 5, true, &t, &msg) == LM_HIP_ERR_CAPACITY && !msg.empty());
    r.capacity = 44;
    CHECK(check(r, 5, false, &t, &msg) == LM_HIP_ERR_CAPACITY);
    r.capacity = 45;
    CHECK(check(r, 5, false, &t, &msg) == LM_HIP_OK);
    for (size_t stride : {0, 8, 15}) {
        Request b = r;
        b.stride = stride;
        CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    }
    Request b = r;
    b.widths = zero;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = r, b.counts = nullptr;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = r, b.widths = nullptr;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = r, b.sites = nullptr;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = r, b.out = nullptr;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_BAD_ARGS);
    b = Request();
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_OK && t.sites == 0);  // n == 0 needs nothing
    // sizes that overflow 64 bits are a capacity matter, whatever the capacity says
    const size_t huge_counts[] = {~(size_t)0 / 2, 3}, huge_widths[] = {3, ~(size_t)0 / 2};
    b = r, b.n = 2, b.counts = huge_counts, b.capacity = ~(size_t)0;
    CHECK(check(b, 5, true, &t, &msg) == LM_HIP_ERR_CAPACITY);
    b = r, b.n = 2, b.widths = huge_widths, b.capacity = ~(size_t)0;
    CHECK(check(b, 5, false, &t, &msg) == LM_HIP_ERR_CAPACITY);
}

// One random request: plan it, build every image, and account for every live site exactly once and in order.
static void check_plan(unsigned long long &seed, bool windows, size_t k)
{
    const size_t n = rnd(seed) % 9;
    std::vector<size_t> counts(n), widths(n);
    std::vector<int64_t> shifts(n);
    const size_t max_width = 1 + rnd(seed) % 4000;
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        counts[i] = rnd(seed) % 4 == 0 ? 0 : rnd(seed) % 700;
        widths[i] = rnd(seed) % 5 == 0 ? 1 + rnd(seed) % 5000 : 1 + rnd(seed) % 40;
        shifts[i] = (int64_t)(rnd(seed) % 7) - 3;
        total += counts[i];
    }
    const size_t stride = 16 + 8 * (rnd(seed) % 4);
    std::vector<unsigned char> raw(total * stride + 1, 0xEE);
    for (size_t s = 0; s < total; ++s) {
        const unsigned long long pair[2] = {s, ~(unsigned long long)s};  // every site is its own index
        memcpy(raw.data() + s * stride, pair, 16);
    }
    std::vector<unsigned char> out(1);
    Request r;
    r.counts = counts.data(), r.widths = widths.data(), r.shifts = rnd(seed) % 3 ? shifts.data() : nullptr, r.n = n;
    r.sites = raw.data(), r.stride = stride, r.out = out.data(), r.capacity = ~(size_t)0;
    Totals t;
    std::string msg;
    CHECK(check(r, k, windows, &t, &msg) == LM_HIP_OK && t.sites == total);
    const size_t site_chunk = rnd(seed) % 3 == 0 ? 0 : 1 + rnd(seed) % 300;
    const size_t block = rnd(seed) % 2 ? kBlockBytes : 64 + rnd(seed) % 20000;
    Plan p;
    make_plan(r, k, windows, max_width, site_chunk, block, &p);

    std::vector<unsigned long long> image;
    std::vector<Run> runs;
    size_t next_motif = 0, next_first = 0, live_sites = 0, covered_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool live = counts[i] && widths[i] <= max_width;
        CHECK((p.live[i] != kDead) == live);
        live_sites += live ? counts[i] : 0;
    }
    size_t seen = 0;
    for (const Chunk &c : p.chunks) {
        CHECK(c.seg1 > c.seg0 && c.sites > 0 && c.units > 0);
        CHECK(!site_chunk || c.sites <= site_chunk);
        size_t bytes = 0;
        build_image(r, p, c, &image);
        CHECK(image.size() == p.image_words(c) && image.size() <= p.max_image_words());
        const size_t nseg = c.seg1 - c.seg0;
        const unsigned long long *prefix = image.data(), *segs = prefix + nseg + 1, *sites = segs + nseg * kSegWords;
        CHECK(prefix[0] == 0 && prefix[nseg] == c.units && c.units <= p.max_units);
        size_t site0 = 0;
        for (size_t s = 0; s < nseg; ++s) {
            const Seg &g = p.segs[c.seg0 + s];
            const unsigned long long *w = segs + s * kSegWords;
            // in caller order, continuing where the last segment stopped
            while (next_motif < n && (p.live[next_motif] == kDead || next_first == counts[next_motif]))
                ++next_motif, next_first = 0;
            CHECK(g.motif == next_motif && g.first == next_first && g.count > 0);
            next_first += g.count;
            CHECK(next_first <= counts[g.motif]);
            CHECK(w[0] == site0 && w[1] == g.count && w[2] == widths[g.motif] && (long long)w[3] == (r.shifts ? shifts[g.motif] : 0));
            CHECK(w[5] == p.live[g.motif] && w[5] < p.nlive && w[4] == p.table[w[5]] && w[4] + widths[g.motif] * k <= p.live_entries);
            CHECK(prefix[s + 1] > prefix[s]);
            if (windows) {
                CHECK(prefix[s + 1] - prefix[s] == g.count * widths[g.motif]);
            } else {
                const bool direct = widths[g.motif] * k + 1 > kLdsCounters;
                CHECK(direct == c.direct && w[6] >= 1 && w[6] <= kGroupSites);
                CHECK(prefix[s + 1] - prefix[s] == (g.count + w[6] - 1) / w[6]);
                CHECK(direct || widths[g.motif] * k + 1 <= c.counters);
            }
            for (size_t j = 0; j < g.count; ++j) {
                const unsigned long long id = p.site_base[g.motif] + g.first + j;
                CHECK(sites[2 * (site0 + j)] == id && sites[2 * (site0 + j) + 1] == ~id);
            }
            site0 += g.count;
            bytes += g.count * (16 + (windows ? widths[g.motif] : 0));
        }
        CHECK(site0 == c.sites && c.sites <= p.max_sites);
        CHECK(bytes <= block || c.sites == 1);
        CHECK(windows || c.counters <= kLdsCounters);
        seen += c.sites;
        if (windows) {
            window_runs(r, p, c, &runs);
            size_t run_sites = 0;
            for (const Run &x : runs) {
                CHECK(x.dev_byte + x.bytes <= c.units && x.dev_site + x.sites <= c.sites && x.host_byte + x.bytes <= t.window_bytes);
                CHECK(x.host_site + x.sites <= total);
                run_sites += x.sites;
                covered_bytes += x.bytes;
            }
            CHECK(run_sites == c.sites);
        }
    }
    CHECK(seen == live_sites);
    if (windows) {
        size_t live_bytes = 0;
        for (size_t i = 0; i < n; ++i)
            live_bytes += p.live[i] != kDead ? counts[i] * widths[i] : 0;
        CHECK(covered_bytes == live_bytes);
    }
}

int main()
{
    check_window_rule();
    check_arguments();
    unsigned long long seed = 0x9E3779B97F4A7C15ull;
    for (int round = 0; round < 400; ++round) {
        check_plan(seed, true, 5);
        check_plan(seed, false, 5);
        check_plan(seed, false, 21);
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_sites_plan: all checks passed\n");
    return 0;
}
