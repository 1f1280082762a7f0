// A derived set through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): SequenceSet::regions against plain
// slices of the host's records -- rec[s:e], or the complement (abc.rs:174-185) of rec[s:e] reversed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lightmotif_hip.hpp"

using namespace lightmotif;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

namespace {

template <class A>
std::string random_text(size_t n, unsigned &seed)
{
    std::string s(n, 'N');
    for (size_t i = 0; i < n; ++i) {
        seed = seed * 1664525u + 1013904223u;
        s[i] = A::symbols()[(seed >> 12) % A::K];
    }
    return s;
}

lm_hip_region region(size_t record, int64_t start, int64_t end, uint8_t strand)
{
    lm_hip_region r{};
    r.record = record, r.start = start, r.end = end, r.strand = strand;
    return r;
}

template <class A>
void check_alphabet(unsigned seed, bool both_strands)
{
    Pipeline<A> pli = Pipeline<A>::hip();
    std::vector<std::string> texts = {"", random_text<A>(1, seed), random_text<A>(5003, seed), "", random_text<A>(97, seed)};
    std::vector<EncodedSequence<A>> records;
    for (const std::string &t : texts)
        records.push_back(EncodedSequence<A>::encode(t));
    SequenceSet<A> set = pli.stripe_set(records);

    std::vector<lm_hip_region> regs = {region(2, INT64_MIN, INT64_MAX, 0), region(5, 0, 10, 0), region(2, 10, 10, 0),
                                       region(4, -3, 200, 0), region(0, 0, 5, 0), region(1, 0, 1, 0)};
    for (size_t i = 0; i < 400; ++i) {
        seed = seed * 1664525u + 1013904223u;
        const size_t r = (seed >> 8) % (records.size() + 1);
        const int64_t len = r < records.size() ? (int64_t)records[r].len() : 0;
        const int64_t s = (int64_t)((seed >> 3) % (unsigned)(len + 7)) - 3;
        seed = seed * 1664525u + 1013904223u;
        regs.push_back(region(r, s, s + (int64_t)((seed >> 5) % 70) - 2, both_strands ? (seed >> 20) & 1 : 0));
    }
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<lm_hip_region_span> taken;
        SequenceSet<A> got = set.regions(regs, &taken);
        CHECK(got.records() == regs.size() && taken.size() == regs.size());
        CHECK(got.columns() == set.columns() && got.wrap() == 0);
        size_t total = 0;
        for (size_t i = 0; i < regs.size(); ++i) {
            const lm_hip_region &x = regs[i];
            std::vector<uint8_t> want;
            uint64_t s = 0, e = 0;
            if (x.record < records.size()) {
                const int64_t len = (int64_t)records[x.record].len();
                const int64_t a = x.start < 0 ? 0 : x.start, b = x.end > len ? len : x.end;
                if (a < b) {
                    s = (uint64_t)a, e = (uint64_t)b;
                    for (uint64_t j = 0; j < e - s; ++j) {
                        const uint8_t v = records[x.record].data[x.strand ? e - 1 - j : s + j];
                        want.push_back(x.strand && v < 4 ? v ^ 2 : v);
                    }
                }
            }
            CHECK(taken[i].start == s && taken[i].end == e);
            CHECK(got.len(i) == want.size());
            if (got.len(i) == want.size())
                CHECK(got.record(i).data == want);
            total += want.size();
        }
        CHECK(got.total_length() == total);
        set.configure_wrap(40);   // wrap rows of the source are never read
    }
    // no regions: a set of no records; no taken table
    SequenceSet<A> none = set.regions({});
    CHECK(none.records() == 0 && none.total_length() == 0);
    bool threw = false;
    try {
        set.regions({region(1, 0, 1, 2)});
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        set.regions({region(1, 0, 1, 1)});
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw == (A::K != 5));   // the reverse complement is DNA's
}

}  // namespace

int main()
{
    try {
        check_alphabet<Dna>(1u, true);
        check_alphabet<Protein>(2u, false);
    } catch (const UnsupportedBackend &e) {
        std::fprintf(stderr, "UnsupportedBackend: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_regions: all checks passed\n");
    return 0;
}
