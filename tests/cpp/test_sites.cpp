// Hit windows through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): SequenceSet::windows, count_sites and
// record against plain slices of the host's records (seq.rs:433-442, pwm/mod.rs:209-237, 313-321).
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

template <class A>
void check_alphabet(unsigned seed)
{
    using Site = typename SequenceSet<A>::Site;
    Pipeline<A> pli = Pipeline<A>::hip();
    std::vector<std::string> texts = {"", random_text<A>(1, seed), random_text<A>(70001, seed), ""};
    for (size_t r = 0; r < 40; ++r)
        texts.push_back(random_text<A>(r % 9, seed));
    std::vector<EncodedSequence<A>> records;
    for (const std::string &t : texts)
        records.push_back(EncodedSequence<A>::encode(t));
    SequenceSet<A> set = pli.stripe_set(records);

    // three motifs, the middle one without a site; sites past the end, in a record that does not exist, moved by the shift
    const std::vector<size_t> widths = {4, 7, 600};
    const std::vector<int64_t> shifts = {-1, 0, 2};
    std::vector<std::vector<Site>> sites(3);
    for (size_t i = 0; i < 500; ++i) {
        seed = seed * 1664525u + 1013904223u;
        const size_t r = (seed >> 8) % (records.size() + 1);
        const size_t len = r < records.size() ? records[r].len() : 0;
        sites[i % 2 ? 0 : 2].push_back(Site{r, (size_t)((seed >> 3) % (len + 3))});
    }
    sites[0].push_back(Site{2, ~(size_t)0});
    for (int pass = 0; pass < 2; ++pass) {
        const auto got = set.windows(sites, widths, shifts);
        const auto counted = set.count_sites(sites, widths, shifts);
        CHECK(got.size() == 3 && counted.tables.size() == 3 && counted.used.size() == 3);
        for (size_t i = 0; i < 3; ++i) {
            const size_t w = widths[i];
            std::vector<uint64_t> table(w * A::K, 0);
            uint64_t used = 0;
            CHECK(got[i].symbols.size() == sites[i].size() * w && got[i].valid.size() == sites[i].size());
            for (size_t s = 0; s < sites[i].size(); ++s) {
                const Site &x = sites[i][s];
                const __int128 start = (__int128)x.position + shifts[i];
                const bool valid = x.record < records.size() && start >= 0 && start + (__int128)w <= (__int128)records[x.record].len();
                CHECK((got[i].valid[s] != 0) == valid);
                for (size_t j = 0; j < w; ++j) {
                    const uint8_t want = valid ? records[x.record].data[(size_t)start + j] : 0xFF;
                    if (got[i].symbols[s * w + j] != want) {
                        CHECK(got[i].symbols[s * w + j] == want);
                        break;
                    }
                    if (valid)
                        ++table[j * A::K + want];
                }
                used += valid;
            }
            CHECK(counted.tables[i] == table && counted.used[i] == used);
            const CountMatrix<A> m = CountMatrix<A>::from_table(counted.tables[i]);
            CHECK(m.data.rows() == w && (w == 0 || m.data(0, 0) == table[0]));
        }
        CHECK(sites[1].empty() && counted.used[1] == 0);
        set.configure_wrap(50);   // wrap rows are never read
    }
    for (size_t r : {(size_t)0, (size_t)1, (size_t)2, (size_t)7})
        CHECK(set.record(r).data == records[r].data);
    bool threw = false;
    try {
        set.windows(sites, {4, 7});
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
}

}  // namespace

int main()
{
    // (needs no device) pwm/mod.rs:313-321 on a table, and the u32 of a CountMatrix
    const std::vector<uint64_t> table = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    const CountMatrix<Dna> m = CountMatrix<Dna>::from_table(table), rc = m.reverse_complement();
    const uint32_t want[2][5] = {{8, 9, 6, 7, 10}, {3, 4, 1, 2, 5}};
    for (size_t i = 0; i < 2; ++i)
        for (size_t s = 0; s < 5; ++s) {
            CHECK(rc.data(i, s) == want[i][s]);
            CHECK(rc.reverse_complement().data(i, s) == m.data(i, s));
        }
    bool threw = false;
    try {
        CountMatrix<Dna>::from_table({0, 0, 0, 0, 1ull << 32});
    } catch (const std::overflow_error &) {
        threw = true;
    }
    CHECK(threw);
    try {
        check_alphabet<Dna>(1u);
        check_alphabet<Protein>(2u);
    } catch (const UnsupportedBackend &e) {
        std::fprintf(stderr, "UnsupportedBackend: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_sites: all checks passed\n");
    return 0;
}
