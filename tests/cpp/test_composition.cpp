// Symbol counts through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): StripedSequence::count_symbols,
// SequenceSet::count_symbols and background_from_counts against a plain loop over the host symbols
// (seq.rs:444-483, abc.rs:389-456).
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
        const unsigned r = (seed >> 8) % 100u;
        // skewed: the first symbol takes 40 %, the default symbol 3 %
        s[i] = r < 3 ? A::symbols()[A::K - 1] : r < 43 ? A::symbols()[0] : A::symbols()[1 + (seed >> 16) % (A::K - 2)];
    }
    return s;
}

template <class A>
std::vector<uint64_t> plain_counts(const std::string &text)
{
    const EncodedSequence<A> enc = EncodedSequence<A>::encode(text);
    std::vector<uint64_t> out(A::K, 0);
    for (uint8_t s : enc.data)
        ++out[s];
    return out;
}

template <class A>
void check_alphabet(unsigned seed)
{
    Pipeline<A> pli = Pipeline<A>::hip();
    for (const size_t n : {(size_t)1, (size_t)33, (size_t)1025, (size_t)70001}) {
        const std::string text = random_text<A>(n, seed);
        StripedSequence<A> seq = pli.stripe(pli.encode(text));
        const std::vector<uint64_t> want = plain_counts<A>(text);
        CHECK(seq.count_symbols() == want);
        seq.configure_wrap(9);
        CHECK(seq.count_symbols() == want);
    }
    // a set: empty records at both ends and in the middle, one long record, many short ones
    std::vector<std::string> records = {"", random_text<A>(1, seed), "", "", random_text<A>(40000, seed)};
    for (size_t r = 0; r < 300; ++r)
        records.push_back(random_text<A>(r % 7, seed));
    records.push_back("");
    std::vector<uint64_t> want, all(A::K, 0);
    for (const std::string &r : records) {
        const std::vector<uint64_t> c = plain_counts<A>(r);
        want.insert(want.end(), c.begin(), c.end());
        for (size_t s = 0; s < A::K; ++s)
            all[s] += c[s];
    }
    const SequenceSet<A> set = pli.stripe_set(records);
    const std::vector<uint64_t> got = set.count_symbols();
    CHECK(got == want);
    CHECK(pli.stripe_set(std::vector<std::string>{}).count_symbols().empty());

    // Background::from_counts of the table = of its column sums; the default symbol leaves the total unless asked for
    const std::vector<float> bg = background_from_counts<A>(got), bg_sum = background_from_counts<A>(all);
    CHECK(bg.size() == A::K && std::memcmp(bg.data(), bg_sum.data(), A::K * sizeof(float)) == 0);
    uint64_t known = 0;
    for (size_t s = 0; s + 1 < A::K; ++s)
        known += all[s];
    for (size_t s = 0; s + 1 < A::K; ++s)
        CHECK(bg[s] == (float)all[s] / (float)known);
    CHECK(bg[A::K - 1] == 0.0f && all[A::K - 1] > 0);
    const std::vector<float> bg_n = background_from_counts<A>(got, true);
    CHECK(bg_n[A::K - 1] == (float)all[A::K - 1] / (float)(known + all[A::K - 1]));
    bool threw = false;
    try {
        std::vector<uint64_t> only_default(A::K, 0);
        only_default[A::K - 1] = 5;
        background_from_counts<A>(only_default);
    } catch (const InvalidData &) {
        threw = true;
    }
    CHECK(threw);
}

}  // namespace

int main()
{
    // (needs no device) abc.rs:382-387
    const std::vector<float> doc = background_from_counts<Dna>({2, 2, 5, 1, 0});
    CHECK(doc == std::vector<float>({0.2f, 0.2f, 0.5f, 0.1f, 0.0f}));
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
    std::printf("test_composition: all checks passed\n");
    return 0;
}
