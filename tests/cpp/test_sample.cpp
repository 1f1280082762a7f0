// A null set through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): SequenceSet::sample against the rule
// walked on the host (csrc/sample_plan.hpp: host_record, itself held to the rule's known answers by test_sample_plan.cpp),
// and SequenceSet::count_pairs against a plain loop.
#include <cstdio>
#include <string>
#include <vector>

#include "lightmotif_hip.hpp"
#include "sample_plan.hpp"

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
void check_set(const Pipeline<A> &pli, const std::vector<uint64_t> &lengths, const std::vector<float> &f, const std::vector<float> *t,
               uint64_t seed, uint64_t base)
{
    SequenceSet<A> got = SequenceSet<A>::sample(pli, lengths, f, t, seed, base);
    lm::sample::Args a;
    a.ctx = a.out = true;
    a.alphabet = A::code;
    a.lengths = lengths.data(), a.n_records = lengths.size();
    a.frequencies = f.data(), a.n_models = f.size() == A::K ? 1 : lengths.size();
    a.transitions = t ? t->data() : nullptr;
    a.cols = 32;
    lm::sample::Plan p;
    std::string msg;
    CHECK(lm::sample::make_plan(a, &p, &msg) == LM_HIP_OK);
    CHECK(got.records() == lengths.size() && got.columns() == 32 && got.wrap() == 0);
    std::vector<uint64_t> pairs(A::K * A::K, 0);
    for (size_t i = 0; i < lengths.size(); ++i) {
        const std::vector<uint8_t> want = lm::sample::host_record(a, p, seed, base, i);
        CHECK(got.len(i) == want.size());
        if (got.len(i) == want.size() && !want.empty())
            CHECK(got.record(i).data == want);
        for (size_t j = 0; j + 1 < want.size(); ++j)
            ++pairs[want[j] * A::K + want[j + 1]];
    }
    CHECK(got.count_pairs() == pairs);
}

}  // namespace

int main()
{
    try {
        const std::vector<uint64_t> lengths = {0, 1, 17, 0, 4097, 5, 300};
        const std::vector<float> f = {0.3f, 0.2f, 0.15f, 0.35f, 0.0f};
        const std::vector<float> t = {.1f, .2f, .3f, .4f, 0, .4f, .3f, .2f, .1f, 0, .25f, .25f, .25f, .25f, 0, .7f, .1f, .1f, .1f, 0, 0, 0, 0, 0, 0};
        Pipeline<Dna> dna = Pipeline<Dna>::hip();
        check_set<Dna>(dna, lengths, f, nullptr, 1, 0);
        check_set<Dna>(dna, lengths, f, &t, 99, (1ull << 32) - 3);
        std::vector<float> per;
        for (size_t i = 0; i < lengths.size(); ++i)
            for (unsigned s = 0; s < 5; ++s)
                per.push_back((float)((i + s) % 4 + (s == 4 ? 0 : 1)));
        check_set<Dna>(dna, lengths, per, nullptr, 5, 11);
        Pipeline<Protein> protein = Pipeline<Protein>::hip();
        std::vector<float> g(21, 0.05f);
        g[20] = 0.0f;
        check_set<Protein>(protein, lengths, g, nullptr, 7, 0);
        bool threw = false;
        try {
            SequenceSet<Protein>::sample(protein, lengths, g, &t);  // 25 entries are no 21 x 21 table
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            SequenceSet<Dna>::sample(dna, lengths, {0, 0, 0, 0, 0});  // no model
        } catch (const std::runtime_error &) {
            threw = true;
        }
        CHECK(threw);
    } catch (const UnsupportedBackend &e) {
        std::fprintf(stderr, "UnsupportedBackend: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_sample: all checks passed\n");
    return 0;
}
