// The device's FASTA reader through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp):
// SequenceSet::from_fasta against Pipeline::stripe_set of the same records, by record lengths, header spans and the hits of
// a one-row matrix at a threshold every position passes (the list is the sequence).
#include <cstdio>
#include <limits>
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

int main()
{
    try {
        Pipeline<Dna> pli = Pipeline<Dna>::hip();
        const std::vector<std::string> names = {"one first", "two", "", "four\r"};
        const std::vector<std::string> records = {"ACGTNACGTTGCA", "", "GGGTTTAAAC?CC", "AC"};
        std::string text = "text before the first header\nACGT\n";
        std::vector<size_t> begins;
        for (size_t r = 0; r < records.size(); ++r) {
            text += ">";
            begins.push_back(text.size());
            text += names[r] + "\n";
            for (size_t i = 0; i < records[r].size(); i += 5)
                text += records[r].substr(i, 5) + (r == 3 ? "\r\n" : "\n");
        }
        auto got = SequenceSet<Dna>::from_fasta(pli, text.data(), text.size(), true);
        auto want = pli.stripe_set(records, true);
        CHECK(got.records() == records.size() && got.total_length() == want.total_length() && got.rows() == want.rows());
        CHECK(got.lengths() == want.lengths());
        CHECK(got.header_spans().size() == records.size() && want.header_spans().empty());
        for (size_t r = 0; r < got.header_spans().size() && r < records.size(); ++r) {
            const lm_hip_fasta_span s = got.header_spans()[r];
            CHECK(s.begin == begins[r] && s.end == begins[r] + names[r].size());
            CHECK(text.substr(s.begin, s.end - s.begin) == names[r]);
        }

        DenseMatrix<float> w(1, Dna::K);
        for (size_t s = 0; s < Dna::K; ++s)
            w(0, s) = float(s + 1);
        const ScoringMatrix<Dna> pssm(std::vector<float>(Dna::K, 0.25f), w);
        got.configure_wrap(1);
        want.configure_wrap(1);
        const float all = -std::numeric_limits<float>::infinity();
        const auto a = pli.scan_threshold({&pssm}, {all}, got), b = pli.scan_threshold({&pssm}, {all}, want);
        CHECK(a.size() == 1 && b.size() == 1 && a[0].size() == b[0].size() && a[0].size() == want.total_length());
        for (size_t i = 0; a.size() == 1 && b.size() == 1 && i < a[0].size() && i < b[0].size(); ++i)
            CHECK(a[0][i].record == b[0][i].record && a[0][i].position == b[0][i].position && a[0][i].score == b[0][i].score);

        // strict mode names the residue's place; no header line, no records
        bool threw = false;
        try {
            SequenceSet<Dna>::from_fasta(pli, text.data(), text.size());
        } catch (const InvalidSymbol &e) {
            threw = e.record == 2 && e.index == 10;
        }
        CHECK(threw);
        const std::string junk = "ACGT\nACGT\n";
        CHECK(SequenceSet<Dna>::from_fasta(pli, junk.data(), junk.size(), true).records() == 0);
        CHECK(SequenceSet<Dna>::from_fasta(pli, nullptr, 0).records() == 0);
    } catch (const UnsupportedBackend &e) {
        std::fprintf(stderr, "UnsupportedBackend: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("test_fasta: all checks passed\n");
    return 0;
}
