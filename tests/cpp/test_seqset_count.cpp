// The hit counts per record through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): Pipeline::scan_count
// over the planted edge records of tests/seqset_best_cases.py.  The case file is written by
// tests/test_cpp_seqset_count.py:
//   line 1     the consensus (the matrix: +2 for the consensus base, -2 for the others, +2 for N)
//   line 2     the number of records, the number of levels, then the bit patterns of the levels' thresholds
//   then per record one line `text count_0 ... count_{levels-1}` with the values Python's scan_count_set gave
//   (an empty record's text is `-`).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
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

int main(int argc, char **argv)
{
    try {
        Pipeline<Dna> pli = Pipeline<Dna>::hip();
        if (argc < 2) {
            std::fprintf(stderr, "usage: test_seqset_count CASE_FILE\n");
            return 3;
        }
        std::ifstream in(argv[1]);
        std::string consensus;
        size_t n = 0, levels = 0;
        in >> consensus >> n >> levels;
        std::vector<float> thresholds(levels);
        for (size_t l = 0; l < levels; ++l) {
            uint32_t bits = 0;
            in >> bits;
            std::memcpy(&thresholds[l], &bits, 4);
        }
        std::vector<std::string> records(n);
        std::vector<std::vector<uint32_t>> want(levels, std::vector<uint32_t>(n));
        for (size_t r = 0; r < n; ++r) {
            in >> records[r];
            for (size_t l = 0; l < levels; ++l)
                in >> want[l][r];
            if (records[r] == "-")
                records[r].clear();
        }
        CHECK(bool(in) && n > 0 && levels > 0 && !consensus.empty());

        const size_t m = consensus.size();
        DenseMatrix<float> w(m, Dna::K);
        for (size_t j = 0; j < m; ++j)
            for (size_t s = 0; s < Dna::K; ++s)
                w(j, s) = (s == 4 || Dna::symbols()[s] == consensus[j]) ? 2.0f : -2.0f;
        const ScoringMatrix<Dna> pssm(std::vector<float>(Dna::K, 0.25f), w);

        auto set = pli.stripe_set(records);
        set.configure_wrap(m);
        const auto got = pli.scan_count({&pssm}, thresholds, levels, set);
        CHECK(got.size() == 1 && got[0].size() == levels);
        for (size_t l = 0; l < levels && got.size() == 1 && got[0].size() == levels; ++l) {
            CHECK(got[0][l].size() == n);
            for (size_t r = 0; r < n && got[0][l].size() == n; ++r)
                CHECK(got[0][l][r] == want[l][r]);
        }
        // one level of the same call; no motifs: an empty result
        const auto one = pli.scan_count({&pssm}, {thresholds[0]}, 1, set);
        CHECK(one.size() == 1 && one[0].size() == 1 && one[0][0] == want[0]);
        CHECK(pli.scan_count({}, {}, 1, set).empty());
        // the wrong number of thresholds, no levels and too many are refused before the library is asked
        int refused = 0;
        try {
            pli.scan_count({&pssm}, thresholds, levels + 1, set);
        } catch (const std::invalid_argument &) {
            ++refused;
        }
        try {
            pli.scan_count({&pssm}, {}, 0, set);
        } catch (const std::invalid_argument &) {
            ++refused;
        }
        try {
            pli.scan_count({&pssm}, std::vector<float>(LM_HIP_MAX_COUNT_LEVELS + 1, 0.0f), LM_HIP_MAX_COUNT_LEVELS + 1, set);
        } catch (const std::invalid_argument &) {
            ++refused;
        }
        CHECK(refused == 3);
        // a set without wrap rows is refused by the library
        bool threw = false;
        try {
            auto bare = pli.stripe_set(records);
            pli.scan_count({&pssm}, thresholds, levels, bare);
        } catch (const std::exception &) {
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
    std::printf("test_seqset_count: all checks passed\n");
    return 0;
}
