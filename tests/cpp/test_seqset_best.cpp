// The best hit per record through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): Pipeline::scan_best over
// the planted edge records of tests/seqset_best_cases.py.  The case file is written by tests/test_cpp_seqset_best.py:
//   line 1     the consensus (the matrix: +2 for the consensus base, -2 for the others, +2 for N)
//   line 2     the number of records
//   then per record one line `text found position score_bits` with the values Python's scan_best_set printed
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
            std::fprintf(stderr, "usage: test_seqset_best CASE_FILE\n");
            return 3;
        }
        std::ifstream in(argv[1]);
        std::string consensus;
        size_t n = 0;
        in >> consensus >> n;
        std::vector<std::string> records(n);
        std::vector<int> found(n);
        std::vector<long long> position(n);
        std::vector<uint32_t> score_bits(n);
        for (size_t r = 0; r < n; ++r) {
            in >> records[r] >> found[r] >> position[r] >> score_bits[r];
            if (records[r] == "-")
                records[r].clear();
        }
        CHECK(bool(in) && n > 0 && !consensus.empty());

        const size_t m = consensus.size();
        DenseMatrix<float> w(m, Dna::K);
        for (size_t j = 0; j < m; ++j)
            for (size_t s = 0; s < Dna::K; ++s)
                w(j, s) = (s == 4 || Dna::symbols()[s] == consensus[j]) ? 2.0f : -2.0f;
        const ScoringMatrix<Dna> pssm(std::vector<float>(Dna::K, 0.25f), w);

        auto set = pli.stripe_set(records);
        set.configure_wrap(m);
        const auto got = pli.scan_best({&pssm}, set);
        CHECK(got.size() == 1 && got[0].size() == n);
        for (size_t r = 0; r < n && got.size() == 1 && got[0].size() == n; ++r) {
            const auto &b = got[0][r];
            CHECK(b.found == (found[r] != 0));
            if (found[r]) {
                uint32_t gb;
                std::memcpy(&gb, &b.score, 4);
                CHECK((long long)b.position == position[r] && gb == score_bits[r]);
            } else {
                CHECK(b.position == 0 && b.score != b.score);
            }
        }
        // no motifs: an empty result; a set without wrap rows is refused
        CHECK(pli.scan_best({}, set).empty());
        bool threw = false;
        try {
            auto bare = pli.stripe_set(records);
            pli.scan_best({&pssm}, bare);
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
    std::printf("test_seqset_best: all checks passed\n");
    return 0;
}
