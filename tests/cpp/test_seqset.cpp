// The sequence set through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): SequenceSet +
// Pipeline::scan_threshold(pssms, thresholds, set) against Pipeline::scan on every record alone -- the CLI's job
// product (lightmotif-cli main.rs:502-561) in one call.  The golden motif and sequence are those of tests/dna.rs:
// hits at 18, 27 and 32 for a threshold of -10 (scan.rs:279-353).
#include <cmath>
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

static const char *SEQUENCE = "ATGTCCCAACAACGATACCCCGAGCCCATCGCCGTCATCGGCTCGGCATGCAGATTCCCAGGCG";
static const std::vector<std::string> PATTERNS = {"GTTGACCTTATCAAC", "GTTGATCCAGTCAAC"};

static ScoringMatrix<Dna> golden_pssm()
{
    std::vector<EncodedSequence<Dna>> sites;
    for (const auto &p : PATTERNS)
        sites.push_back(EncodedSequence<Dna>::encode(p));
    return CountMatrix<Dna>::from_sequences(sites).to_freq(0.1f).to_weight().to_scoring();
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main()
{
    try {
        Pipeline<Dna> pli = Pipeline<Dna>::hip();
        const auto pssm = golden_pssm();
        const auto rc = pssm.reverse_complement();
        const std::string s(SEQUENCE);
        // the whole sequence | empty | cut inside the window of the hit at 27 (27 .. 41) | shorter than the motif | the
        // whole sequence again | its first 33 bases: the hit at 18 ends exactly on the last base
        const std::vector<std::string> records = {s, "", s.substr(0, 35), s.substr(35), "ACGTACGT", s, s.substr(0, 33)};
        auto set = pli.stripe_set(records);
        CHECK(set.records() == records.size());
        size_t total = 0;
        for (size_t r = 0; r < records.size(); ++r) {
            CHECK(set.len(r) == records[r].size());
            total += records[r].size();
        }
        CHECK(set.total_length() == total && set.lengths().size() == records.size() && set.columns() == 32);
        set.configure_wrap(pssm.len());
        CHECK(set.wrap() == pssm.len());

        const std::vector<const ScoringMatrix<Dna> *> motifs = {&pssm, &rc};
        const auto got = pli.scan_threshold(motifs, {-10.0f, -12.0f}, set);
        CHECK(got.size() == 2);
        const float ts[2] = {-10.0f, -12.0f};
        size_t n_hits = 0;
        for (size_t mi = 0; mi < got.size(); ++mi) {
            std::vector<Pipeline<Dna>::SetHit> want;   // every record alone through the one-sequence scanner
            for (size_t r = 0; r < records.size(); ++r) {
                if (records[r].empty())
                    continue;
                auto striped = pli.stripe(EncodedSequence<Dna>::encode(records[r]));
                striped.configure_wrap(pssm.len());
                for (const auto &h : pli.scan(*motifs[mi], striped, ts[mi]))
                    want.push_back({r, h.position, h.score});
            }
            CHECK(got[mi].size() == want.size());
            for (size_t k = 0; k < std::min(got[mi].size(), want.size()); ++k)
                CHECK(got[mi][k].record == want[k].record && got[mi][k].position == want[k].position &&
                      same_bits(got[mi][k].score, want[k].score));
            n_hits += want.size();
        }
        CHECK(n_hits >= 8);
        // the literal expectation for the direct strand: 18, 27, 32 in the whole records; 18 alone in [0, 35) and in
        // [0, 33); nothing in the tail [35, 64) (the hit at 27 straddles the cut, 32 + 15 > 35)
        const std::vector<std::pair<size_t, size_t>> literal = {{0, 18}, {0, 27}, {0, 32}, {2, 18}, {5, 18}, {5, 27}, {5, 32}, {6, 18}};
        CHECK(got[0].size() == literal.size());
        for (size_t k = 0; k < std::min(got[0].size(), literal.size()); ++k)
            CHECK(got[0][k].record == literal[k].first && got[0][k].position == literal[k].second);
        if (!got[0].empty())
            CHECK(std::fabs(got[0][0].score - (-5.50167f)) < 1e-5f);

        // encoded records give the same set
        std::vector<EncodedSequence<Dna>> encoded;
        for (const auto &r : records)
            encoded.push_back(EncodedSequence<Dna>::encode(r));
        auto set2 = pli.stripe_set(encoded);
        set2.configure_wrap(pssm.len());
        const auto got2 = pli.scan_threshold(motifs, {-10.0f, -12.0f}, set2);
        CHECK(got2.size() == 2 && got2[0].size() == got[0].size() && got2[1].size() == got[1].size());

        // misuse: strict text with an unknown symbol names it; a set without wrap rows is refused
        bool threw = false;
        try {
            pli.stripe_set(std::vector<std::string>{"ACGT", "AC?T"});
        } catch (const InvalidSymbol &e) {
            threw = e.symbol == '?';
        }
        CHECK(threw);
        threw = false;
        try {
            auto bare = pli.stripe_set(records);
            pli.scan_threshold(motifs, {-10.0f, -12.0f}, bare);
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
    std::printf("test_seqset: all checks passed\n");
    return 0;
}
