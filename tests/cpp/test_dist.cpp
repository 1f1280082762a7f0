// The device's score distributions through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp):
// ScoreDistributions against the plain sequential f64 loops of pwm/dist.rs:129-225 written out below -- the survival
// functions bit for bit, the thresholds of `scores` and the p-values of `pvalues`.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

constexpr int kRange = 1000;

struct HostDist {
    std::vector<double> sf;
    double scale = 0, offset = 0;
    long min_score = 0, max_score = 0;
    size_t rows = 0;

    template <class A>
    explicit HostDist(const ScoringMatrix<A> &pssm) : rows(pssm.len())
    {
        const double inf = std::numeric_limits<double>::infinity();
        double small = inf, large = -inf;
        for (size_t i = 0; i < rows; ++i)
            for (size_t a = 0; a < A::K; ++a) {
                const double w = pssm.data(i, a);
                if (std::isfinite(w)) {
                    small = w < small ? w : small;
                    large = w > large ? w : large;
                }
            }
        if (small == large)
            small = large - 1.0;
        offset = std::floor(small);
        scale = std::floor(kRange / (large - offset));
        const size_t size = rows * kRange + 1;
        std::vector<double> pdf_old(size, 0.0), pdf_new(size, 0.0);
        pdf_new[0] = 1.0;
        for (size_t i = 0; i < rows; ++i) {
            const size_t mx = i * kRange;
            pdf_old.swap(pdf_new);
            std::fill(pdf_new.begin(), pdf_new.end(), 0.0);
            for (size_t a = 0; a < A::K; ++a) {
                const double w = pssm.data(i, a);
                if (!std::isfinite(w))
                    continue;
                const size_t s = (size_t)std::round((w - offset) * scale);
                const double bg = (double)pssm.background[a];
                for (size_t t = 0; t <= mx; ++t)
                    pdf_new[t + s] += pdf_old[t] * bg;
            }
        }
        sf.assign(size, 0.0);
        double above = 0.0;
        for (size_t t = size; t-- > 0;) {
            const double x = pdf_new[t] + above;
            above = x > 1.0 ? 1.0 : x;
            sf[t] = above;
            if (pdf_new[t] > 0.0) {
                if (t >= 1 && max_score == 0)
                    max_score = (long)t;
                if (t + 2 <= size)
                    min_score = (long)t;
            }
        }
    }
    float unscale(long t) const { return (float)t / (float)scale + (float)((double)rows * offset); }
    float score(double p) const
    {
        if (p >= 1.0)
            return unscale(min_score);
        if (p <= 0.0)
            return unscale(max_score);
        size_t lo = 0, hi = sf.size();
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (p == sf[mid])
                return unscale((long)mid);
            if (p < sf[mid])
                lo = mid + 1;
            else
                hi = mid;
        }
        return unscale((long)lo);
    }
    double pvalue(float score) const
    {
        const double r = std::round(((double)score - (double)rows * offset) * scale);
        if (r < (double)min_score)
            return 1.0;
        if (r >= (double)sf.size())
            return 0.0;
        return sf[(size_t)r];
    }
};

bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

ScoringMatrix<Dna> dna_matrix(size_t rows, unsigned seed, bool holes)
{
    DenseMatrix<float> w(rows, Dna::K);
    for (size_t i = 0; i < rows; ++i)
        for (size_t a = 0; a < Dna::K; ++a) {
            seed = seed * 1664525u + 1013904223u;
            w(i, a) = (float)((seed >> 8) % 9000u) / 1000.0f - 6.5f;
            if (holes && (seed >> 28) == 3u)
                w(i, a) = -std::numeric_limits<float>::infinity();
        }
    return ScoringMatrix<Dna>({0.3f, 0.2f, 0.2f, 0.3f, 0.0f}, w);
}

}  // namespace

int main()
{
    try {
        Pipeline<Dna> pli = Pipeline<Dna>::hip();
        std::vector<ScoringMatrix<Dna>> owned;
        owned.push_back(dna_matrix(1, 1u, false));
        owned.push_back(dna_matrix(2, 2u, true));
        owned.push_back(dna_matrix(7, 3u, false));
        owned.push_back(dna_matrix(12, 4u, true));
        owned.push_back(dna_matrix(5, 5u, false));
        std::vector<const ScoringMatrix<Dna> *> pssms;
        for (const auto &p : owned)
            pssms.push_back(&p);
        const ScoreDistributions<Dna> dists = pli.score_distributions(pssms);
        CHECK(dists.size() == pssms.size());

        std::vector<HostDist> want;
        for (const auto &p : owned)
            want.emplace_back(p);
        for (size_t i = 0; i < pssms.size(); ++i) {
            const auto info = dists.info(i);
            CHECK(info.rows == owned[i].len() && info.sf_len == want[i].sf.size());
            CHECK(info.scale == want[i].scale && info.offset == want[i].offset);
            CHECK(info.min_score == want[i].min_score && info.max_score == want[i].max_score);
            CHECK(same_bits(dists.sf(i), want[i].sf));
        }
        for (const double p : {1e-5, 1e-3, 0.3, 1.0, 0.0, 1.5, -1.0, 1e-300}) {
            const std::vector<float> got = dists.scores(p);
            for (size_t i = 0; i < pssms.size(); ++i) {
                const float w = want[i].score(p);
                CHECK(std::memcmp(&got[i], &w, sizeof(float)) == 0);
            }
        }
        // p-values: a sweep across and beyond each table's range, an empty list in between
        std::vector<std::vector<float>> scores(pssms.size());
        for (size_t i = 0; i < pssms.size(); ++i) {
            if (i == 2)
                continue;
            const float lo = want[i].unscale(0), hi = want[i].unscale((long)want[i].sf.size() - 1);
            for (int j = -20; j <= 220; ++j)
                scores[i].push_back(lo + (hi - lo) * (float)j / 200.0f);
            scores[i].push_back(std::numeric_limits<float>::infinity());
            scores[i].push_back(-std::numeric_limits<float>::infinity());
        }
        const auto got = dists.pvalues(scores);
        CHECK(got.size() == scores.size() && got[2].empty());
        for (size_t i = 0; i < got.size(); ++i) {
            CHECK(got[i].size() == scores[i].size());
            for (size_t j = 0; j < got[i].size() && j < scores[i].size(); ++j) {
                const double w = want[i].pvalue(scores[i][j]);
                CHECK(std::memcmp(&got[i][j], &w, sizeof(double)) == 0);
            }
        }
        // a strided read: the score field of a hit list
        std::vector<lm_hip_set_hit> hits(3);
        for (size_t j = 0; j < hits.size(); ++j)
            hits[j] = {j, j, want[3].unscale(want[3].max_score - (long)(400 * j))};
        const std::vector<double> strided = dists.pvalues({0, 0, 0, hits.size(), 0}, &hits[0].score, sizeof(lm_hip_set_hit));
        CHECK(strided.size() == hits.size());
        for (size_t j = 0; j < strided.size(); ++j)
            CHECK(strided[j] == want[3].pvalue(hits[j].score));

        CHECK(pli.score_distributions({}).size() == 0);
        bool threw = false;
        try {
            DenseMatrix<float> w(2, Dna::K);
            w(1, 2) = std::numeric_limits<float>::quiet_NaN();
            const ScoringMatrix<Dna> bad(uniform_background<Dna>(), w);
            pli.score_distributions({&bad});
        } catch (const UnsupportedBackend &) {
            throw;
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
    std::printf("test_dist: all checks passed\n");
    return 0;
}
