// Variant effects through the C++ host mirror (lightmotif_amd/host/lightmotif_hip.hpp): SequenceSet::variant_effects and
// variant_hits against windows scored on the host, M sequential f32 adds from +0.0 in row order (pli/mod.rs:96-105;
// pwm/mod.rs:651-662 of the record and of the record with one symbol replaced).
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

namespace {

unsigned next(unsigned &seed)
{
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
}

bool same_bits(float a, float b)
{
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y || (a != a && b != b);
}

// the best window covering p in `text`: greatest score, NaN never competing, the lowest start among equals
template <class A>
void best_side(const ScoringMatrix<A> &pssm, const std::vector<uint8_t> &text, size_t p, float *score, uint32_t *back)
{
    const size_t m = pssm.len(), len = text.size();
    *score = std::nanf("");
    *back = LM_HIP_VARIANT_NONE;
    if (len < m || m == 0)
        return;
    const size_t lo = p + 1 >= m ? p + 1 - m : 0, hi = std::min(p, len - m);
    for (size_t s = lo; s <= hi; ++s) {
        volatile float acc = 0.0f;
        for (size_t j = 0; j < m; ++j)
            acc = acc + pssm.matrix()(j, text[s + j]);
        const float v = acc;
        if (v == v && !(v <= *score)) {
            *score = v;
            *back = (uint32_t)(p - s);
        }
    }
}

template <class A>
void check_alphabet(unsigned seed)
{
    using Set = SequenceSet<A>;
    Pipeline<A> pli = Pipeline<A>::hip();
    std::vector<EncodedSequence<A>> records;
    for (size_t len : {(size_t)0, (size_t)1, (size_t)7, (size_t)300, (size_t)2, (size_t)45}) {
        std::string s(len, 'A');
        for (size_t i = 0; i < len; ++i)
            s[i] = A::symbols()[next(seed) % A::K];
        records.push_back(EncodedSequence<A>::encode(s));
    }
    Set set = pli.stripe_set(records);

    std::vector<ScoringMatrix<A>> owned;
    for (size_t m : {(size_t)1, (size_t)7, (size_t)12, (size_t)45, (size_t)70}) {
        DenseMatrix<float> d(m, A::K);
        for (size_t j = 0; j < m; ++j)
            for (size_t s = 0; s < A::K; ++s)
                d(j, s) = s + 1 == A::K ? -INFINITY : (float)((int)(next(seed) % 7) - 3);  // small integers: ties
        owned.emplace_back(std::vector<float>(A::K, 1.0f / A::K), std::move(d));
    }
    std::vector<const ScoringMatrix<A> *> pssms;
    for (const auto &p : owned)
        pssms.push_back(&p);

    std::vector<typename Set::Variant> variants;
    for (size_t i = 0; i < 700; ++i) {
        typename Set::Variant v{};
        v.record = next(seed) % (records.size() + 1);
        const size_t len = v.record < records.size() ? records[v.record].len() : 0;
        v.position = next(seed) % (len + 2);
        v.alt = (uint8_t)(next(seed) % (A::K + 1));
        variants.push_back(v);
    }
    typename Set::Variant far{};
    far.record = 3, far.position = ~(size_t)0, far.alt = 0;
    variants.push_back(far);

    for (int pass = 0; pass < 2; ++pass) {
        const auto got = set.variant_effects(pssms, variants);
        CHECK(got.effects.size() == pssms.size() && got.ref_symbols.size() == variants.size());
        std::vector<float> thresholds;
        for (size_t i = 0; i < pssms.size(); ++i)
            thresholds.push_back(i == 1 ? -INFINITY : i == 2 ? std::nanf("") : 2.0f);
        const auto hits = set.variant_hits(pssms, thresholds, variants);
        CHECK(hits.hits.size() == pssms.size() && hits.ref_symbols == got.ref_symbols);
        for (size_t i = 0; i < pssms.size(); ++i) {
            size_t next_hit = 0;
            for (size_t v = 0; v < variants.size(); ++v) {
                const auto &x = variants[v];
                const bool valid = x.record < records.size() && x.position < records[x.record].len() && x.alt < A::K;
                float rs = std::nanf(""), as = std::nanf("");
                uint32_t rb = LM_HIP_VARIANT_NONE, ab = LM_HIP_VARIANT_NONE;
                if (valid) {
                    std::vector<uint8_t> text = records[x.record].data;
                    best_side(*pssms[i], text, x.position, &rs, &rb);
                    text[x.position] = x.alt;
                    best_side(*pssms[i], text, x.position, &as, &ab);
                }
                if (i == 0)
                    CHECK(got.ref_symbols[v] == (valid ? records[x.record].data[x.position] : 0xFF));
                const auto &e = got.effects[i][v];
                CHECK(same_bits(e.ref_score, rs) && same_bits(e.alt_score, as) && e.ref_back == rb && e.alt_back == ab);
                if (rs >= thresholds[i] || as >= thresholds[i]) {
                    CHECK(next_hit < hits.hits[i].size());
                    if (next_hit < hits.hits[i].size()) {
                        const auto &h = hits.hits[i][next_hit++];
                        CHECK(h.variant == v && std::memcmp(&h.effect, &e, sizeof e) == 0);
                    }
                }
            }
            CHECK(next_hit == hits.hits[i].size());
        }
        set.configure_wrap(50);   // wrap rows are never read
    }
    bool threw = false;
    try {
        set.variant_hits(pssms, {1.0f}, variants);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    CHECK(set.variant_effects(pssms, {}).ref_symbols.empty());
}

}  // namespace

int main()
{
    static_assert(sizeof(lm_hip_variant) == 24 && sizeof(lm_hip_variant_effect) == 16 && sizeof(lm_hip_variant_hit) == 24, "the ABI's sizes");
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
    std::printf("test_variants: all checks passed\n");
    return 0;
}
