// sample_plan.hpp -- the host half of sample.hip: the generator, the threshold tables of a model, argument checks, the
// offsets of the sampled set, the capacity refusals, the image the draw kernels read and the packed transition maps of the
// first-order chain.  Plain C++ (no HIP header), so that tests/cpp/test_sample_plan.cpp can run it alone; the functions the
// kernels share with the host carry LM_SAMPLE_HD, which sample.hip defines as `__host__ __device__`.
//
// THE RULE (the device result equals it byte for byte).  u(seed, R, j), the uniform of position j of record number R, is
// word j & 3 of the Philox4x32-10 block with key (lo32(seed), hi32(seed)) and counter (lo32(j >> 2), lo32(R), hi32(R),
// hi32(j >> 2)): a record's text depends on the seed, its number and its model alone, and a longer record extends a
// shorter one.  A frequency row f[0..K) becomes K - 1 thresholds T[s] = floor(c_s / c_{K-1} * 2^32), c the running f64 sum,
// and draw(T, u) = #{s < K - 1 : u >= T[s]}.  T[s] lies in [0, 2^32]; the tables hold it as two things a 32-bit compare can
// use: `base`, the number of thresholds that are 0 (always passed; they are a prefix, T is ascending), and for the others
// T[s] - 1 in [0, 2^32 - 1], so that u >= T[s] is u > T[s] - 1 and 2^32 ("never") is 0xFFFFFFFF.  The slots of the always
// passed prefix hold 0xFFFFFFFF as well (never passed again): draw = base + #{s : u > word[s]}.
//
// ORDER 1.  x_0 = draw(T_initial, u_0), x_j = draw(T_row(x_{j-1}), u_j).  The step of a position is a map {0..4} -> {0..4},
// 3 bits per entry in 15 bits (entry a at bits 3a); the step of a record's first position is a CONSTANT map, so composing
// maps along the joined text needs no segmented scan: composition resets itself at every record start.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "lightmotif_hip.h"

#ifndef LM_SAMPLE_HD
#define LM_SAMPLE_HD
#endif

namespace lm {
namespace sample {

constexpr unsigned kRun = 16;                    // text bytes one lane draws: one 16-byte store
constexpr unsigned kBlockLanes = 256;
constexpr unsigned kTile = kBlockLanes * kRun;   // text bytes of one workgroup
constexpr unsigned kLdsSlab = 1024;              // dst entries (8 B each) a workgroup stages in LDS; global memory beyond
constexpr unsigned long long kMaxCells = 1ull << 40;  // what a hit list addresses (hits.hip: key = job << 40 | cell)
constexpr unsigned kDna = 5, kProtein = 21;
constexpr unsigned kNever = 0xFFFFFFFFu;
constexpr unsigned kIdentityMap = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12;

// words of one packed threshold row: K - 1 compare words and `base`, padded to a multiple of four
constexpr unsigned row_words(unsigned k) { return (k + 3u) & ~3u; }

// ---- the generator -------------------------------------------------------------------------------------------------------

LM_SAMPLE_HD inline unsigned mulhi32(unsigned a, unsigned b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

// Philox4x32-10: counter c[4] -> c[4] under key (k0, k1)
LM_SAMPLE_HD inline void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = mulhi32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = mulhi32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the four uniforms of positions 4q .. 4q + 3 of record number R
LM_SAMPLE_HD inline void uniforms(unsigned long long seed, unsigned long long R, unsigned long long q, unsigned out[4])
{
    out[0] = (unsigned)q, out[1] = (unsigned)R, out[2] = (unsigned)(R >> 32), out[3] = (unsigned)(q >> 32);
    philox4x32_10(out, (unsigned)seed, (unsigned)(seed >> 32));
}

// ---- transition maps ---------------------------------------------------------------------------------------------------------

LM_SAMPLE_HD inline unsigned map_apply(unsigned map, unsigned a) { return (map >> (3u * a)) & 7u; }
LM_SAMPLE_HD inline unsigned map_constant(unsigned x) { return x * 011111u; }  // x in every entry
// first f, then g
LM_SAMPLE_HD inline unsigned map_compose(unsigned f, unsigned g)
{
    unsigned h = 0;
    for (unsigned a = 0; a < kDna; ++a)
        h |= map_apply(g, map_apply(f, a)) << (3u * a);
    return h;
}

// ---- models ------------------------------------------------------------------------------------------------------------------

// every entry finite and >= 0 (a row like that whose sum is 0 is the ZERO row; with a sum > 0 it is VALID)
inline bool row_plausible(const float *f, unsigned k)
{
    for (unsigned s = 0; s < k; ++s)
        if (!std::isfinite(f[s]) || f[s] < 0)
            return false;
    return true;
}
inline double row_sum(const float *f, unsigned k)
{
    double c = 0;
    for (unsigned s = 0; s < k; ++s)
        c += (double)f[s];
    return c;
}
inline bool row_valid(const float *f, unsigned k) { return row_plausible(f, k) && row_sum(f, k) > 0; }
inline bool row_zero(const float *f, unsigned k) { return row_plausible(f, k) && row_sum(f, k) == 0; }

// T[0 .. k - 1) of a valid row, each in [0, 2^32]
inline void thresholds(const float *f, unsigned k, uint64_t *T)
{
    const double total = row_sum(f, k);
    double c = 0;
    for (unsigned s = 0; s + 1 < k; ++s) {
        c += (double)f[s];
        T[s] = (uint64_t)std::floor(c / total * 4294967296.0);
    }
}

LM_SAMPLE_HD inline unsigned draw_packed(const unsigned *row, unsigned k, unsigned u)
{
    unsigned x = row[k - 1];
    for (unsigned s = 0; s + 1 < k; ++s)
        x += u > row[s] ? 1u : 0u;
    return x;
}

// the rule's draw on the thresholds themselves
inline unsigned draw(const uint64_t *T, unsigned k, unsigned u)
{
    unsigned x = 0;
    for (unsigned s = 0; s + 1 < k; ++s)
        x += (uint64_t)u >= T[s] ? 1u : 0u;
    return x;
}

// row_words(k) words: see the head of this file
inline void pack_row(const float *f, unsigned k, unsigned *row)
{
    uint64_t T[kProtein];
    thresholds(f, k, T);
    unsigned base = 0;
    for (unsigned s = 0; s + 1 < k; ++s) {
        if (T[s] == 0) {
            ++base;
            row[s] = kNever;
        } else {
            row[s] = (unsigned)(T[s] - 1);
        }
    }
    row[k - 1] = base;
    for (unsigned s = k; s < row_words(k); ++s)
        row[s] = 0;
}

// The chain of a call, as the kernels take it (by value, in scalar registers): row 0 is `initial`, row 1 + a the row of
// state a -- or `initial` again where that row is the zero row.
struct MarkovModel {
    unsigned row[1 + kDna][row_words(kDna)];
};

// the step of a position that is not a record's first: a -> draw(row(a), u)
LM_SAMPLE_HD inline unsigned markov_step(const MarkovModel &m, unsigned u)
{
    unsigned map = 0;
    for (unsigned a = 0; a < kDna; ++a)
        map |= draw_packed(m.row[1 + a], kDna, u) << (3u * a);
    return map;
}
LM_SAMPLE_HD inline unsigned markov_first(const MarkovModel &m, unsigned u) { return map_constant(draw_packed(m.row[0], kDna, u)); }

// ---- the call ----------------------------------------------------------------------------------------------------------------

inline int refuse(std::string *msg, int status, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    if (msg)
        *msg = buf;
    return status;
}

// What the call was handed, as far as it can be judged without the device.
struct Args {
    bool ctx = false, out = false;  // the pointers are there
    char alphabet = 0;
    const uint64_t *lengths = nullptr;
    size_t n_records = 0;
    const float *frequencies = nullptr;
    size_t n_models = 0;
    const float *transitions = nullptr;
    size_t cols = 0;
};

inline int check(const Args &a, std::string *msg)
{
    if (!a.ctx || !a.out || !a.frequencies)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null argument");
    if (a.n_records && !a.lengths)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null lengths with a count of %llu", a.n_records);
    if (a.cols == 0)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "zero columns");
    if (a.alphabet != 'D' && a.alphabet != 'P')
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "alphabet %llu: 'D' or 'P'", (unsigned long long)(unsigned char)a.alphabet);
    if (a.n_models != 1 && a.n_models != a.n_records)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "%llu models for %llu records: one, or one per record", a.n_models, a.n_records);
    if (a.transitions && a.alphabet != 'D')
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "a first-order model is DNA only");
    if (a.transitions && a.n_models != 1)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "a first-order model is one model per call, not %llu", a.n_models);
    return LM_HIP_OK;
}

struct Plan {
    unsigned k = 0;
    bool order1 = false, shared = true;
    std::vector<uint64_t> offsets;            // n + 1: the sampled set's
    std::vector<unsigned long long> image;    // dst[nlive + 1] | record[nlive], as regions_plan.hpp; empty when nlive == 0
    std::vector<unsigned> rows;               // packed threshold rows: one (shared), or one per LIVE record
    MarkovModel chain{};
    size_t nlive = 0;
    uint64_t total = 0;                       // offsets[n]
    uint64_t nrows = 0;                       // ceil(total / cols)
    const unsigned long long *dst() const { return image.data(); }
    const unsigned long long *record() const { return image.data() + nlive + 1; }
};

// After check().  LM_HIP_ERR_CAPACITY as soon as the sum passes 2^40, long before it could wrap; LM_HIP_ERR_BAD_ARGS for a
// model row that a non-empty record would use and that is not valid (a transition row may be the zero row).
inline int make_plan(const Args &a, Plan *p, std::string *msg)
{
    *p = Plan();
    const unsigned k = a.alphabet == 'D' ? kDna : kProtein, w = row_words(k);
    const size_t n = a.n_records;
    p->k = k;
    p->order1 = a.transitions != nullptr;
    p->shared = a.n_models == 1;
    p->offsets.assign(n + 1, 0);
    uint64_t longest = 0;
    for (size_t i = 0; i < n; ++i) {
        if (a.lengths[i] > kMaxCells - p->total)
            return refuse(msg, LM_HIP_ERR_CAPACITY, "the records up to %llu hold more than the 2^40 cells a hit list can address", i);
        p->total += a.lengths[i];
        p->offsets[i + 1] = p->total;
        p->nlive += a.lengths[i] != 0;
        longest = a.lengths[i] > longest ? a.lengths[i] : longest;
    }
    p->nrows = (p->total + a.cols - 1) / a.cols;
    if (p->nrows > kMaxCells / a.cols)
        return refuse(msg, LM_HIP_ERR_CAPACITY, "%llu symbols in %llu columns exceed the 2^40 cells a hit list can address", p->total,
                      a.cols);
    if ((p->total + kTile - 1) / kTile >> 31)
        return refuse(msg, LM_HIP_ERR_CAPACITY, "%llu symbols are beyond the grid", p->total);
    if (p->nlive == 0)
        return LM_HIP_OK;
    // the models that will be used
    if (p->shared && !row_valid(a.frequencies, k))
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "row 0 of the frequencies is not a model: finite entries >= 0 with a sum > 0");
    if (p->order1) {
        pack_row(a.frequencies, k, p->chain.row[0]);
        for (unsigned s = 0; s < k; ++s) {
            const float *row = a.transitions + s * k;
            if (row_valid(row, k))
                pack_row(row, k, p->chain.row[1 + s]);
            else if (row_zero(row, k) || longest < 2)  // (no record of two symbols: no transition is taken)
                pack_row(a.frequencies, k, p->chain.row[1 + s]);
            else
                return refuse(msg, LM_HIP_ERR_BAD_ARGS, "row %llu of the transitions is neither a model nor zero", s);
        }
    }
    p->image.resize(2 * p->nlive + 1);
    unsigned long long *dst = p->image.data(), *rec = dst + p->nlive + 1;
    if (!p->order1)
        p->rows.resize(p->shared ? w : p->nlive * w);
    if (!p->order1 && p->shared)
        pack_row(a.frequencies, k, p->rows.data());
    size_t j = 0;
    for (size_t i = 0; i < n; ++i) {
        if (a.lengths[i] == 0)
            continue;
        if (!p->shared) {
            if (!row_valid(a.frequencies + i * k, k))
                return refuse(msg, LM_HIP_ERR_BAD_ARGS, "the frequencies of record %llu are not a model: finite entries >= 0 with a sum > 0",
                              i);
            pack_row(a.frequencies + i * k, k, p->rows.data() + j * w);
        }
        dst[j] = p->offsets[i];
        rec[j] = i;
        ++j;
    }
    dst[p->nlive] = p->total;
    return LM_HIP_OK;
}

// The rule on the host, from a plan: the text of record i (tests; nothing in the library calls it).
inline std::vector<uint8_t> host_record(const Args &a, const Plan &p, uint64_t seed, uint64_t record_base, size_t i)
{
    const uint64_t len = a.lengths[i], R = record_base + i;
    std::vector<uint8_t> text((size_t)len);
    unsigned row[row_words(kProtein)];
    if (len && !p.order1)
        pack_row(a.frequencies + (p.shared ? 0 : i * p.k), p.k, row);
    unsigned x = 0;
    for (uint64_t j = 0; j < len; ++j) {
        unsigned u[4];
        uniforms(seed, R, j >> 2, u);
        if (!p.order1)
            x = draw_packed(row, p.k, u[j & 3]);
        else
            x = map_apply(j ? markov_step(p.chain, u[j & 3]) : markov_first(p.chain, u[j & 3]), x);
        text[(size_t)j] = (uint8_t)x;
    }
    return text;
}

}  // namespace sample
}  // namespace lm
