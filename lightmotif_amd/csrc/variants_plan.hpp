// variants_plan.hpp -- the host half of variants.hip: argument checks, the validity and clipping rules of a variant, and
// how a call's motifs and variants are cut into what is launched together.  Plain C++ (no HIP), so that
// tests/cpp/test_variants_plan.cpp can run it alone.
//
// A call names n motifs and V variants (record, position, alt).  The variants are cut into CHUNKS of at most `chunk`
// variants: a chunk is uploaded once and its clipped neighbourhoods [p - W + 1, p + W - 1] (W = the longest live motif,
// 2W - 1 bytes per variant, 0xFF outside the record) are gathered once.  The motifs are cut, in caller order, into GROUPS
// (what one workgroup loops over: up to kGroupMotifs motifs whose transposed tables fit the LDS budget together, or ONE
// motif whose table does not, read from global memory) and whole groups into BATCHES: batch x chunk is one dense device
// block of 16-byte effects, bounded by `block_bytes`.  Motifs with no rows or longer than every record have no window
// anywhere: they are DEAD, never reach the device, and the host writes "none" for them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "lightmotif_hip.h"

#if defined(__HIPCC__)
#define LM_VARIANTS_HD __host__ __device__
#else
#define LM_VARIANTS_HD
#endif

namespace lm {
namespace variants {

constexpr size_t kBlockBytes = (size_t)256 << 20;  // the dense effects of one batch x chunk (as seqset_best's slots)
constexpr size_t kDefaultChunk = (size_t)1 << 20;  // variants per chunk when the option "variant_chunk" is 0: a call of up to
                                                   // 2^20 variants is one chunk, and its dense rows go home in one copy
constexpr size_t kMaxChunk = (size_t)1 << 22;
constexpr unsigned kGroupMotifs = 64;              // most motifs one workgroup loops over
constexpr unsigned kLdsTableBytes = 24576;         // LDS for the tables of a group (option "variant_lds_bytes")
constexpr unsigned kLdsNeighbourBytes = 32768;     // LDS for the byte-transposed neighbourhoods of a workgroup's lanes
constexpr unsigned kWideBlock = 256, kNarrowBlock = 64;
constexpr unsigned kNbPad = 4;  // bytes behind each row nb[j][0 .. block): the transposing writes of a wavefront (j ascending, pitch
                                // block + 4 = an odd number of dwords) then fall on distinct banks
constexpr size_t kVariantBytes = sizeof(lm_hip_variant);
constexpr size_t kDead = ~(size_t)0;

// (record, position, alt) names a symbol of the set: evaluated on 64-bit values, nothing is added before it is settled.
// `len` is the record's length and is only looked at when record < records.
LM_VARIANTS_HD inline bool variant_valid(unsigned long long record, unsigned long long position, unsigned alt,
                                         unsigned long long records, unsigned long long len, unsigned k)
{
    return record < records && position < len && alt < k;
}

// How many symbols of the record lie in front of and behind position p (< len), at most w - 1 each: the neighbourhood
// [p - left, p + right].  No intermediate wraps for any 64-bit p < len.
LM_VARIANTS_HD inline void clip(unsigned long long p, unsigned long long len, unsigned w, unsigned *left, unsigned *right)
{
    const unsigned long long reach = (unsigned long long)w - 1, behind = len - 1 - p;
    *left = (unsigned)(p < reach ? p : reach);
    *right = (unsigned)(behind < reach ? behind : reach);
}

// The windows of a motif of m rows that cover the variant and lie inside the record, by `back` = p - start:
// back in [*lo, *lo + count).  Ascending start is DESCENDING back.
LM_VARIANTS_HD inline unsigned windows(unsigned m, unsigned left, unsigned right, unsigned *lo)
{
    if (m == 0)
        return 0;
    const unsigned hi = left < m - 1 ? left : m - 1;
    *lo = m - 1 > right ? m - 1 - right : 0;
    return hi >= *lo ? hi - *lo + 1 : 0;
}

inline int refuse(std::string *msg, int status, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    if (msg)
        *msg = buf;
    return status;
}

struct Pointers {
    bool ctx = false, set = false;
    bool pssms = false, variants = false;
    bool hits_form = false;
    bool effects = false;                                  // dense form
    bool thresholds = false, counts = false, hits = false;  // hits form
    size_t n = 0, n_variants = 0;
};

// Null arguments: everything that can be said before a matrix is looked at.
inline int check_pointers(const Pointers &p, std::string *msg)
{
    if (!p.ctx || !p.set)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null context or set");
    if (p.n && !p.pssms)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null matrix list");
    if (p.n && (p.hits_form ? !p.thresholds || !p.counts || !p.hits : !p.effects))
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null output or thresholds");
    if (p.n_variants && !p.variants)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null variant list");
    return LM_HIP_OK;
}

// The matrices against the set: ms[i] rows, ks[i] symbols.
inline int check_motifs(const size_t *ms, const size_t *ks, size_t n, size_t set_k, size_t n_variants, bool dense, std::string *msg)
{
    for (size_t i = 0; i < n; ++i)
        if (ks[i] != set_k)
            return refuse(msg, LM_HIP_ERR_BAD_ARGS, "matrix %llu has another alphabet size than the set's %llu", i, set_k);
    for (size_t i = 0; i < n; ++i)
        if ((unsigned long long)ms[i] >> 32)
            return refuse(msg, LM_HIP_ERR_CAPACITY, "matrix %llu has %llu rows: `back` is 32 bits", i, ms[i]);
    size_t cells, bytes;
    if (dense && (__builtin_mul_overflow(n, n_variants, &cells) || __builtin_mul_overflow(cells, sizeof(lm_hip_variant_effect), &bytes)))
        return refuse(msg, LM_HIP_ERR_CAPACITY, "%llu motifs x %llu variants overflow", n, n_variants);
    return LM_HIP_OK;
}

struct Group {
    unsigned first = 0, count = 0;  // live motifs, relative to the batch
    bool lds = true;
};

struct Batch {
    size_t live0 = 0, live1 = 0;   // live motifs
    size_t group0 = 0, group1 = 0;
    unsigned lds_groups = 0;       // of the batch; the others read global memory
    unsigned table_floats = 0;     // the largest group's LDS tables
};

struct Plan {
    std::vector<size_t> live;      // live motif -> motif of the call
    std::vector<size_t> live_of;   // motif -> live index or kDead
    std::vector<unsigned> tab;     // live motif -> first float of its LDS table inside its group's block
    std::vector<Group> groups;
    std::vector<Batch> batches;
    unsigned w = 1;                // the longest live motif (1 when none is live)
    unsigned long long nb = 1;     // 2w - 1: neighbourhood bytes per variant
    bool nb_in_lds = true;
    unsigned block = kWideBlock;   // lanes (variants) per workgroup of the effects kernel
    unsigned nb_lds_bytes = 0;
    size_t chunk = 0, nchunks = 0;  // variants per chunk, chunks
    size_t batch_motifs = 0;       // most live motifs per batch
    size_t max_batch = 0, max_groups = 0;
};

// floats of a motif's transposed LDS table: table[s * ts + j], ts odd so that the k symbol rows start on distinct banks
inline unsigned table_stride(size_t m) { return (unsigned)m | 1u; }
inline unsigned long long table_floats(size_t m, size_t k) { return (unsigned long long)table_stride(m) * k; }

// `max_len`: the longest record.  `variant_chunk`: most variants per chunk, 0 = kDefaultChunk.  `lds_bytes`: LDS for a
// group's tables, 0 = kLdsTableBytes.  A chunk holds at least one variant and a batch at least one motif.
inline void make_plan(const size_t *ms, size_t n, size_t k, unsigned long long max_len, size_t n_variants, size_t variant_chunk,
                      size_t lds_bytes, size_t block_bytes, Plan *p)
{
    *p = Plan();
    p->live_of.assign(n, kDead);
    size_t w = 1;
    for (size_t i = 0; i < n; ++i)
        if (ms[i] && ms[i] <= max_len) {
            p->live_of[i] = p->live.size();
            p->live.push_back(i);
            w = ms[i] > w ? ms[i] : w;
        }
    p->w = (unsigned)w;
    p->nb = 2ull * w - 1;
    if (p->nb * (kWideBlock + kNbPad) <= kLdsNeighbourBytes)
        p->block = kWideBlock;
    else if (p->nb * (kNarrowBlock + kNbPad) <= kLdsNeighbourBytes)
        p->block = kNarrowBlock;
    else
        p->nb_in_lds = false;
    p->nb_lds_bytes = p->nb_in_lds ? (unsigned)((p->nb * (p->block + kNbPad) + 15) / 16 * 16) : 0;

    // a chunk: the variants, a symbol and a clip per variant, the neighbourhoods; and one motif's effects must fit
    const unsigned long long per_variant = kVariantBytes + 1 + 8 + p->nb;
    size_t chunk = variant_chunk ? variant_chunk : kDefaultChunk;
    chunk = chunk > kMaxChunk ? kMaxChunk : chunk;
    if ((unsigned long long)chunk > block_bytes / per_variant)
        chunk = (size_t)(block_bytes / per_variant);
    if (chunk > block_bytes / sizeof(lm_hip_variant_effect))
        chunk = block_bytes / sizeof(lm_hip_variant_effect);
    chunk = chunk > n_variants ? n_variants : chunk;
    chunk = chunk ? chunk : 1;
    p->chunk = chunk;
    p->nchunks = (n_variants + chunk - 1) / chunk;
    size_t mb = block_bytes / sizeof(lm_hip_variant_effect) / chunk;
    mb = mb > 32768 ? 32768 : mb ? mb : 1;
    p->batch_motifs = mb;

    const unsigned long long budget = (lds_bytes ? lds_bytes : kLdsTableBytes) / sizeof(float);
    const size_t group_cap = mb < kGroupMotifs ? mb : kGroupMotifs;
    p->tab.assign(p->live.size(), 0);
    Batch b;
    Group g;
    unsigned long long g_floats = 0;
    auto close_group = [&]() {
        if (g.count) {
            p->groups.push_back(g);
            if (g.lds) {
                ++b.lds_groups;
                b.table_floats = g_floats > b.table_floats ? (unsigned)g_floats : b.table_floats;
            }
            b.live1 += g.count;
        }
        g = Group();
        g.first = (unsigned)(b.live1 - b.live0);
        g_floats = 0;
    };
    auto close_batch = [&]() {
        close_group();
        if (b.live1 > b.live0) {
            b.group1 = p->groups.size();
            p->batches.push_back(b);
            p->max_batch = b.live1 - b.live0 > p->max_batch ? b.live1 - b.live0 : p->max_batch;
            p->max_groups = b.group1 - b.group0 > p->max_groups ? b.group1 - b.group0 : p->max_groups;
        }
        const size_t at = b.live1;
        b = Batch();
        b.live0 = b.live1 = at;
        b.group0 = p->groups.size();
        g = Group();
    };
    for (size_t li = 0; li < p->live.size(); ++li) {
        const unsigned long long floats = table_floats(ms[p->live[li]], k);
        const bool lds = floats <= budget;
        if (g.count && (g.lds != lds || !lds || g.count >= group_cap || g_floats + floats > budget))
            close_group();
        if ((b.live1 - b.live0) + g.count >= mb)
            close_batch();
        g.lds = lds;
        p->tab[li] = lds ? (unsigned)g_floats : 0;
        g_floats += lds ? floats : 0;
        ++g.count;
    }
    close_batch();
}

}  // namespace variants
}  // namespace lm
