// regions_plan.hpp -- the host half of regions.hip: argument checks, the clipping rule, the offsets of the derived set
// and the image the gather kernel reads.  Plain C++ (no HIP), so that tests/cpp/test_regions_plan.cpp can run it alone.
//
// A call names n regions; region i is [start, end) of source record `record` (BED: 0-based, half-open), clipped to the
// record, on strand 0 (as it stands) or 1 (reverse complement).  Record i of the derived set is region i, so its
// offsets are the prefix sum of the clipped lengths.  Both sets keep their offsets on the host: nothing here needs the
// device.  Regions that clip to nothing are EMPTY: they keep their place in the offsets and never reach the device.
// The others are LIVE, and the device image lists them in caller order as one array of 64-bit words:
//
//     dst[nlive + 1] | nlive x {src, strand}
//
// dst[j] is where live region j begins in the joined text of the result (strictly ascending, dst[nlive] = its length),
// so the kernel finds the region of a destination byte by binary search; src is the position of the region's FIRST
// SOURCE symbol, offsets[record] + s, in the source's concatenation (its last symbol, which a minus-strand record
// begins with, is src + length - 1).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "lightmotif_hip.h"

namespace lm {
namespace regions {

constexpr unsigned kRun = 16;                    // destination bytes one lane gathers: one 16-byte store
constexpr unsigned kBlockLanes = 256;
constexpr unsigned kTile = kBlockLanes * kRun;   // destination bytes of one workgroup
constexpr unsigned kLdsSlab = 1024;              // dst entries (8 B each) a workgroup stages in LDS; global memory beyond
constexpr unsigned kLiveWords = 2;               // {src, strand}
constexpr unsigned long long kMaxCells = 1ull << 40;  // what a hit list addresses (hits.hip: key = job << 40 | cell)

static_assert(sizeof(lm_hip_region) == 32, "lm_hip_region is 32 bytes");

// [start, end) against a record of `len` symbols: s = max(start, 0), e = min(end, len).  false (and s == e == 0): nothing
// is left.  Every comparison is on the signed value or on a value already known to be >= 0: no intermediate wraps.
inline bool clip(int64_t start, int64_t end, uint64_t len, uint64_t *s, uint64_t *e)
{
    const uint64_t a = start < 0 ? 0 : (uint64_t)start;
    const uint64_t b = end < 0 ? 0 : ((uint64_t)end > len ? len : (uint64_t)end);
    if (a >= b) {
        *s = *e = 0;
        return false;
    }
    *s = a;
    *e = b;
    return true;
}

// abc.rs:174-185 on symbol bytes: A0 <-> T2, C1 <-> G3; N and whatever else a matrix holds stay
inline uint8_t complement(uint8_t b) { return b < 4 ? (uint8_t)(b ^ 2u) : b; }

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
    bool ctx = false, src = false, out = false;  // the pointers are there
    int ctx_device = 0, src_device = 0;
    size_t k = 0;                                // the source's alphabet size
    const lm_hip_region *regions = nullptr;
    size_t n = 0;
};

inline int check(const Args &a, std::string *msg)
{
    if (!a.ctx || !a.src || !a.out)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null argument");
    if (a.n && !a.regions)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null regions with a count of %llu", a.n);
    if (a.src_device != a.ctx_device)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "the set lives on device %llu, the context on %llu", (unsigned long long)a.src_device,
                      (unsigned long long)a.ctx_device);
    for (size_t i = 0; i < a.n; ++i) {
        if (a.regions[i].strand > 1)
            return refuse(msg, LM_HIP_ERR_BAD_ARGS, "region %llu has strand %llu: 0 (as it stands) or 1 (reverse complement)", i,
                          a.regions[i].strand);
        if (a.regions[i].strand == 1 && a.k != 5)
            return refuse(msg, LM_HIP_ERR_BAD_ARGS, "region %llu asks for the reverse complement of a set of alphabet size %llu: DNA only",
                          i, a.k);
    }
    return LM_HIP_OK;
}

struct Plan {
    std::vector<uint64_t> offsets;            // n + 1: the derived set's
    std::vector<unsigned long long> image;    // see the head of this file; empty when nlive == 0
    size_t nlive = 0;
    uint64_t total = 0;                       // offsets[n]
    uint64_t rows = 0;                        // ceil(total / cols)
    const unsigned long long *dst() const { return image.data(); }
    const unsigned long long *live(size_t j) const { return image.data() + nlive + 1 + j * kLiveWords; }
};

// `src_offsets`: records + 1 entries.  `taken` (n entries) may be null.  LM_HIP_ERR_CAPACITY when ceil(total / cols) * cols
// exceeds kMaxCells: the sum is refused as soon as it passes 2^40, long before it could wrap.
inline int make_plan(const uint64_t *src_offsets, size_t records, size_t cols, const lm_hip_region *regions, size_t n,
                     lm_hip_region_span *taken, Plan *p, std::string *msg)
{
    *p = Plan();
    p->offsets.assign(n + 1, 0);
    std::vector<size_t> live;
    for (size_t i = 0; i < n; ++i) {
        const lm_hip_region &r = regions[i];
        uint64_t s = 0, e = 0;
        if (r.record < records && clip(r.start, r.end, src_offsets[r.record + 1] - src_offsets[r.record], &s, &e))
            live.push_back(i);
        if (taken) {
            taken[i].start = s;
            taken[i].end = e;
        }
        p->total += e - s;  // (a term is below 2^63 -- an int64 end -- and the sum so far at most 2^40: no wrap)
        if (p->total > kMaxCells)
            return refuse(msg, LM_HIP_ERR_CAPACITY, "the regions up to %llu hold more than the 2^40 cells a hit list can address", i);
        p->offsets[i + 1] = p->total;
    }
    p->rows = (p->total + cols - 1) / cols;
    if (p->rows > kMaxCells / cols)
        return refuse(msg, LM_HIP_ERR_CAPACITY, "%llu symbols in %llu columns exceed the 2^40 cells a hit list can address", p->total, cols);
    p->nlive = live.size();
    if (p->nlive == 0)
        return LM_HIP_OK;
    p->image.resize(p->nlive + 1 + p->nlive * kLiveWords);
    unsigned long long *dst = p->image.data(), *w = dst + p->nlive + 1;
    for (size_t j = 0; j < p->nlive; ++j, w += kLiveWords) {
        const size_t i = live[j];
        const lm_hip_region &r = regions[i];
        uint64_t s, e;
        (void)clip(r.start, r.end, src_offsets[r.record + 1] - src_offsets[r.record], &s, &e);
        dst[j] = p->offsets[i];
        w[0] = src_offsets[r.record] + s;
        w[1] = r.strand;
    }
    dst[p->nlive] = p->total;
    return LM_HIP_OK;
}

}  // namespace regions
}  // namespace lm
