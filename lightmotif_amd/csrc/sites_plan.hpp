// sites_plan.hpp -- the host half of sites.hip: argument checks, the window rule, and how a list of sites is cut into
// chunks and described to the kernels.  Plain C++ (no HIP), so that tests/cpp/test_sites_plan.cpp can run it alone.
//
// A call names n motifs; counts[i] consecutive sites belong to motif i, each site a (record, position) pair that names
// the window [position + shifts[i], position + shifts[i] + widths[i]) of its record.  Motifs without sites, and motifs
// wider than the whole set (none of whose windows can be valid), never reach the device: they are DEAD and the host
// fills their output.  The others are cut, in caller order, into SEGMENTS (the sites of one motif inside one chunk) and
// CHUNKS (what is uploaded and launched together).  A chunk's device image is one array of 64-bit words:
//
//     prefix[nseg + 1] | nseg x {site0, count, width, shift, table, used, slice} | sites x {record, position}
//
// prefix counts UNITS in front of each segment: output bytes for site_windows, workgroups for site_counts, so a kernel
// finds the segment of a unit by binary search.  site0 is relative to the chunk's sites.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lightmotif_hip.h"

#if defined(__HIPCC__)
#define LM_SITES_HD __host__ __device__
#else
#define LM_SITES_HD
#endif

namespace lm {
namespace sites {

constexpr size_t kBlockBytes = (size_t)256 << 20;  // sites + windows of one chunk on the device (as seqset_best's slots)
constexpr unsigned kSegWords = 7;
constexpr unsigned kGroupSites = 2048;     // site_counts: most sites one workgroup takes ...
constexpr unsigned kGroupItems = 65536;    // ... and about how many (site, j) pairs
constexpr unsigned kLdsCounters = 12288;   // 48 KB of u32: width * k + 1 of them make a private table
constexpr unsigned kLdsPrefix = 2048;      // prefix entries (8 B each) site_windows stages in LDS
constexpr size_t kDead = ~(size_t)0;

// Where the window of (position, shift, width) starts inside a record of `len` symbols; false: it does not lie inside.
// No intermediate wraps for any 64-bit position or shift: `position <= len` is settled before anything is added.
LM_SITES_HD inline bool window_start(unsigned long long position, long long shift, unsigned long long width, unsigned long long len,
                                     unsigned long long *start)
{
    unsigned long long s;
    if (shift >= 0) {
        if (position > len || (unsigned long long)shift > len - position)
            return false;
        s = position + (unsigned long long)shift;
    } else {
        const unsigned long long back = 0ull - (unsigned long long)shift;  // 2^63 for INT64_MIN
        if (position < back)
            return false;
        s = position - back;
        if (s > len)
            return false;
    }
    if (width > len - s)
        return false;
    *start = s;
    return true;
}

struct Request {
    const size_t *counts = nullptr, *widths = nullptr;
    const int64_t *shifts = nullptr;  // nullptr: all zero
    size_t n = 0;
    const void *sites = nullptr;
    size_t stride = 0;
    const void *out = nullptr;
    size_t capacity = 0;
};

struct Totals {
    size_t sites = 0;         // sum(counts)
    size_t window_bytes = 0;  // sum(counts[i] * widths[i])
    size_t width_sum = 0;     // sum(widths)
    size_t entries = 0;       // k * width_sum
};

inline int refuse(std::string *msg, int status, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    if (msg)
        *msg = buf;
    return status;
}

// Everything that can be said without the device.  `windows`: the output is sum(counts * widths) bytes, else k * sum(widths)
// table entries.
inline int check(const Request &r, size_t k, bool windows, Totals *t, std::string *msg)
{
    *t = Totals();
    if (r.n == 0)
        return LM_HIP_OK;
    if (!r.counts || !r.widths || !r.sites || !r.out)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "null argument");
    if (r.stride < 16)
        return refuse(msg, LM_HIP_ERR_BAD_ARGS, "a site holds a record at +0 and a position at +8: a stride of %llu bytes is below 16", r.stride);
    for (size_t i = 0; i < r.n; ++i)
        if (r.widths[i] == 0)
            return refuse(msg, LM_HIP_ERR_BAD_ARGS, "motif %llu has a width of 0", i);
    for (size_t i = 0; i < r.n; ++i) {
        size_t bytes;
        if (__builtin_add_overflow(t->sites, r.counts[i], &t->sites) || __builtin_mul_overflow(r.counts[i], r.widths[i], &bytes) ||
            __builtin_add_overflow(t->window_bytes, bytes, &t->window_bytes) ||
            __builtin_add_overflow(t->width_sum, r.widths[i], &t->width_sum))
            return refuse(msg, LM_HIP_ERR_CAPACITY, "the sizes of %llu motifs overflow", r.n);
    }
    size_t last;
    if (__builtin_mul_overflow(t->width_sum, k, &t->entries) || __builtin_mul_overflow(t->entries, sizeof(uint64_t), &last) ||
        (t->sites && __builtin_mul_overflow(t->sites - 1, r.stride, &last)))
        return refuse(msg, LM_HIP_ERR_CAPACITY, "the sizes of %llu motifs overflow", r.n);
    const size_t need = windows ? t->window_bytes : t->entries;
    if (r.capacity < need)
        return refuse(msg, LM_HIP_ERR_CAPACITY, "room for %llu of %llu elements", r.capacity, need);
    return LM_HIP_OK;
}

struct Seg {
    size_t motif = 0;
    size_t first = 0;       // of the motif's sites
    size_t count = 0;
    size_t site0 = 0;       // in the chunk
    unsigned long long units0 = 0;  // units of the chunk in front of this segment
    unsigned slice = 0;     // site_counts: sites per workgroup
};

struct Chunk {
    size_t seg0 = 0, seg1 = 0;
    size_t sites = 0;
    unsigned long long units = 0;
    bool direct = false;    // site_counts: tables too wide for LDS
    unsigned counters = 0;  // site_counts, LDS route: the widest table of the chunk, + 1
};

struct Plan {
    std::vector<Seg> segs;
    std::vector<Chunk> chunks;
    std::vector<size_t> site_base;  // first site of motif i in the caller's list
    std::vector<size_t> out_base;   // first output element of motif i in the caller's array
    std::vector<size_t> live;       // motif i -> its index among the live motifs, or kDead
    std::vector<size_t> table;      // live motif -> first entry of its table in the device block
    size_t nlive = 0, live_entries = 0;
    size_t max_sites = 0, max_segs = 0;
    unsigned long long max_units = 0;
    size_t image_words(const Chunk &c) const { return (c.seg1 - c.seg0) * (kSegWords + 1) + 1 + 2 * c.sites; }
    size_t max_image_words() const { return max_segs * (kSegWords + 1) + 1 + 2 * max_sites; }
};

inline bool counts_direct(size_t width, size_t k) { return width > (kLdsCounters - 1) / k; }

inline unsigned counts_slice(size_t width, bool direct)
{
    const size_t s = kGroupItems / width;  // (0 for very wide windows)
    const size_t lo = direct ? 1 : 8;      // an LDS table is flushed per workgroup: at least 8 sites to each flush
    return (unsigned)(s < lo ? lo : s > kGroupSites ? kGroupSites : s);
}

// `max_width`: windows wider than this cannot be valid (the set's total length).  `site_chunk`: most sites per chunk, 0 =
// bounded by `block_bytes` alone (16 bytes per site, + its window's bytes for site_windows).  A chunk holds at least one site.
inline void make_plan(const Request &r, size_t k, bool windows, size_t max_width, size_t site_chunk, size_t block_bytes, Plan *p)
{
    *p = Plan();
    p->site_base.resize(r.n);
    p->out_base.resize(r.n);
    p->live.assign(r.n, kDead);
    size_t sites = 0, out = 0;
    for (size_t i = 0; i < r.n; ++i) {
        p->site_base[i] = sites;
        p->out_base[i] = out;
        sites += r.counts[i];
        out += windows ? r.counts[i] * r.widths[i] : r.widths[i] * k;
        if (r.counts[i] && r.widths[i] <= max_width) {
            p->live[i] = p->nlive++;
            p->table.push_back(p->live_entries);
            p->live_entries += r.widths[i] * k;
        }
    }
    Chunk cur;
    size_t cur_bytes = 0;
    auto close = [&]() {
        if (cur.sites) {
            cur.seg1 = p->segs.size();
            p->chunks.push_back(cur);
            p->max_sites = cur.sites > p->max_sites ? cur.sites : p->max_sites;
            p->max_segs = cur.seg1 - cur.seg0 > p->max_segs ? cur.seg1 - cur.seg0 : p->max_segs;
            p->max_units = cur.units > p->max_units ? cur.units : p->max_units;
        }
        cur = Chunk();
        cur.seg0 = p->segs.size();
        cur_bytes = 0;
    };
    for (size_t i = 0; i < r.n; ++i) {
        if (p->live[i] == kDead)
            continue;
        const size_t width = r.widths[i];
        const bool direct = !windows && counts_direct(width, k);
        const size_t per_site = 16 + (windows ? width : 0);
        size_t first = 0;
        while (first < r.counts[i]) {
            if (cur.sites && cur.direct != direct)
                close();
            size_t take = r.counts[i] - first;
            if (site_chunk && take > site_chunk - cur.sites)
                take = site_chunk - cur.sites;
            const size_t room = cur_bytes < block_bytes ? (block_bytes - cur_bytes) / per_site : 0;
            if (take > room)
                take = room;
            if (take == 0) {
                if (cur.sites) {
                    close();
                    continue;
                }
                take = 1;
            }
            Seg s;
            s.motif = i;
            s.first = first;
            s.count = take;
            s.site0 = cur.sites;
            s.units0 = cur.units;
            s.slice = windows ? 0 : counts_slice(width, direct);
            p->segs.push_back(s);
            cur.direct = direct;
            cur.sites += take;
            cur.units += windows ? (unsigned long long)take * width : (take + s.slice - 1) / s.slice;
            if (!windows && !direct && width * k + 1 > cur.counters)
                cur.counters = (unsigned)(width * k + 1);
            cur_bytes += take * per_site;
            first += take;
        }
    }
    close();
}

// The device image of chunk `c` (see the head of this file); `image` is resized to plan.image_words(c).
inline void build_image(const Request &r, const Plan &p, const Chunk &c, std::vector<unsigned long long> *image)
{
    const size_t nseg = c.seg1 - c.seg0;
    image->resize(p.image_words(c));
    unsigned long long *prefix = image->data(), *segs = prefix + nseg + 1, *sites = segs + nseg * kSegWords;
    for (size_t s = 0; s < nseg; ++s) {
        const Seg &g = p.segs[c.seg0 + s];
        prefix[s] = g.units0;
        unsigned long long *w = segs + s * kSegWords;
        w[0] = g.site0;
        w[1] = g.count;
        w[2] = r.widths[g.motif];
        w[3] = (unsigned long long)(r.shifts ? r.shifts[g.motif] : 0);
        w[4] = p.table[p.live[g.motif]];
        w[5] = p.live[g.motif];
        w[6] = g.slice;
        const char *src = static_cast<const char *>(r.sites) + (p.site_base[g.motif] + g.first) * r.stride;
        unsigned long long *dst = sites + 2 * g.site0;
        if (r.stride == 16)
            memcpy(dst, src, g.count * 16);
        else
            for (size_t j = 0; j < g.count; ++j)
                memcpy(dst + 2 * j, src + j * r.stride, 16);
    }
    prefix[nseg] = c.units;
}

// What of a chunk's device output lies contiguously in the caller's arrays as well: dead motifs leave gaps.
struct Run {
    size_t dev_byte = 0, host_byte = 0, bytes = 0;
    size_t dev_site = 0, host_site = 0, sites = 0;
};
inline void window_runs(const Request &r, const Plan &p, const Chunk &c, std::vector<Run> *runs)
{
    runs->clear();
    for (size_t s = c.seg0; s < c.seg1; ++s) {
        const Seg &g = p.segs[s];
        Run x;
        x.dev_byte = (size_t)g.units0;
        x.host_byte = p.out_base[g.motif] + g.first * r.widths[g.motif];
        x.bytes = g.count * r.widths[g.motif];
        x.dev_site = g.site0;
        x.host_site = p.site_base[g.motif] + g.first;
        x.sites = g.count;
        if (!runs->empty() && runs->back().host_byte + runs->back().bytes == x.host_byte &&
            runs->back().host_site + runs->back().sites == x.host_site) {
            runs->back().bytes += x.bytes;
            runs->back().sites += x.sites;
        } else {
            runs->push_back(x);
        }
    }
}

}  // namespace sites
}  // namespace lm
