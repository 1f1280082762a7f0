// pssm_tables.hpp -- everything the kernels read of one scoring matrix, as ONE host image (host only: included by pssm.hip
// and tests/cpp/test_pssm_tables.cpp, by no kernel header; no HIP call).  lm_hip_pssm_create uploads `bytes` in one copy
// and points the d_* views of lm_hip_pssm at slab + offset.  Every table starts on a 256-byte boundary of the image (what
// an allocation of its own would have given it: the kernels copy tables 16 bytes at a time); padding bytes are zero.
//   dense         m x k row-major weights (generic / tiled kernels, re-scoring, Scanner::max)
//   table         transposed, padded table of score_c32<M>: table[s * ts + j] = pssm[j][s], M <= kMaxFastM
//   table_pad     the same with `lead` leading zero rows up to a multiple of 4 (M % 4 != 0, M + lead <= 32)
//   parts         slices of motifs beyond kMaxFastM rows (K <= 64), each with a table of its own
//   image         u16 image of the one-symbol prefilter scan (score_prefilter.hpp), M <= kMaxFastM
//   image2        pair-symbol table (score_prefilter2.hpp): DNA / protein up to kMaxFastM, DNA up to kMaxPairM
//   image2_drop   DNA, M = 20, 24 ... 36: the pair table of the first M - 1 rows (lm_hip_pssm::d_image2_drop)
//   image2_multi  DNA, M <= kMaxFastM: the pair table in the layout of the batch's multi-motif passes
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "score_prefilter2.hpp"

namespace lm {

constexpr size_t kAbsent = ~(size_t)0;

struct PssmTables {
    std::vector<unsigned char> bytes;  // the whole device image
    // byte offsets into `bytes`, kAbsent where the matrix has no such table
    size_t dense = kAbsent, table = kAbsent, table_pad = kAbsent, image = kAbsent, image2 = kAbsent, image2_drop = kAbsent,
           image2_multi = kAbsent;
    struct Part {
        size_t off, m, ts, lead, table;  // as lm_hip_pssm::Part; `table` = byte offset
    };
    std::vector<Part> parts;
    size_t ts = 0, lead = 0;
    unsigned drop_dmax = 0;
    bool has_prefilter = false;
    double pre_offset = 0, pre_factor = 0, pre_emax = 0;
};

// appends a table to the image on the next 256-byte boundary; returns its offset
template <class T>
inline size_t put_table(PssmTables &t, const std::vector<T> &v)
{
    const size_t at = (t.bytes.size() + 255) / 256 * 256;
    t.bytes.resize(at + v.size() * sizeof(T), 0);
    std::memcpy(t.bytes.data() + at, v.data(), v.size() * sizeof(T));
    return at;
}

// The discrete weights d'[0 .. mp) of the prefilter scans and the affine map discrete ~ (score - offset) / factor.  Follows
// the idea of DiscreteMatrix (pwm/mod.rs:665-696: per-row offsets, one global factor, weights rounded UP) on 16 bits;
// leading zero rows pad the motif to mp = prefilter_mp rows (even; a multiple of 4 for wide alphabets).  Returns false
// when no sound prefilter exists -- the exact f32 fused kernels are used then.
inline bool build_prefilter(const float *w, int m, int k, std::vector<unsigned> &d, PssmTables &t)
{
    const int mp = prefilter_mp(m, lds_wide(k)), shift = mp - m;
    std::vector<double> off(m);
    double offset = 0, range = 0, abs_sum = 0;
    for (int j = 0; j < m; ++j) {
        double lo = INFINITY, hi = -INFINITY, amax = 0;
        for (int s = 0; s < k; ++s) {
            const float x = w[(size_t)j * k + s];
            if (x != x || x == INFINITY)
                return false;             // NaN / +inf: score semantics the bound cannot cover
            if (x == -INFINITY)
                continue;                 // stands for the row minimum (over-estimate)
            lo = std::min(lo, (double)x);
            hi = std::max(hi, (double)x);
            amax = std::max(amax, std::fabs((double)x));
        }
        if (lo == INFINITY)
            return false;                 // a row of -inf only: every score is -inf
        off[j] = lo;
        offset += lo;
        range += hi - lo;
        abs_sum += amax;
    }
    if (!(range > 0))
        return false;
    // A window's partial sums stay within abs_sum in real arithmetic and within abs_sum * (1 + (m - 1) * 2^-24 * 1.5)
    // in f32; while that is below FLT_MAX none of them rounds to +-inf.  Above it a window can overflow to +inf (or
    // to NaN, +inf + -inf) although its real sum lies below the threshold, which no image of real sums can flag.
    if (abs_sum * (1.0 + (double)(m + 1) * std::ldexp(1.0, -23)) >= (double)FLT_MAX)
        return false;
    const double factor = range / (double)kPrefilterTop;
    d.assign((size_t)mp * k, 0);
    for (int j = 0; j < m; ++j)
        for (int s = 0; s < k; ++s) {
            const float x = w[(size_t)j * k + s];
            const double v = (x == -INFINITY) ? 0.0 : ((double)x - off[j]) / factor;
            unsigned q = (unsigned)std::ceil(v);
            if ((double)q < v + 1e-9)     // guard the ceil against representation error
                q += 1;
            d[(size_t)(j + shift) * k + s] = q;
        }
    t.pre_offset = offset;
    t.pre_factor = factor;
    // |f32 sum - real sum| <= (M-1) * 2^-24 * sum |terms|  (each add rounds to nearest; no partial sum overflows, see
    // the abs_sum limit above -- a sum that rounds to +-inf has an unbounded error)
    t.pre_emax = (double)m * std::ldexp(1.0, -24) * abs_sum * 1.5;
    return true;
}

// `w`: m x k row-major weights.  `xlong_store`: the context option of that name (65 ... kMaxStoreM rows as one slice).
inline PssmTables build_pssm_tables(const float *w, size_t m, size_t k, bool xlong_store)
{
    PssmTables t;
    if (!m)
        return t;
    const bool wide = lds_wide((int)k), fast = m <= (size_t)kMaxFastM;
    // transposed table of rows [off, off + real) behind `lead` zero rows: table[s * ts + lead + j] = w[off + j][s]
    // (K > 16: rows of 2 * odd dwords for the 8-byte reads of the WIDE kernels, see table_stride)
    auto transposed = [&](size_t off, size_t real, size_t lead, size_t ts) {
        std::vector<float> table(k * ts, 0.0f);
        for (size_t s = 0; s < k; ++s)
            for (size_t j = 0; j < real; ++j)
                table[s * ts + lead + j] = w[(off + j) * k + s];
        return put_table(t, table);
    };
    t.dense = put_table(t, std::vector<float>(w, w + m * k));
    if (fast) {
        t.ts = (size_t)table_stride((int)m, wide);
        t.table = transposed(0, m, 0, t.ts);
        // 33..35 stay as they are (36 rows cost more than the byte loads)
        if (m % 4 != 0 && (m + 3) / 4 * 4 <= 32) {
            t.lead = (m + 3) / 4 * 4 - m;
            t.table_pad = transposed(0, m, t.lead, (size_t)table_stride((int)(m + t.lead), wide));
        }
    } else if (k <= 64) {
        // long motifs: slices of <= kMaxLongM rows (multiples of 4 rows: dword symbol loads).  Up to kMaxLongM that is ONE
        // slice -- a single pass of the long kernel family (score_long_inst.hip); beyond, the first slice is stored and the
        // others continue in place (MODE_CONTINUE).  65 ... kMaxStoreM rows: ONE slice as well, padded to a multiple of 8 --
        // the store-only kernels of score_xlong_inst.hip (`xlong_store` false keeps the slices for A/B runs)
        const bool xlong = m > (size_t)kMaxLongM && m <= (size_t)kMaxStoreM && xlong_store;
        const size_t nparts = xlong ? 1 : (m + kMaxLongM - 1) / kMaxLongM, unit = xlong ? 8 : 4;
        const size_t len = xlong ? m : std::min<size_t>(((m + nparts - 1) / nparts + 3) / 4 * 4, (size_t)kMaxLongM);
        for (size_t off = 0; off < m; off += len) {
            const size_t real = std::min(len, m - off);
            PssmTables::Part part{off, 0, 0, (unit - real % unit) % unit, 0};  // the last slice: leading zero rows up to a multiple of 4 (8)
            part.m = real + part.lead;
            part.ts = (size_t)table_stride((int)part.m, wide);
            part.table = transposed(off, real, part.lead, part.ts);
            t.parts.push_back(part);
        }
    }
    // Prefilter images.  Up to kMaxFastM rows: the one-symbol image for every alphabet, the pair table for DNA / protein
    // (25 / 441 pair rows).  DNA up to kMaxPairM: the pair table alone, so that the fused scans of those lengths flag
    // candidates like the shorter ones do (the one-symbol u16 scan ends at kMaxFastM).
    const int mi = (int)m, ki = (int)k;
    std::vector<unsigned> d, img;
    if (!(fast || (m <= (size_t)kMaxPairM && k == 5)) || !build_prefilter(w, mi, ki, d, t))
        return t;
    t.has_prefilter = true;
    const unsigned *du = d.data() + (size_t)(prefilter_mp(mi, wide) - mi) * k;  // the unpadded weights
    // pair-symbol table of score_c32_prefilter2<M>: row (a, b) holds E[e] = d[e-1][a] + d[e][b] over the motif padded to
    // an ODD length M' by a leading zero row; dword m = (lo E[2m+1], hi E[2m]).  Same weights, same sums, same bound.
    auto pair_table = [&](int rows, int layout) {
        img.assign((size_t)prefilter2_image_dw(rows, layout), 0u);
        prefilter2_pack_image(du, rows, img.data(), layout);
        return put_table(t, img);
    };
    if (fast) {
        img.assign((size_t)prefilter_image_dw(mi, ki), 0u);
        prefilter_pack_image(d.data(), mi, ki, img.data());
        t.image = put_table(t, img);
    }
    if (k == 5 || k == 21)
        t.image2 = pair_table(mi, ki);
    if (fast && k == 5) {
        // the table without the motif's last row, for lengths whose padding wastes a read; what the last row can add at
        // most goes into the bound  (M = 12, 16: the shorter ring of M - 1 rows costs more than the read it saves:
        // 188 -> 219, 183 -> 192 us per Gbp)
        if (m >= 20 && m % 4 == 0) {
            t.image2_drop = pair_table(mi - 1, ki);
            t.drop_dmax = *std::max_element(du + (m - 1) * k, du + m * k);
        }
        t.image2_multi = pair_table(mi, kDnaMulti);
    }
    return t;
}

}  // namespace lm
