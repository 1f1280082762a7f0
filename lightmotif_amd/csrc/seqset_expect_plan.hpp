// seqset_expect_plan.hpp -- the arithmetic of seqset_expect.hip (expected site counts of a set: the E-step of motif EM):
// the fixed point, the weight of one window and the run of one lane of the record walk.  Host- and device-compilable (no
// HIP call, no launch), so that tests/cpp/test_seqset_expect.cpp runs it with the Walker in plain C++.
//
// The rule.  Per motif i (M rows, scale s_i) and record r with gain g = gains[i][r] (finite, >= 0), every window p with
// p + M <= len(r) scores v as `score_into` scores it (M sequential f32 adds from +0.0), and
//       e = exp2_wide(fl32(s_i * v))          (seqset_sum_plan.hpp: the term of the sum of odds)
//       z = min(e * g, 1.0)   in f64          (a NaN score or a NaN product: the window contributes nothing)
//       q = (u64) rint(z * 2^F)               (round to nearest even)
//       F = min(40, 62 - bit_length(N)),  N the positions of the set
// and Q[i][j][s] is the sum of q over the windows whose symbol at offset j is s: an exact integer.  z <= 1 and a cell
// sums at most N windows, so Q < 2^62.  The caller's table is (double) Q * 2^-F.
//
// Integer additions commute: Q does not depend on who adds first, so the lanes may meet in integer atomics (LDS, then
// global memory) and the result has the same bits at any rows_per_stream and in any batch.  A window with q == 0 is
// skipped, exactly.
#pragma once

#include <cstddef>
#include <cstdint>

#include "seqset_sum_plan.hpp"
#include "seqset_walk.hpp"

namespace lm {
namespace setexpect {

typedef unsigned long long u64;

constexpr int kMaxFracBits = 40;
constexpr size_t kExpectLdsBytes = 64 * 1024;  // of a workgroup: weights, offsets and the table

LM_SUM_HD int bit_length(u64 x)
{
    int b = 0;
    for (; x; x >>= 1)
        ++b;
    return b;
}

// F of a set of `positions` symbols (bit_length <= 62 - F: a cell of `positions` windows of weight 1 stays below 2^62)
LM_SUM_HD int frac_bits_of(u64 positions)
{
    const int f = 62 - bit_length(positions);
    return f < kMaxFracBits ? (f < 0 ? 0 : f) : kMaxFracBits;
}

// 2^f as a double, 0 <= f <= 62
LM_SUM_HD double pow2_of(int f) { return (double)(1ull << f); }

// the weight of a window that scored v in a record of gain g, as a multiple of 2^-F (`unit` = 2^F)
LM_SUM_HD u64 quantum(float v, float scale, double g, double unit)
{
    if (!(v == v))
        return 0;
    const double zz = setsum::exp2_wide(scale * v) * g;
    if (!(zz == zz))  // +inf * 0
        return 0;
    const double z = zz < 1.0 ? zz : 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
    return (u64)__builtin_rint(z * unit);
#else
    return (u64)std::nearbyint(z * unit);  // (the default rounding mode: to nearest even)
#endif
}

// bytes of LDS a workgroup of the kernel takes: [weights, 16-byte padded when staged][offsets when staged][table when it
// fits].  The launcher and the kernel both ask here.
LM_SUM_HD bool table_in_lds(size_t staged_bytes, size_t m, size_t k) { return staged_bytes + m * k * sizeof(u64) <= kExpectLdsBytes; }

// The reducer of the Walker: the walk's events are all this route needs of it (which record a window lies in and whether
// it is inside); the weights of the windows do not go through slots of a record.
struct ExpectReducer {
    typedef u64 Slot;
    template <typename Job>
    LM_SUM_HD void begin(const Job &)
    {
    }
    LM_SUM_HD void window(u64, float, bool) {}
    LM_SUM_HD void flush(Slot *, u64, u64, u64) {}
};

// One lane's run: rows [r0, r1) of column `col`.  Every window is summed from scratch over its M symbols (w: M x K
// row-major) and, when it lies inside a record and its weight is not 0, its M symbols are read again and `add(j * K +
// symbol, q)` is called for each.  The gain of a record is fetched when the walk enters it.  Rows up to r1 + M - 2 are
// read: the wrap rows behind the column.
template <typename Add>
LM_SUM_HD void expect_run(const uint8_t *seq, const u64 stride, const u64 rows, const u64 col, const u64 r0, const u64 r1,
                          const unsigned M, const unsigned K, const float *w, const u64 *off, const u64 n, const double *gains,
                          const float scale, const double unit, Add add)
{
    Walker<ExpectReducer> wk;
    wk.off = off;
    wk.n = n;
    wk.m = M;
    wk.slots = nullptr;
    wk.begin(col * rows + r0, 0);
    u64 rec = kNoEnd;  // whose gain `g` is
    double g = 0.0;
    const uint8_t *sp = seq + col;
    for (u64 row = r0; row < r1; ++row) {
        const uint8_t *s = sp + row * stride;
        float v = 0.0f;
        for (unsigned j = 0; j < M; ++j)
            v = v + w[j * K + s[j * stride]];
        wk.take(col * rows + row, v);
        if (!wk.competing || wk.rec >= n)
            continue;
        if (wk.rec != rec) {
            rec = wk.rec;
            g = gains[rec];
        }
        const u64 q = quantum(v, scale, g, unit);
        if (q == 0)
            continue;
        for (unsigned j = 0; j < M; ++j)
            add(j * K + s[j * stride], q);
    }
}

}  // namespace setexpect
}  // namespace lm
