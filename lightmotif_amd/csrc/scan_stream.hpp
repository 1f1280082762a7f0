// scan_stream.hpp -- the stream skeleton every discrete scan kernel shares, defined once.
//
// A scan cuts rows [row_begin, row_end) into `nstreams` streams of T output rows, one per half-wave.  A stream walks its
// rows in GROUPS of `step` input rows (the padded motif length of the one-symbol scans, the ring of the pair scans):
// the FIRST group only fills the accumulators and completes `first` rows (1; the pair scans 2), every later group
// completes `step` rows, so
//     T = q * step + first          q >= 1, in q + 1 groups.
// The threshold scans remember which groups saw a flagged sum in at most 64 NOTES of G consecutive groups each, and
// hand the rows of the flagged notes to the exact re-scoring.
//
// Two layers.  The GEOMETRY is plain C++17 (constexpr, no HIP builtin): the planner (score_plan.hip) takes a stream's
// length from the same StreamGeom the kernels take their group count and row ranges from, and
// tests/cpp/test_scan_stream.cpp checks it on the host.  The DEVICE layer places a half-wave on its stream, requests a
// block scan's first symbol blocks, turns flagged notes into candidate rows and launches a scan.
//
// What is NOT here, although every threshold scan has it: the three lines that count groups into notes (ngroups in 32
// bits, G, `if (--gleft == 0)`), the byte-load prologue, the FIRST / MAIN / LAST walk and the pick of a batch's job.
// Each was tried as a helper and changed the instructions of the kernels that used it; a copy names the others.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lm {

// ---- geometry ---------------------------------------------------------------------------------------------------

// (always inlined, like the kernels' own helpers)
#define LM_GEOM_INLINE __attribute__((always_inline))

// padded motif length of the one-symbol scans: even (two accumulators per register); a multiple of 4 for wide alphabets,
// whose scan fetches symbols in 4-row blocks that must not straddle a group (score_prefilter_blk.hpp) -- every user of
// a wide image shares that geometry
constexpr int prefilter_mp(int m, int wide = 0) { return wide ? (m + 3) / 4 * 4 : (m + 1) / 2 * 2; }
// pair scans: padded length M' = 3 (mod 4) and the input rows per group, M' + 1 (score_prefilter2.hpp)
constexpr int prefilter2_mo(int m) { return m | 3; }
constexpr int prefilter2_ring(int m) { return prefilter2_mo(m) + 1; }

// what the planner takes a stream's length from, picked per kernel family below
struct StreamGeom {
    int step;   // input rows per group = rows completed by every group but the first
    int first;  // rows completed by the FIRST group
    LM_GEOM_INLINE constexpr unsigned long long rows(unsigned long long q) const { return q * (unsigned long long)step + (unsigned long long)first; }
};

// The kernels' side of the same rule, with the geometry as template arguments (GEOM.step, GEOM.first of a constexpr
// StreamGeom): the constants stand in the functions' own bodies, where the compiler folds them before it inlines.
//
// groups of a stream of T = rows(q) rows: q + 1, in the integer type of `T` (the threshold scans count in 32 bits,
// T <= 2^30).  Exact because 1 <= FIRST <= STEP.  (FIRST == 1 rounds up instead of stepping back: the same quotient,
// and the form the byte-load scans were measured with -- in 64 bits the other one costs score_c32_u8 its countdown loop.)
template <int STEP, int FIRST, typename N>
LM_GEOM_INLINE constexpr N stream_groups(N T)
{
    static_assert(1 <= FIRST && FIRST <= STEP, "the FIRST group completes at most a group's rows");
    if constexpr (FIRST == 1)
        return (T + (N)(STEP - 1)) / (N)STEP;
    else
        return (T - (N)FIRST) / (N)STEP + (N)1;
}
// Note `bit` covers groups [bit * G, (bit + 1) * G) of a stream of `ngroups` groups and T rows.  Group 0 completes
// the stream's rows 0 .. FIRST - 1, group g >= 1 the rows (g - 1) * STEP + FIRST .. g * STEP + FIRST - 1.  The
// stream's first row is `first_row` (relative to row_begin); it OWNS the rows from `own_row` on -- the last
// stream is shifted back onto rows of its neighbour and must not report those twice.  -> rows [r0, r1), empty
// (r1 <= r0) for a note that lies wholly before own_row.
template <int STEP, int FIRST>
LM_GEOM_INLINE constexpr void note_rows(int bit, unsigned G, unsigned ngroups, unsigned long long T, long long first_row, long long own_row,
                                        long long &r0, long long &r1)
{
    const unsigned long long g0 = (unsigned long long)bit * G;
    unsigned long long g1 = g0 + G;
    if (g1 > ngroups)
        g1 = ngroups;
    const long long i0 = g0 == 0 ? 0 : (long long)((g0 - 1) * STEP + FIRST);
    long long i1 = (long long)((g1 - 1) * STEP + FIRST);
    if (i1 > (long long)T)
        i1 = (long long)T;
    r0 = first_row + i0;
    if (r0 < own_row)
        r0 = own_row;
    r1 = first_row + i1;
}
constexpr StreamGeom one_symbol_geom(int m, int wide = 0) { return StreamGeom{prefilter_mp(m, wide), 1}; }
constexpr StreamGeom pair_geom(int m) { return StreamGeom{prefilter2_ring(m), 2}; }

LM_GEOM_INLINE constexpr unsigned groups_per_note(unsigned ngroups) { return (ngroups + 63u) / 64u; }  // G: at most 64 notes per stream
LM_GEOM_INLINE constexpr unsigned notes(unsigned ngroups) { return (ngroups + groups_per_note(ngroups) - 1u) / groups_per_note(ngroups); }

// One bit per NOTE (= G groups of a stream), up to 64 per stream, collected without a compare AND without a 64-bit shift by
// a register (score_prefilter.hpp, prefilter_lookahead: such a shift by the last allocated VGPR is what broke the protein scans): the field shifts right one bit per
// note and takes the note's flag in at bit 63, so after n notes they sit in its top n bits, oldest lowest.
struct GroupNotes {
    unsigned lo = 0, hi = 0;
    // `mx`: bit 15 of a half = that half reached the threshold (the pair scans' biased sums, score_prefilter2.hpp: kFlagBits)
    __host__ __device__ __forceinline__ void note(unsigned &mx)
    {
        const unsigned either = mx | (mx << 16);  // bit 31: one of the two halves reached the threshold
        push(either);
        mx = 0;
    }
    __host__ __device__ __forceinline__ void push(const unsigned flag31)  // bit 31 of `flag31` = the note's flag
    {
#if defined(__HIP_DEVICE_COMPILE__)
        lo = __builtin_amdgcn_alignbit(hi, lo, 1);  // (hi:lo) >> 1
#else
        lo = (lo >> 1) | (hi << 31);
#endif
        hi = (hi >> 1) | (flag31 & 0x80000000u);
    }
    __host__ __device__ __forceinline__ unsigned long long finish(unsigned n) const  // n = notes taken, 1 ... 64 (wave-uniform)
    {
        // (hi:lo) >> (64 - n) with 32-bit operations only
        const unsigned sh = 64u - n;
        const unsigned a = sh >= 32u ? hi : lo, b = sh >= 32u ? 0u : hi, r = sh & 31u;
        const unsigned out_lo = r ? (a >> r) | (b << (32u - r)) : a;
        const unsigned out_hi = r ? (b >> r) : b;
        return ((unsigned long long)out_hi << 32) | out_lo;
    }
};

// ---- device -----------------------------------------------------------------------------------------------------

constexpr int kBlock = 256;                      // threads per workgroup (4 wavefronts)
constexpr int kStreamsPerBlock = kBlock / 32;    // 2 per wavefront

// The half-wave's stream and its first output row.  Half-waves beyond the last stream re-do it (`idle`: same reads, and
// they report nothing); the last stream is shifted back so that it ends at row_end and overlaps its neighbour.
struct StreamPlace {
    unsigned long long stream, o0;
    bool idle;
};
__device__ __forceinline__ StreamPlace place_stream(const unsigned long long row_begin, const unsigned long long row_end,
                                                    const unsigned long long T, const unsigned long long nstreams)
{
    const int lane = threadIdx.x & 63;
    unsigned long long stream =
        ((unsigned long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 2 + (lane >> 5);
    const bool idle = stream >= nstreams;
    if (idle)
        stream = nstreams - 1;
    unsigned long long o0 = row_begin + stream * T;
    if (o0 + T > row_end)
        o0 = row_end - T;
    return StreamPlace{stream, o0, idle};
}

// A flagged note's candidate rows, in the form emit_candidates takes (note_rows)
template <int STEP, int FIRST>
struct GroupRows {
    unsigned G, ngroups;
    long long first_row, own_row;
    unsigned long long T;
    __device__ __forceinline__ void operator()(const int bit, long long &r0, long long &r1) const
    {
        note_rows<STEP, FIRST>(bit, G, ngroups, T, first_row, own_row, r0, r1);
    }
};

// Prologue of the block scans: blocks 0 .. PFB - 1 of the (zeroed) ring of 4-row symbol blocks requested.  `spq` = the
// lane's dword of block 0, `in0` the stream's first padded input row, `brow` the lane's row of a block.  A lane whose
// row lies before the matrix skips the load (its "symbols" read as 0, a valid table row); SHIFT > 3: block 1 may
// start before the matrix too.
template <int NB, int PFB, int SHIFT>
__device__ __forceinline__ void block_prologue(unsigned (&blk)[NB], const uint8_t *spq, const long long in0, const int brow)
{
    if (in0 + (long long)brow >= 0)
        blk[0] = *reinterpret_cast<const unsigned *>(spq);
#pragma unroll
    for (int j = 1; j < PFB; ++j)
        if (4 * j >= SHIFT || in0 + 4 * j + (long long)brow >= 0)
            blk[j] = *reinterpret_cast<const unsigned *>(spq + j * 128);
}

// ---- host: the launch shim of every scan kernel ---------------------------------------------------------------------
// (its address converts to the family's launcher type, which fixes A...: score_registry.hpp)
template <auto KERNEL, class... A>
hipError_t launch_scan(dim3 grid, size_t lds_bytes, hipStream_t stream, A... args)
{
    hipLaunchKernelGGL(KERNEL, grid, dim3(kBlock), lds_bytes, stream, args...);
    return hipGetLastError();
}

}  // namespace lm
