// host_plan.hpp -- the host arithmetic of the host-pointer path (hostptr.hip, host_lane.hip, host_pipe.hip, host_cost.hip):
// size thresholds, the tile shape of a large call, the digests and the Dispatch::Hip cost model.  Pure functions, no HIP
// include: a host-only program compiles them (tests/cpp/test_host_plan.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include <sched.h>

namespace lm::host {

constexpr size_t kZeroCopyBytes = 128u << 10;   // tiniest calls: symbols / scores straight from / to pinned memory
constexpr size_t kKeepBytes = 256u << 20;       // staging buffers above this are released when the call ends
constexpr size_t kPipeMinOutBytes = 96u << 20;  // score matrices from here on take the tile pipeline (below, its ramp --
                                                // helper threads, one tile each of upload / read-back / copy-out latency --
                                                // costs more than the 15 % the pinned read-back gains: r04_host_pointer.json)
constexpr size_t kPipeMinTileBytes = 4u << 20;  // tiles: a twelfth of the score matrix, between this and a ring slot
constexpr size_t kTileBytes = 32u << 20;        // one tile of scores (and one pinned ring slot)

// Rows per tile of a large call: a ring slot (32 MB) of scores for genome-sized calls, smaller tiles for smaller calls --
// the pipeline's ramp is one tile each of upload, read-back and copy-out latency, a tile costs ~20 us of its own -- and
// at most two slots' worth of symbols.  `in_tile` / `out_tile`: bytes of one device slot of symbols / scores.
struct TilePlan {
    size_t tr, in_tile, out_tile, ntiles;
    bool fits;  // false: more than 32 K columns, not a shape the pipeline is for (the caller goes piece by piece)
};
inline TilePlan plan_tiles(size_t nrows, size_t cols, size_t elem, size_t seq_stride, size_t halo, size_t tile_bytes)
{
    const size_t row_bytes = cols * elem;
    const size_t target = std::min(tile_bytes, std::max(kPipeMinTileBytes, nrows * row_bytes / 12));
    size_t tr = std::min(target / row_bytes, (2 * tile_bytes) / seq_stride);
    tr = std::max<size_t>(tr / 256 * 256, 256);
    const size_t in_tile = ((tr + halo) * seq_stride + 255) / 256 * 256, out_tile = (tr * row_bytes + 255) / 256 * 256;
    return {tr, in_tile, out_tile, (nrows + tr - 1) / tr, !(tr * row_bytes > tile_bytes)};
}

// Rows per piece of a call that goes through the lane's own buffers: 64 MB of scores, one row at the least.
inline size_t piece_rows(size_t cols, size_t elem)
{
    return std::max<size_t>((64u << 20) / (cols * elem), 1);
}

// "0-63,128-191" -> cpu set
inline bool parse_cpulist(const char *text, cpu_set_t *set)
{
    CPU_ZERO(set);
    bool any = false;
    const char *p = text;
    while (*p) {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p)
            break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            if (end == p + 1)
                break;
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (c >= 0) {
                CPU_SET((int)c, set);
                any = true;
            }
        if (*p == ',')
            ++p;
        else
            break;
    }
    return any;
}

inline uint64_t hash_weights(const float *w, size_t m, size_t stride, size_t k)
{
    uint64_t h = 0xcbf29ce484222325ull ^ (m * 0x9E3779B97F4A7C15ull) ^ (k << 48);
    for (size_t j = 0; j < m; ++j)
        for (size_t s = 0; s < k; ++s) {
            uint32_t bits;
            memcpy(&bits, &w[j * stride + s], 4);
            h = (h ^ bits) * 0x100000001b3ull;
        }
    return h;
}

// 64 bits over the shape and 67 cells spread over the matrix (first, last, 65 in between), by bit pattern.
inline uint64_t sample_digest(const float *scores, size_t rows, size_t stride, size_t cols)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (rows * 0x100000001b3ull) ^ (cols << 32);
    const size_t cells = rows * cols;
    constexpr size_t kSamples = 67;
    for (size_t i = 0; i < kSamples && cells; ++i) {
        const size_t cell = cells <= kSamples ? i % cells : (size_t)((unsigned __int128)i * (cells - 1) / (kSamples - 1));
        uint32_t bits;
        memcpy(&bits, scores + (cell / cols) * stride + cell % cols, 4);
        h = (h ^ bits) * 0xff51afd7ed558ccdull;
        h ^= h >> 29;
    }
    return h;
}

// ---- the Dispatch::Hip policy: where a call on host matrices should go ------------------------------

// Cost model behind lm_hip_host_crossover, constants measured by tools/crossover.py (profiles/r05_crossover.json: MI355X on
// PCIe Gen5, 2 x EPYC 9575F; one CPU thread, as the reference gives a call):
//   GPU call  ~ t0 + g * cells     t0 = launch + synchronisation + copy set-up of the copy path (calls above 128 KB;
//                                  the zero-copy path below is cheaper but so is the CPU there), g = link bytes per cell
//   CPU tier  ~ c * cells          Score: c = c_row * M (AVX2 f32 permute / u8 shuffle kernels), reductions: one pass
// crossover = t0 / (c - g), never when the CPU's per-cell cost does not exceed the link's by a margin.
struct HostCost {
    double t0_us, gpu_ns, cpu_ns, cpu_ns_per_row;
};
//                                      t0 us  GPU ns/cell  CPU ns/cell  CPU ns/(cell x motif row)
constexpr HostCost kCostScoreF32{47.0, 0.093, 0.0, 0.0316};      // 1 B up + 4 B down; AVX2 f32 permute kernel (M = 4 ... 30 measured)
constexpr HostCost kCostScoreU8{60.0, 0.036, 0.0, 0.0071};       // 1 B up + 1 B down; AVX2 u8 shuffle kernel
constexpr HostCost kCostMaximumF32{37.0, 0.070, 0.247, 0.0};     // 4 B up; the Generic scan (the rule the variant keeps, pli/mod.rs:135-160)
constexpr HostCost kCostThresholdF32{63.0, 0.073, 0.252, 0.0};   // 4 B up; the default body (pli/mod.rs:210-221)
// Scanner: t0 and g measured (tests/cpp/test_dispatch --bench -> profiles/r05_scan_crossover.json: 29 us at 10 kbp, 41 at
// 100 kbp, 78 at 1 Mbp with the short form of the hit-list ordering; 46 / 49 / 85 before it); the CPU side is the reference's block loop on its AVX2 tier, PRICED from the u8 shuffle kernel + one pass of the
// vectorised u8 reductions -- the C++ port that stands in for it in the tests has scalar reductions (0.54 ns per cell: it
// crosses over at ~85 k cells); a Rust build should re-measure with its own tier (lm_hip_host_set_cpu_cost).
constexpr HostCost kCostScan{38.0, 0.044, 0.03, 0.0071};
constexpr double kCrossoverMargin = 1.25;  // the CPU must cost this much more per cell than the link before a call leaves it

inline size_t crossover_cells(const HostCost &k, size_t m)
{
    const double c = k.cpu_ns + k.cpu_ns_per_row * (double)m;
    if (c <= k.gpu_ns * kCrossoverMargin)
        return SIZE_MAX;
    const double cells = k.t0_us * 1e3 / (c - k.gpu_ns);
    return cells >= 9e18 ? SIZE_MAX : (size_t)cells + 1;
}

}  // namespace lm::host
