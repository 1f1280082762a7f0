// The host arithmetic of the host-pointer path (lightmotif_amd/csrc/host_plan.hpp): the tile shape of a large call, the
// piece size, the cpulist parser, the two digests and the crossover of the cost model.  A stand-alone program (no device,
// no HIP call), built by tests/test_cpp_host_plan.py with the address and undefined-behaviour sanitizers.  The expected
// values are worked out by hand from the constants (32 MB tiles, 4 MB smallest tile, a twelfth of the matrix per tile).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "host_plan.hpp"

using namespace lm::host;

static long g_checks = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        ++g_checks;                                                  \
        if (!(cond)) {                                               \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                            \
            fprintf(stderr, "\n");                                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// ---- plan_tiles, piece_rows ---------------------------------------------------------------------------------------------

// the tile arithmetic spelled out a second time, expression by expression: what plan_tiles is held against over the sweep
static TilePlan tiles_restated(size_t nrows, size_t cols, size_t elem, size_t seq_stride, size_t halo, size_t tile_bytes)
{
    const size_t row_bytes = cols * elem;
    const size_t target = std::min(tile_bytes, std::max(kPipeMinTileBytes, nrows * row_bytes / 12));
    size_t tr = std::min(target / row_bytes, (2 * tile_bytes) / seq_stride);
    tr = std::max<size_t>(tr / 256 * 256, 256);
    const size_t in_tile = ((tr + halo) * seq_stride + 255) / 256 * 256, out_tile = (tr * row_bytes + 255) / 256 * 256;
    bool fits = true;
    if (tr * row_bytes > tile_bytes)
        fits = false;
    return {tr, in_tile, out_tile, (nrows + tr - 1) / tr, fits};
}

static void test_plan_tiles()
{
    const size_t tile = 32u << 20;
    CHECK(kTileBytes == tile && kPipeMinTileBytes == (4u << 20) && kPipeMinOutBytes == (96u << 20), "size constants moved");
    CHECK(kZeroCopyBytes == (128u << 10) && kKeepBytes == (256u << 20), "size constants moved");
    TilePlan p = plan_tiles(31250000, 32, 4, 32, 19, tile);  // 1 Gbp, f32
    CHECK(p.tr == 262144 && p.ntiles == 120 && p.out_tile == 33554432 && p.in_tile == 8389376 && p.fits, "%zu %zu %zu %zu",
          p.tr, p.ntiles, p.out_tile, p.in_tile);
    CHECK(p.in_tile == ((size_t)(262144 + 19) * 32 + 255) / 256 * 256 && p.in_tile % 256 == 0, "%zu", p.in_tile);
    p = plan_tiles(786432, 32, 4, 32, 19, tile);  // the smallest pipelined f32 call: 96 MB of scores
    CHECK(786432u * 32 * 4 == kPipeMinOutBytes && p.tr == 65536 && p.ntiles == 12 && p.fits, "%zu %zu", p.tr, p.ntiles);
    p = plan_tiles(3145728, 32, 1, 32, 14, tile);  // u8 with 96 MB of scores
    CHECK(3145728u * 32 == kPipeMinOutBytes && p.tr == 262144 && p.ntiles == 12 && p.fits, "%zu %zu", p.tr, p.ntiles);
    p = plan_tiles(1024, 32768, 4, 32768, 19, tile);  // the widest shape that fits: 256 rows fill one slot exactly (>, not >=)
    CHECK(p.tr == 256 && p.out_tile == tile && p.tr * 32768 * 4 == tile && p.fits && p.ntiles == 4, "%zu %zu", p.tr, p.out_tile);
    p = plan_tiles(700, 40000, 4, 40000, 19, tile);  // ... and one that does not: the LM_HIP_ERR_CAPACITY fall-back
    CHECK(p.tr == 256 && !p.fits, "%zu", p.tr);
    p = plan_tiles(1024, 32769, 4, 32800, 0, tile);
    CHECK(!p.fits, "one column beyond the widest shape");

    long swept = 0;
    for (size_t cols : {1, 16, 20, 32, 40})
        for (size_t elem : {1, 4})
            for (size_t halo : {0, 14, 127})
                for (size_t seq_stride : {cols, (cols + 31) / 32 * 32}) {
                    const size_t rb = cols * elem;
                    std::vector<size_t> edges = {1, 256, 257, (48u << 20) / rb, kPipeMinOutBytes / rb, (384u << 20) / rb,
                                                 (2 * tile) / seq_stride, 31250000};
                    for (size_t e : std::vector<size_t>(edges)) {  // ... and whole tiles of what each edge gives
                        const size_t tr = tiles_restated(e, cols, elem, seq_stride, halo, tile).tr;
                        edges.push_back(tr);
                        edges.push_back(12 * tr);
                    }
                    for (size_t e : edges)
                        for (size_t nrows : {e - 1, e, e + 1}) {
                            if (nrows == 0)
                                continue;
                            const TilePlan a = plan_tiles(nrows, cols, elem, seq_stride, halo, tile);
                            const TilePlan b = tiles_restated(nrows, cols, elem, seq_stride, halo, tile);
                            CHECK(a.tr == b.tr && a.in_tile == b.in_tile && a.out_tile == b.out_tile && a.ntiles == b.ntiles &&
                                      a.fits == b.fits,
                                  "nrows %zu cols %zu elem %zu stride %zu halo %zu", nrows, cols, elem, seq_stride, halo);
                            // what the pipeline relies on: whole 256-row tiles that cover the rows, slots that hold a tile
                            CHECK(a.tr % 256 == 0 && a.ntiles * a.tr >= nrows && (a.ntiles - 1) * a.tr < nrows, "cover");
                            CHECK(a.in_tile >= (a.tr + halo) * seq_stride && a.out_tile >= a.tr * rb && a.fits, "slots");
                            ++swept;
                        }
                }
    CHECK(swept > 2000, "%ld", swept);

    CHECK(piece_rows(32, 4) == 524288, "%zu", piece_rows(32, 4));
    CHECK(piece_rows(32, 1) == 2097152, "%zu", piece_rows(32, 1));
    CHECK(piece_rows((size_t)1 << 26, 4) == 1, "a row wider than a piece is still one row, never none");
}

// ---- parse_cpulist ------------------------------------------------------------------------------------------------------

static void expect_cpus(const char *text, bool want_any, std::initializer_list<int> want)
{
    cpu_set_t set;
    memset(&set, 0xff, sizeof set);  // whatever was there is cleared
    CHECK(parse_cpulist(text, &set) == want_any, "\"%s\"", text);
    CHECK(CPU_COUNT(&set) == (int)want.size(), "\"%s\": %d CPUs", text, CPU_COUNT(&set));
    for (int c : want)
        CHECK(CPU_ISSET(c, &set), "\"%s\": CPU %d missing", text, c);
}

static void test_parse_cpulist()
{
    expect_cpus("0-3,8\n", true, {0, 1, 2, 3, 8});
    expect_cpus("", false, {});
    expect_cpus("abc", false, {});
    expect_cpus("5-", false, {});
    expect_cpus("3,", true, {3});
    expect_cpus("7-3", false, {});
    expect_cpus("1020-1030", true, {1020, 1021, 1022, 1023});  // clipped at CPU_SETSIZE
    CHECK(CPU_SETSIZE == 1024, "%d", (int)CPU_SETSIZE);
    cpu_set_t set;
    CHECK(parse_cpulist("0-63,128-191", &set) && CPU_COUNT(&set) == 128, "%d", CPU_COUNT(&set));
    CHECK(CPU_ISSET(63, &set) && !CPU_ISSET(64, &set) && !CPU_ISSET(127, &set) && CPU_ISSET(128, &set) && CPU_ISSET(191, &set) &&
              !CPU_ISSET(192, &set),
          "range ends");
}

// ---- sample_digest --------------------------------------------------------------------------------------------------------

static float pattern(size_t i)
{
    return (float)((i * 2654435761u) % 1000003u) * 0.25f - 1000.0f;
}

static void test_sample_digest()
{
    struct Shape {
        size_t rows, cols, stride;
    };
    for (const Shape &s : {Shape{1, 1, 1}, Shape{3, 5, 8}, Shape{1, 67, 67}, Shape{4, 17, 17}, Shape{1000, 32, 40}}) {
        // exactly up to the last cell: a read of the padding behind it is a heap overflow the sanitizer reports
        std::vector<float> m((s.rows - 1) * s.stride + s.cols);
        for (size_t i = 0; i < m.size(); ++i)
            m[i] = pattern(i);
        const uint64_t h = sample_digest(m.data(), s.rows, s.stride, s.cols);
        CHECK(h == sample_digest(m.data(), s.rows, s.stride, s.cols), "deterministic");
        std::vector<float> c = m;
        c[0] += 1.0f;
        CHECK(sample_digest(c.data(), s.rows, s.stride, s.cols) != h, "%zu x %zu: first cell", s.rows, s.cols);
        c = m;
        c.back() += 1.0f;
        CHECK(sample_digest(c.data(), s.rows, s.stride, s.cols) != h, "%zu x %zu: last cell", s.rows, s.cols);
        if (s.rows == 1000) {  // cell 1 is not one of the 67 samples of 32 000 cells; the padding never is
            c = m;
            c[1] += 1.0f;
            c[32] = c[39] = 5e8f;
            CHECK(sample_digest(c.data(), s.rows, s.stride, s.cols) == h, "an unsampled cell or the padding was read");
        }
        if (s.stride == s.cols && s.rows != s.cols)  // the same bits as cols x rows
            CHECK(sample_digest(m.data(), s.cols, s.rows, s.rows) != h, "%zu x %zu against its transpose's shape", s.rows, s.cols);
        c = m;
        c[0] = 0.0f;
        const uint64_t h0 = sample_digest(c.data(), s.rows, s.stride, s.cols);
        c[0] = -0.0f;  // by bit pattern
        CHECK(sample_digest(c.data(), s.rows, s.stride, s.cols) != h0, "-0.0f against 0.0f");
    }
    std::vector<float> m(15);
    for (size_t i = 0; i < m.size(); ++i)
        m[i] = pattern(i);
    CHECK(sample_digest(m.data(), 3, 5, 5) != sample_digest(m.data(), 5, 3, 3), "3 x 5 against 5 x 3 over the same bits");
    CHECK(sample_digest(nullptr, 0, 32, 32) == sample_digest(nullptr, 0, 40, 32), "no cell, nothing read");
}

// ---- hash_weights ---------------------------------------------------------------------------------------------------------

static void test_hash_weights()
{
    const size_t m = 4, k = 5, stride = 8;
    std::vector<float> a((m - 1) * stride + k), dense(m * k);
    for (size_t j = 0; j < m; ++j)
        for (size_t s = 0; s < k; ++s)
            a[j * stride + s] = dense[j * k + s] = pattern(j * k + s);
    std::vector<float> b = a;
    for (size_t j = 0; j + 1 < m; ++j)
        for (size_t s = k; s < stride; ++s) {
            a[j * stride + s] = 1.0f;
            b[j * stride + s] = -7.5f;
        }
    const uint64_t h = hash_weights(a.data(), m, stride, k);
    CHECK(h == hash_weights(b.data(), m, stride, k) && h == hash_weights(dense.data(), m, k, k), "the row padding was hashed");
    uint32_t bits;
    memcpy(&bits, &b[2 * stride + 3], 4);
    bits ^= 1u;
    memcpy(&b[2 * stride + 3], &bits, 4);
    CHECK(hash_weights(b.data(), m, stride, k) != h, "one bit");
    CHECK(hash_weights(dense.data(), m, k, k) != hash_weights(dense.data(), k, m, m), "4 x 5 against 5 x 4 over the same bytes");
}

// ---- crossover_cells ------------------------------------------------------------------------------------------------------

static void test_crossover_cells()
{
    CHECK(kCrossoverMargin == 1.25, "%f", kCrossoverMargin);
    CHECK(crossover_cells(kCostScoreF32, 1) == SIZE_MAX, "0.0316 is at most 0.093 * 1.25");
    CHECK(crossover_cells(kCostScoreF32, 4) == 1407186, "%zu", crossover_cells(kCostScoreF32, 4));
    CHECK(crossover_cells(kCostScoreF32, 15) == 123360, "%zu", crossover_cells(kCostScoreF32, 15));
    const HostCost edge{47.0, 0.5, 0.625, 0.0};  // cpu_ns == gpu_ns * 1.25, both exact in binary: <=
    CHECK(edge.cpu_ns == edge.gpu_ns * kCrossoverMargin && crossover_cells(edge, 7) == SIZE_MAX, "the margin itself stays");
    const HostCost above{47.0, 0.5, 0.625, 0.125};
    CHECK(crossover_cells(above, 1) == 188001, "%zu", crossover_cells(above, 1));  // 47 000 / 0.25 + 1
    const HostCost slow{1e18, 0.5, 0.75, 0.0};  // 1e21 / 0.25 cells: beyond a size_t
    CHECK(crossover_cells(slow, 0) == SIZE_MAX, "%zu", crossover_cells(slow, 0));
}

int main()
{
    test_plan_tiles();
    test_parse_cpulist();
    test_sample_digest();
    test_hash_weights();
    test_crossover_cells();
    printf("test_host_plan: all checks passed (%ld)\n", g_checks);
    return 0;
}
