// The expected site counts of a set (lightmotif_amd/csrc/seqset_expect_plan.hpp: the fixed point, the weight of a window,
// the run of a lane) on the host, driven by the Walker of seqset_walk.hpp exactly as the kernel drives it, with the LDS
// atomics replaced by plain adds, against brute-force loops over the offsets table.  A stand-alone program (no device, no
// HIP call), built by tests/test_cpp_seqset_expect.py with the address and undefined-behaviour sanitizers.
//
// Every (rows, cols, T, M, K) of a small grid; record layouts whose junctions fall on run and column boundaries, with
// empty records sharing such an offset, records shorter than M and of exactly M, records over several runs, one record
// that fills the set; gains of 0, powers of two and gains that clamp; weights that are small integers (every weight of a
// window is then exact) with NaN and infinities planted.  Checked: the table of the walk equals the brute-force table,
// cell for cell, with the lanes in ascending and in descending order; every row of a table has the same total; the fixed
// point of a set; the weight of the special scores.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "seqset_expect_plan.hpp"

using namespace lm;
using namespace lm::setexpect;

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

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()  // xorshift64*
{
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}

struct Case {
    u64 rows, cols, T, m, k;
    std::vector<u64> off;         // n + 1
    std::vector<uint8_t> text;    // rows * cols symbols of the concatenation (the default symbol behind the last record)
    std::vector<float> w;         // m x k
    std::vector<double> gains;    // n
    float scale;
};

struct PlainAdd {
    u64 *tab;
    u64 cells;
    void operator()(unsigned cell, u64 q) const
    {
        CHECK(cell < cells, "cell %u of %llu", cell, cells);
        tab[cell] += q;
    }
};

// the striped matrix: symbol p at row p % rows, column p / rows; wrap rows repeat the top of the next column
static std::vector<uint8_t> stripe(const Case &c, u64 wrap, u64 stride)
{
    std::vector<uint8_t> mat((c.rows + wrap) * stride, (uint8_t)(c.k - 1));
    for (u64 col = 0; col < c.cols; ++col)
        for (u64 row = 0; row < c.rows + wrap; ++row) {
            const u64 p = col * c.rows + row;
            if (row < c.rows || col + 1 < c.cols)
                mat[row * stride + col] = p < c.text.size() ? c.text[p] : (uint8_t)(c.k - 1);
        }
    return mat;
}

static std::vector<u64> walk_table(const Case &c, bool descending, int F)
{
    const u64 n = c.off.size() - 1, stride = c.cols + 3, wrap = c.m ? c.m - 1 : 0;
    const std::vector<uint8_t> mat = stripe(c, wrap, stride);
    std::vector<u64> tab(c.m * c.k, 0);
    const u64 streams = (c.rows + c.T - 1) / c.T, lanes = streams * c.cols;
    for (u64 i = 0; i < lanes; ++i) {
        const u64 lane = descending ? lanes - 1 - i : i;
        const u64 col = lane % c.cols, r0 = (lane / c.cols) * c.T;
        const u64 r1 = r0 + c.T < c.rows ? r0 + c.T : c.rows;
        expect_run(mat.data(), stride, c.rows, col, r0, r1, (unsigned)c.m, (unsigned)c.k, c.w.data(), c.off.data(), n, c.gains.data(), c.scale,
                   pow2_of(F), PlainAdd{tab.data(), c.m * c.k});
    }
    return tab;
}

static std::vector<u64> brute_table(const Case &c, int F, u64 *row_total)
{
    const u64 n = c.off.size() - 1;
    std::vector<u64> tab(c.m * c.k, 0);
    *row_total = 0;
    for (u64 r = 0; r < n; ++r)
        for (u64 p = c.off[r]; p + c.m <= c.off[r + 1]; ++p) {
            float v = 0.0f;
            for (u64 j = 0; j < c.m; ++j)
                v = v + c.w[j * c.k + c.text[p + j]];
            if (!(v == v))
                continue;
            const double zz = std::exp2((double)(c.scale * v)) * c.gains[r];  // (integer scores, an integer scale: exact)
            if (!(zz == zz))
                continue;
            const u64 q = (u64)std::nearbyint((zz < 1.0 ? zz : 1.0) * std::ldexp(1.0, F));
            *row_total += q;
            for (u64 j = 0; j < c.m; ++j)
                tab[j * c.k + c.text[p + j]] += q;
        }
    return tab;
}

static void check_case(const Case &c)
{
    const int F = frac_bits_of(c.off.back());
    u64 total;
    const std::vector<u64> want = brute_table(c, F, &total);
    for (int descending = 0; descending < 2; ++descending) {
        const std::vector<u64> got = walk_table(c, descending, F);
        for (u64 i = 0; i < want.size(); ++i)
            CHECK(got[i] == want[i], "cell [%llu][%llu] (rows %llu cols %llu T %llu M %llu K %llu descending %d): %llu, want %llu", i / c.k, i % c.k,
                  c.rows, c.cols, c.T, c.m, c.k, descending, got[i], want[i]);
        for (u64 j = 0; j < c.m; ++j) {
            u64 sum = 0;
            for (u64 s = 0; s < c.k; ++s)
                sum += got[j * c.k + s];
            CHECK(sum == total, "row %llu sums to %llu, the windows weigh %llu", j, sum, total);
        }
    }
}

static Case make_case(u64 rows, u64 cols, u64 T, u64 m, u64 k, int layout)
{
    Case c{rows, cols, T, m, k, {0}, {}, {}, {}, 1.0f};
    const u64 positions = rows * cols;
    auto push = [&](u64 end) {
        end = end < positions ? end : positions;
        c.off.push_back(end < c.off.back() ? c.off.back() : end);
    };
    if (layout == 0) {  // junctions on the run boundaries of the first column and on every column boundary, empties there
        push(0);        // an empty record at the start
        for (u64 r0 = T; r0 < rows && c.off.size() < 12; r0 += T) {
            push(r0);
            push(r0);
            push(r0);
        }
        for (u64 col = 1; col <= cols; ++col) {
            push(col * rows);
            if (col % 2)
                push(col * rows);  // (the last one: an empty record at the end)
        }
    } else if (layout == 1) {  // one record that fills the set
        push(positions);
    } else if (layout == 2) {  // shorter than M, exactly M, over three runs and more
        push(m - 1);
        push(c.off.back() + m);
        push(c.off.back() + 3 * T + m + 1);
        push(c.off.back() + 1);
        push(c.off.back() + rows + 2 * T);
        while (c.off.back() + 3 < positions)
            push(c.off.back() + rnd() % (2 * m + 2));
    } else {  // random lengths; the last record ends short of the layout: the tail of the last column is padding
        while (c.off.back() + 2 < positions && c.off.size() < 400) {
            const u64 pick = rnd() % 6;
            const u64 len = pick == 0 ? 0 : pick == 1 ? rnd() % m : pick == 2 ? m : pick == 3 ? T + rnd() % (m + 1) : pick == 4 ? rows - 1 + rnd() % 3 : rnd() % (3 * T + 1);
            push(std::min(c.off.back() + len, positions - 2));
        }
    }
    c.text.resize(positions);
    for (u64 p = 0; p < positions; ++p)
        c.text[p] = p < c.off.back() ? (uint8_t)(rnd() % k) : (uint8_t)(k - 1);
    c.w.resize(m * k);
    const float inf = std::numeric_limits<float>::infinity();
    for (float &x : c.w) {
        const u64 r = rnd();
        x = r % 97 == 0 ? std::numeric_limits<float>::quiet_NaN() : r % 89 == 0 ? inf : r % 83 == 0 ? -inf : (float)((long long)(r % 7) - 3);
    }
    c.scale = layout % 2 ? 2.0f : 1.0f;
    const u64 n = c.off.size() - 1;
    c.gains.resize(n);
    for (u64 r = 0; r < n; ++r) {
        const u64 x = rnd() % 8;
        c.gains[r] = x == 0 ? 0.0 : x == 1 ? 1024.0 : std::ldexp(1.0, -(int)(rnd() % 12));  // off, clamping, 2^-k
    }
    return c;
}

static void check_rule()
{
    CHECK(frac_bits_of(0) == 40 && frac_bits_of(1) == 40 && frac_bits_of((1ull << 22) - 1) == 40 && frac_bits_of(1ull << 22) == 39, "F of small sets");
    CHECK(frac_bits_of(1ull << 40) == 21 && frac_bits_of(~0ull) == 0, "F of large sets");
    for (int b = 1; b < 63; ++b) {
        const u64 N = (1ull << b) - 1;  // the most windows of weight 1 a cell can sum
        const int F = frac_bits_of(N);
        CHECK(F >= 0 && (F == 0 || b + F <= 62), "N of %d bits: F %d overflows a cell", b, F);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double unit = pow2_of(40);
    CHECK(quantum(nan, 1.0f, 1.0, unit) == 0, "a NaN score contributes nothing");
    CHECK(quantum(inf, 1.0f, 0.0, unit) == 0, "+inf * 0 contributes nothing");
    CHECK(quantum(inf, 1.0f, 0.5, unit) == 1ull << 40, "+inf clamps to 1");
    CHECK(quantum(-inf, 1.0f, 1e300, unit) == 0, "-inf contributes 0");
    CHECK(quantum(3.0f, 1.0f, 1.0, unit) == 1ull << 40, "the clamp at 1");
    CHECK(quantum(-3.0f, 1.0f, 0.5, unit) == 1ull << 36, "2^-3 * 2^-1");
    CHECK(quantum(-41.0f, 1.0f, 1.0, unit) == 0 && quantum(-40.0f, 1.0f, 1.0, unit) == 1, "half a quantum rounds to even, a whole one stays");
    CHECK(quantum(-40.0f, 1.0f, 1.5, unit) == 2 && quantum(-40.0f, 1.0f, 2.5, unit) == 2, "ties go to even");
    CHECK(quantum(-2.0f, 2.0f, 8.0, unit) == 1ull << 39, "the scale multiplies the score");
    CHECK(table_in_lds(0, 70, 5) && table_in_lds(kExpectLdsBytes - 40, 1, 5) && !table_in_lds(kExpectLdsBytes - 39, 1, 5), "the table's place in LDS");
}

int main()
{
    check_rule();
    const u64 rows_[] = {1, 7, 16, 45}, cols_[] = {1, 3, 8}, ts[] = {1, 7, 64}, ms[] = {1, 4, 17};
    for (const u64 rows : rows_)
        for (const u64 cols : cols_)
            for (const u64 T : ts)
                for (const u64 m : ms)
                    for (int layout = 0; layout < 4; ++layout)
                        check_case(make_case(rows, cols, T, m, layout % 2 ? 21 : 5, layout));
    printf("test_seqset_expect: all checks passed (%ld checks)\n", g_checks);
    return 0;
}
