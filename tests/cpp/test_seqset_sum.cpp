// The sum of odds per record (lightmotif_amd/csrc/seqset_sum_plan.hpp: the run arithmetic, SumReducer, merge_record) on
// the host, driven by the Walker of seqset_walk.hpp the way the two kernel bodies drive it, against brute-force loops
// over the offsets table.  A stand-alone program (no device, no HIP call), built by tests/test_cpp_seqset_sum.py with the
// address and undefined-behaviour sanitizers.
//
// Every (rows, cols, T, M) of a small grid; record layouts whose junctions fall on run and column boundaries, with empty
// records sharing such an offset, records shorter than M, records that span three runs and more, and a set of one record.
// Checked: the run arithmetic against a sweep over the positions; that every (run, record) pair with a window has one
// target, the cell when the record has one run and the head or tail of that run otherwise; that with scores whose terms
// are exact powers of two every cell equals the direct sum, with the scratch poisoned beforehand and the lanes run in
// ascending and in descending order; and that with arbitrary scores a cell equals, bit for bit, the per-run partial sums
// added in ascending run order.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "seqset_sum_plan.hpp"
#include "seqset_walk.hpp"

using namespace lm;
using namespace lm::setsum;

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

struct HostLane {
    u64 index;
    u64 operator()() const { return index; }
};
typedef SumReducerT<HostLane> SumReducer;

struct HostJob {
    const float *dense;
    u64 slot_base, scratch_off;
    const u64 *offsets;
    Geometry geo;
    float scale;
    u64 lane_;
    HostLane lane_id() const { return HostLane{lane_}; }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Case {
    u64 rows, cols, T, m;
    std::vector<u64> off;      // n + 1
    std::vector<float> score;  // per position of the layout (rows * cols + m: the fused feed looks behind the last run)
};

// the sums of the walk: every lane of the layout in turn (`descending`: the last lane first), then the merge
static std::vector<double> walk_sums(const Case &c, const bool fused, const bool descending, const float scale)
{
    const u64 n = c.off.size() - 1, streams = streams_of(c.rows, c.T), runs = streams * c.cols;
    const Geometry geo{c.rows, c.T, streams, runs, (unsigned)c.cols, (unsigned)c.m};
    std::vector<double> block(n + 2 * runs, std::numeric_limits<double>::quiet_NaN());  // cells, then the scratch: poisoned
    for (u64 r = 0; r < n; ++r)
        block[r] = 0.0;  // (the launcher's memset)
    for (u64 i = 0; i < runs; ++i) {
        const u64 lane = descending ? runs - 1 - i : i;
        const u64 col = lane % c.cols, r0 = (lane / c.cols) * c.T;
        const u64 r1 = r0 + c.T < c.rows ? r0 + c.T : c.rows;
        const u64 p0 = col * c.rows + r0, p1 = col * c.rows + r1;
        const HostJob job{nullptr, 0, n, c.off.data(), geo, scale, lane};
        Walker<SumReducer> wk;
        wk.off = c.off.data();
        wk.n = n;
        wk.m = c.m;
        wk.slots = block.data();
        wk.begin(p0, job);
        const u64 run = run_of_lane(geo, wk.red.lane());
        CHECK(run == run_of(geo, p0) && run_begin(geo, run) == p0 && run_end(geo, run) == p1, "lane %llu owns [%llu, %llu), the plan says run %llu = [%llu, %llu)",
              lane, p0, p1, run, run_begin(geo, run), run_end(geo, run));
        if (fused) {
            const u64 total = (p1 - p0) + (c.m - 1);
            const long long base = (long long)p0 - (long long)(c.m - 1);
            for (u64 g = 0; g < total; g += c.m)
                for (u64 s = 0; s < c.m; ++s) {
                    const u64 t = g + s;
                    const bool live = t >= c.m - 1 && t < total;
                    const long long p = base + (long long)t;
                    wk.take((u64)p, p >= 0 && (u64)p < c.score.size() ? c.score[p] : 1.0f, live);
                }
        } else {
            for (u64 p = p0; p < p1; ++p)
                wk.take(p, c.score[p]);
        }
        wk.flush();
    }
    for (u64 r = 0; r < n; ++r) {
        double sum;
        if (merge_record(geo, block.data() + n, c.off[r], c.off[r + 1], &sum))
            block[r] = sum;
    }
    block.resize(n);
    return block;
}

static void check_case(const Case &c)
{
    const u64 n = c.off.size() - 1, streams = streams_of(c.rows, c.T), runs = streams * c.cols, positions = c.rows * c.cols;
    const Geometry geo{c.rows, c.T, streams, runs, (unsigned)c.cols, (unsigned)c.m};
    CHECK(c.off[n] <= positions, "the records do not fit the layout");
    // the run arithmetic: ascending, contiguous, every position in the run that begins at or before it
    u64 run = 0;
    for (u64 p = 0; p < positions; ++p) {
        while (run + 1 < runs && run_begin(geo, run + 1) <= p)
            ++run;
        CHECK(run_of(geo, p) == run && run_begin(geo, run) <= p && p < run_end(geo, run), "position %llu: run %llu, the sweep says %llu", p, run_of(geo, p), run);
    }
    CHECK(run == runs - 1 && run_end(geo, runs - 1) == positions && run_begin(geo, 0) == 0, "the runs do not tile the layout");
    for (u64 k = 0; k + 1 < runs; ++k)
        CHECK(run_end(geo, k) == run_begin(geo, k + 1), "run %llu ends at %llu, the next begins at %llu", k, run_end(geo, k), run_begin(geo, k + 1));
    for (u64 lane = 0; lane < runs; ++lane)
        CHECK(run_begin(geo, run_of_lane(geo, lane)) == (lane % c.cols) * c.rows + (lane / c.cols) * c.T, "lane %llu", lane);

    // every (run, record) with a window of the record in the run has exactly one target
    std::vector<double> exact(n, 0.0), ordered(n, 0.0);
    for (u64 r = 0; r < n; ++r) {
        const u64 start = c.off[r], end = c.off[r + 1];
        const u64 windows = end - start >= c.m ? end - start - c.m + 1 : 0;
        if (!windows) {
            for (u64 k = 0; k < runs; ++k)
                CHECK(flush_target(start, end, (unsigned)c.m, run_begin(geo, k), run_end(geo, k)) == kNone, "record %llu has no window", r);
            continue;
        }
        const u64 a = run_of(geo, start), b = run_of(geo, start + windows - 1);
        int cells = 0, heads = 0, tails = 0;
        std::vector<double> partial(b - a + 1, 0.0);
        for (u64 p = start; p < start + windows; ++p) {
            const float v = c.score[p];
            if (v == v)
                partial[run_of(geo, p) - a] += exp2_wide(v);
        }
        for (u64 k = a; k <= b; ++k) {
            const Target t = flush_target(start, end, (unsigned)c.m, run_begin(geo, k), run_end(geo, k));
            cells += t == kCell;
            heads += t == kHead;
            tails += t == kTail;
            CHECK(t == (a == b ? kCell : k == a ? kTail : kHead), "record %llu in run %llu of [%llu, %llu]: target %d", r, k, a, b, (int)t);
        }
        CHECK(cells == (a == b) && tails == (a != b) && heads == (int)(b - a), "record %llu: %d cells, %d heads, %d tails over runs [%llu, %llu]", r,
              cells, heads, tails, a, b);
        double sum = partial[0];
        for (u64 k = 1; k < partial.size(); ++k)
            sum += partial[k];
        ordered[r] = sum;
    }

    // arbitrary scores: the cell is the per-run partial sums added in ascending run order, whoever runs first
    for (int fused = 0; fused < 2; ++fused)
        for (int descending = 0; descending < 2; ++descending) {
            const std::vector<double> got = walk_sums(c, fused, descending, 1.0f);
            for (u64 r = 0; r < n; ++r)
                CHECK(same_bits(got[r], ordered[r]), "record %llu (rows %llu cols %llu T %llu M %llu fused %d descending %d): %a, want %a", r, c.rows,
                      c.cols, c.T, c.m, fused, descending, got[r], ordered[r]);
        }
    // integer scores: every term is an exact power of two and the cell the direct sum in any order
    Case q = c;
    for (float &v : q.score)
        v = v == v ? std::floor(v) : v;
    for (u64 r = 0; r < n; ++r) {
        exact[r] = 0.0;
        for (u64 p = c.off[r]; p + c.m <= c.off[r + 1]; ++p)
            if (q.score[p] == q.score[p])
                exact[r] += std::ldexp(1.0, (int)q.score[p]);
    }
    for (int fused = 0; fused < 2; ++fused) {
        const std::vector<double> got = walk_sums(q, fused, false, 1.0f);
        for (u64 r = 0; r < n; ++r)
            CHECK(same_bits(got[r], exact[r]), "record %llu, integer scores (rows %llu cols %llu T %llu M %llu fused %d): %a, want %a", r, c.rows, c.cols,
                  c.T, c.m, fused, got[r], exact[r]);
    }
}

// records on the layout (rows, cols): planted junctions first, random lengths behind
static Case make_case(u64 rows, u64 cols, u64 T, u64 m, int layout)
{
    Case c{rows, cols, T, m, {0}, {}};
    const u64 positions = rows * cols;
    auto push = [&](u64 end) {
        end = end < positions ? end : positions;
        c.off.push_back(end < c.off.back() ? c.off.back() : end);
    };
    if (layout == 0) {  // junctions on the run boundaries of the first column and on every column boundary, empties there
        for (u64 r0 = T; r0 < rows && c.off.size() < 12; r0 += T) {
            push(r0);
            push(r0);  // an empty record on the boundary
            push(r0);
        }
        for (u64 col = 1; col <= cols; ++col) {
            push(col * rows);
            if (col % 2)
                push(col * rows);
        }
    } else if (layout == 1) {  // one record
        push(positions - (positions > 3 ? 3 : 0));
    } else if (layout == 2) {  // a record over three runs and more, short ones around it
        push(m - 1);
        push(c.off.back() + 3 * T + m + 1);
        push(c.off.back() + 1);
        push(c.off.back() + rows + 2 * T);
        while (c.off.back() < positions)
            push(c.off.back() + rnd() % (2 * m + 2));
    } else {  // random lengths: none, shorter than M, about a run, about a column
        while (c.off.back() < positions && c.off.size() < 400) {
            const u64 pick = rnd() % 6;
            push(c.off.back() + (pick == 0 ? 0 : pick == 1 ? rnd() % m : pick == 2 ? m : pick == 3 ? T + rnd() % (m + 1) : pick == 4 ? rows - 1 + rnd() % 3
                                                                                                                                        : rnd() % (3 * T + 1)));
        }
    }
    c.score.resize(positions + m);
    for (float &v : c.score) {
        const u64 x = rnd();
        v = x % 23 == 0 ? std::numeric_limits<float>::quiet_NaN() : (float)((double)(x % 4001) / 100.0 - 20.0);  // [-20, 20]
    }
    return c;
}

static void check_exp2()
{
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(exp2_wide(-inf) == 0.0 && exp2_wide(inf) == (double)inf, "infinities");
    CHECK(exp2_wide(0.0f) == 1.0 && exp2_wide(10.0f) == 1024.0 && exp2_wide(-3.0f) == 0.125, "exact powers");
    CHECK(exp2_wide(1500.0f) == (double)inf && exp2_wide(-1500.0f) == 0.0, "beyond a double");
    CHECK(exp2_wide(-1070.0f) == std::ldexp(1.0, -1070), "a denormal double");
    for (int i = 0; i < 20000; ++i) {
        const float x = (float)((double)(rnd() % 2000001) / 1000.0 - 1000.0);
        const double got = exp2_wide(x), want = std::exp2((double)x);
        CHECK(got > 0.0 && std::isfinite(got) && std::fabs(got - want) <= std::ldexp(want, -22), "2^%a = %a, want %a", (double)x, got, want);
    }
}

int main()
{
    check_exp2();
    const u64 rows_[] = {1, 7, 16, 45}, cols_[] = {1, 3, 8}, ts[] = {1, 7, 16, 64}, ms[] = {1, 4, 17};
    for (const u64 rows : rows_)
        for (const u64 cols : cols_)
            for (const u64 T : ts)
                for (const u64 m : ms)
                    for (int layout = 0; layout < 4; ++layout)
                        check_case(make_case(rows, cols, T, m, layout));
    printf("test_seqset_sum: all checks passed (%ld checks)\n", g_checks);
    return 0;
}
