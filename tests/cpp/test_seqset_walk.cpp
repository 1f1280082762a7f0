// The record walk of the per-record reductions over a sequence set (lightmotif_amd/csrc/seqset_walk.hpp: Walker) on the
// host, with a reducer that records what it is handed, against a brute-force loop over the offsets table.  A stand-alone
// program (no device, no HIP call), built by tests/test_cpp_seqset_walk.py with the address and undefined-behaviour
// sanitizers.
//
// Offset tables of 0, 1, 2, 37 and 5 000 records whose lengths include 0, 1, M - 1, M and M + 1, for M = 1, 2, 17, 36, 70;
// the positions of each concatenation cut into lane runs [p0, p1) of 1, 7, 64 positions and one whole run, fed the way
// walk_generic feeds them (the positions of the run) and the way walk_fused does (M - 1 fill steps in front, the steps up
// to a multiple of M behind, both with `live` off).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "seqset_walk.hpp"

using namespace lm;
typedef unsigned long long u64;

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

struct Window { u64 p; bool inside; };
struct Flush { u64 rec, start; std::vector<u64> inside; };  // the `inside` windows delivered since the flush before
struct Log {
    std::vector<Window> windows;
    std::vector<Flush> flushes;
    std::vector<u64> pending;
    int begun = 0;
};

struct Recorder {
    typedef Log Slot;
    Log *log;
    void begin(Log *const &job)
    {
        log = job;
        ++log->begun;
    }
    void window(u64 p, float, bool inside)
    {
        log->windows.push_back({p, inside});
        if (inside)
            log->pending.push_back(p);
    }
    void flush(Slot *slots, u64 rec, u64 start, u64 n)
    {
        CHECK(slots == log && rec < n, "flush of record %llu of %llu", rec, n);
        log->flushes.push_back({rec, start, log->pending});
        log->pending.clear();
    }
};

// record_of[p] = largest r with off[r] <= p for every position p < positions, by one sweep over the table
static std::vector<u64> sweep_records(const std::vector<u64> &off, u64 positions)
{
    std::vector<u64> rec(positions);
    u64 r = 0;
    for (u64 p = 0; p < positions; ++p) {
        while (r + 1 < off.size() && off[r + 1] <= p)
            ++r;
        rec[p] = r;
    }
    return rec;
}

// one lane run [p0, p1): `fused` feeds the fill and the tail steps of walk_fused<M> as well
static void check_run(const std::vector<u64> &off, const std::vector<u64> &record_of, const u64 m, const u64 p0, const u64 p1, const bool fused)
{
    const u64 n = off.size() - 1;
    Log log;
    Walker<Recorder> wk;
    wk.off = off.data();
    wk.n = n;
    wk.m = m;
    wk.slots = &log;
    wk.begin(p0, &log);
    CHECK(log.begun == 1 && wk.rec == record_of[p0], "begin(%llu) in record %llu, the table says %llu", p0, wk.rec, record_of[p0]);
    u64 live_steps = 0;
    if (fused) {
        const u64 total = (p1 - p0) + (m - 1);
        const long long base = (long long)p0 - (long long)(m - 1);
        for (u64 g = 0; g < total; g += m)
            for (u64 s = 0; s < m; ++s) {
                const u64 t = g + s;
                const bool live = t >= m - 1 && t < total;
                wk.take((u64)(base + (long long)t), 0.0f, live);
                live_steps += live;
            }
    } else {
        for (u64 p = p0; p < p1; ++p, ++live_steps)
            wk.take(p, 0.0f);
    }
    wk.flush();
    CHECK(live_steps == p1 - p0, "%llu live steps for [%llu, %llu)", live_steps, p0, p1);

    // every position of the run is delivered once, `inside` exactly when its window fits its record; everything else
    // the fused feed hands over is not `inside`
    std::vector<int> seen(p1 - p0, 0);
    for (const Window &w : log.windows) {
        const bool own = w.p >= p0 && w.p < p1;  // (the fill and tail steps of the fused feed lie outside the run)
        const u64 r = own ? record_of[w.p] : 0;
        const bool fits = own && r < n && w.p + m <= off[r + 1];
        if (own)
            ++seen[w.p - p0];
        CHECK(w.inside == fits, "position %llu (run [%llu, %llu), M = %llu): inside %d, fits %d", w.p, p0, p1, m, (int)w.inside, (int)fits);
    }
    for (u64 i = 0; i < p1 - p0; ++i)
        CHECK(seen[i] == 1, "position %llu delivered %d times", p0 + i, seen[i]);
    CHECK(log.windows.size() == (fused ? ((p1 - p0 + m - 1 + m - 1) / m) * m : p1 - p0), "%zu deliveries", log.windows.size());

    // flushes: the records from begin's to the one of the run's last position, each once, ascending, none behind the table
    const u64 first = record_of[p0], last = record_of[p1 - 1];
    u64 want = first;
    size_t inside_total = 0;
    for (const Flush &f : log.flushes) {
        CHECK(f.rec == want && f.rec < n, "flush of record %llu, expected %llu (n = %llu)", f.rec, want, n);
        CHECK(f.start == off[f.rec], "record %llu flushed with start %llu, not %llu", f.rec, f.start, off[f.rec]);
        for (const u64 p : f.inside)  // the windows a flush merges are its record's
            CHECK(record_of[p] == f.rec && p >= f.start && p + m <= off[f.rec + 1], "window %llu merged into record %llu", p, f.rec);
        inside_total += f.inside.size();
        ++want;
    }
    CHECK(want == (last < n ? last + 1 : (first < n ? n : first)), "flushed up to record %llu, the run [%llu, %llu) ends in %llu (n = %llu)", want, p0, p1,
          last, n);
    CHECK(log.pending.empty(), "%zu windows inside a record were never flushed", log.pending.size());
    size_t inside_want = 0;
    for (u64 p = p0; p < p1; ++p) {
        const u64 r = record_of[p];
        inside_want += r < n && p + m <= off[r + 1];
    }
    CHECK(inside_total == inside_want, "%zu windows inside, brute force %zu", inside_total, inside_want);
}

static void check_table(const std::vector<u64> &off, const u64 m)
{
    const u64 n = off.size() - 1, length = off[n], positions = length + m + 3;  // a few positions behind the last record
    const std::vector<u64> record_of = sweep_records(off, positions);
    // begin on every offset: the record that starts there, the last of the empty ones that share it
    for (u64 r = 0; r <= n; ++r) {
        Log log;
        Walker<Recorder> wk;
        wk.off = off.data();
        wk.n = n;
        wk.m = m;
        wk.slots = &log;
        wk.begin(off[r], &log);
        u64 lastr = r;
        while (lastr < n && off[lastr + 1] == off[r])
            ++lastr;
        CHECK(wk.rec == lastr && wk.start == off[lastr < n ? lastr : n], "begin(off[%llu] = %llu) lands in %llu, not %llu", r, off[r], wk.rec, lastr);
    }
    const u64 runs[] = {1, 7, 64, positions};
    for (const u64 run : runs) {
        for (u64 p0 = 0; p0 < positions; p0 += run) {
            const u64 p1 = p0 + run < positions ? p0 + run : positions;
            check_run(off, record_of, m, p0, p1, false);
            check_run(off, record_of, m, p0, p1, true);
        }
    }
}

int main()
{
    const u64 ms[] = {1, 2, 17, 36, 70};
    const u64 counts[] = {0, 1, 2, 37, 5000};
    for (const u64 m : ms)
        for (const u64 n : counts) {
            const u64 planted[] = {0, 1, m - 1, m, m + 1};
            std::vector<u64> off(n + 1, 0);
            for (u64 r = 0; r < n; ++r) {
                const u64 pick = rnd() % 8;  // the planted lengths (every one of them from 5 records on), runs of empty records, random ones
                const u64 len = r < 5 && n >= 5 ? planted[r] : pick < 5 ? planted[pick] : pick == 5 ? 0 : rnd() % (3 * m + 2);
                off[r + 1] = off[r] + len;
            }
            if (n == 1)
                off[1] = m + 1;
            check_table(off, m);
            if (n <= 2)  // the small tables with every planted length in turn
                for (const u64 len : planted) {
                    for (u64 r = 0; r < n; ++r)
                        off[r + 1] = off[r] + (r == 0 ? len : planted[rnd() % 5]);
                    check_table(off, m);
                }
        }
    printf("test_seqset_walk: all checks passed (%ld checks)\n", g_checks);
    return 0;
}
