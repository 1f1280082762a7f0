// The host arithmetic of the fused argmax (lightmotif_amd/csrc/argmax_plan.hpp): who takes the candidate route, the
// sample geometry, the list capacities and the layout of its scratch block; the suffix route's choice; the exact route's
// scratch, the job table in the pinned block and the delivery form; the f32 -> 16-bit threshold map.  A stand-alone
// program (no device, no HIP call), built by tests/test_cpp_argmax_plan.py with the address and undefined-behaviour
// sanitizers.
//
// The expected figures are written out.  They come from the expressions score_argmax.hip and score_threshold.hip held
// before the header existed, evaluated once by a scratch program; only the two sweeps the figures cannot cover (10 000
// seeded thresholds, every combination of the delivery's inputs) restate those expressions here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "argmax_plan.hpp"

using namespace lm::argmax;
typedef unsigned long long ull;

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// ---- candidate route, K = 5 --------------------------------------------------------------------------------------------

static bool qualifies(ull cells, size_t m, size_t k, bool has_prefilter, bool one_symbol_scan_fits, bool pair_scan_fits)
{
    return cand_job_qualifies(cells, m, k, has_prefilter, [&] { return one_symbol_scan_fits || pair_scan_fits; });
}

static void test_candidate_gates()
{
    const ull M100 = 100ull * 1000 * 1000;
    CHECK(kmer_count(5, 7) == 16384.0 && kmer_count(5, 6) == 4096.0 && kmer_count(21, 12) == 4.096e15, "(K-1)^M");
    // 100 M cells: 100e6 / 8192 = 12 207.03; 4^7 = 16 384 reaches it, 4^6 = 4 096 does not
    CHECK(qualifies(M100, 7, 5, true, true, true), "100 M cells, M = 7");
    CHECK(!qualifies(M100, 6, 5, true, true, true), "100 M cells, M = 6");
    CHECK(qualifies(8ull << 20, 20, 5, true, true, true) && !qualifies((8ull << 20) - 1, 20, 5, true, true, true), "8 M cells per job");
    CHECK(!qualifies(1ull << 40, 30, 5, true, true, true) && qualifies((1ull << 40) - 1, 30, 5, true, true, true), "2^40 cells");
    // M = 1 fails twice over (4 k-mers); M = 2 against it needs a case the k-mer rule lets through: the rule alone ...
    CHECK(!qualifies(8ull << 20, 1, 5, true, true, true) && !qualifies(8ull << 20, 2, 5, true, true, true), "short motifs, few k-mers");
    // ... and m >= 2 alone, at an alphabet where one row already has the k-mers: K - 1 = 2^20, 8 M cells need 1 024
    CHECK(!qualifies(8ull << 20, 1, (1u << 20) + 1, true, true, true) && qualifies(8ull << 20, 2, (1u << 20) + 1, true, true, true), "M = 1 | 2");
    CHECK(!qualifies(M100, 20, 5, false, true, true), "no prefilter");
    CHECK(!qualifies(M100, 20, 5, true, false, false), "neither scan fits");
    CHECK(qualifies(M100, 20, 5, true, true, false) && qualifies(M100, 20, 5, true, false, true), "one scan suffices");
    // the planner is asked last, and only about jobs whose numbers qualify
    int asked = 0;
    const auto ask = [&] { ++asked; return true; };
    CHECK(cand_job_qualifies(M100, 20, 5, true, ask) && asked == 1, "asked once");
    CHECK(!cand_job_qualifies(M100, 6, 5, true, ask) && !cand_job_qualifies(1 << 20, 20, 5, true, ask) && !cand_job_qualifies(M100, 20, 5, false, ask) && asked == 1,
          "not asked");
    CHECK(cand_call_qualifies(1, M100) && !cand_call_qualifies(1, M100 - 1), "100 M cells per call");
    CHECK(cand_call_qualifies(1u << 20, 1ull << 43) && !cand_call_qualifies((1u << 20) + 1, 1ull << 43), "2^20 jobs per call");
    CHECK(!cand_call_qualifies(0, 0) && !cand_call_qualifies(0, M100), "no job");
}

static void test_sample_geometry()
{
    struct { ull rows; size_t nq; unsigned cus; ull nchunks, stride; } want[] = {
        {1ull << 20, 2, 256, 128, 8256},  {1ull << 18, 2, 256, 32, 8456},     {200000, 2, 256, 32, 6451},  // the floor of 32 chunks binds up to 2^18 rows
        {31250000, 1, 256, 2048, 15266},  {31250000, 2, 256, 3814, 8195},     {31250000, 1, 64, 512, 61154},  // 1 Gbp: a lone job is capped at 8 per CU
    };
    for (const auto &w : want) {
        const SampleGeometry g = sample_geometry(w.rows, w.nq, w.cus);
        CHECK(g.nchunks == w.nchunks && g.stride == w.stride, "rows %llu nq %zu: %llu chunks, stride %llu", w.rows, w.nq, g.nchunks, g.stride);
    }
    CHECK(kSampleRows == 8, "rows per chunk");
    // the last chunk ends inside the rows (8 M cells at C = 32 are 2^18 rows: nothing shorter comes here)
    for (int it = 0; it < 20000; ++it) {
        const ull rows = (1ull << 18) + rnd() % (it % 2 ? 1ull << 22 : 1ull << 35);
        for (size_t nq : {1, 2}) {
            const SampleGeometry g = sample_geometry(rows, nq, it % 3 ? 256 : 8);
            CHECK(g.nchunks >= 32 && g.stride >= kSampleRows && g.stride * (g.nchunks - 1) + kSampleRows <= rows, "rows %llu: %llu x %llu", rows, g.nchunks, g.stride);
        }
    }
    struct { size_t npos; ull maxc; unsigned sgrid; ull cap, ccap; size_t tail; } lists[] = {
        {1, 2048, 2048, 73728, 294912, 8192},        {2, 2048, 1024, 81920, 327680, 8192},
        {300, 2048, 16, 2523136, 10092544, 19200},   {5000, 2048, 16, 33554432, 134217728, 320000},
        {1, 32, 32, 73728, 294912, 128},             {2346, 381, 16, 19283968, 77135872, 150144},
        {5000, 8, 8, 33554432, 134217728, 160000},
    };
    for (const auto &w : lists) {
        const CandLists l = cand_lists(w.npos, w.maxc, 256);
        CHECK(l.sgrid == w.sgrid && l.cap == w.cap && l.ccap == w.ccap, "npos %zu: sgrid %u cap %llu ccap %llu", w.npos, l.sgrid, l.cap, l.ccap);
        CHECK(cand_tail_bytes(w.npos, l.sgrid) == w.tail, "npos %zu: tail %zu", w.npos, cand_tail_bytes(w.npos, l.sgrid));
    }
}

static void test_candidate_head()
{
    CHECK(kSampleJobBytes == 72 && kRescoreJobBytes == 40 && kBatchParamsBytes == 32 && kRecordBytes == 16 && kListHead == 256, "element sizes");
    const size_t want1[7] = {256, 272, 280, 328, 360, 440, 456}, want2346[7] = {256, 9648, 28416, 122256, 197328, 366240, 403776};
    for (const size_t npos : {(size_t)1, (size_t)2346}) {
        const CandHead h = cand_head(npos, kRescoreJobBytes, kBatchParamsBytes, kSampleJobBytes);
        const size_t got[7] = {h.off_bval, h.off_bkey, h.off_rj, h.off_bp, h.off_sj, h.off_res, h.off_hits}, *want = npos == 1 ? want1 : want2346;
        for (int r = 0; r < 7; ++r)
            CHECK(got[r] == want[r], "npos %zu, region %d: %zu, want %zu", npos, r, got[r], want[r]);
    }
    for (size_t npos = 1; npos <= 5000; ++npos) {
        const CandHead h = cand_head(npos, kRescoreJobBytes, kBatchParamsBytes, kSampleJobBytes);
        // counters | best values | best keys | RescoreJob | BatchParams | SampleJob | results | lists: in this order, none
        // overlapping the next
        CHECK(h.off_bval == kListHead && h.off_bval + npos * 4 <= h.off_bkey && h.off_bkey + npos * 8 <= h.off_rj &&
                  h.off_rj + npos * kRescoreJobBytes <= h.off_bp && h.off_bp + npos * kBatchParamsBytes <= h.off_sj &&
                  h.off_sj + npos * kSampleJobBytes <= h.off_res && h.off_res + npos * kRecordBytes == h.off_hits,
              "npos %zu: order", npos);
        // 16-byte aligned where the tables and the u64 keys need it (the key array's END is the one place left unpadded:
        // off_rj is 8-byte aligned, which RescoreJob's pointers ask for)
        CHECK(h.off_bkey % 16 == 0 && h.off_rj % 8 == 0 && (h.off_bp - h.off_rj) % 16 == 0 && (h.off_sj - h.off_bp) % 16 == 0 &&
                  (h.off_res - h.off_sj) % 16 == 0 && h.off_res % 8 == 0 && h.off_hits % 8 == 0,
              "npos %zu: alignment", npos);
        // no padding beyond 15 bytes anywhere
        CHECK(h.off_bkey - (h.off_bval + npos * 4) < 16 && h.off_bp - (h.off_rj + npos * kRescoreJobBytes) < 16 &&
                  h.off_sj - (h.off_bp + npos * kBatchParamsBytes) < 16 && h.off_res - (h.off_sj + npos * kSampleJobBytes) < 16,
              "npos %zu: padding", npos);
    }
}

// ---- suffix route ------------------------------------------------------------------------------------------------------

static void test_suffix()
{
    CHECK(suffix_occurrences(0, 2.0) == 1.5 && suffix_occurrences(0, 1e6) == 8.0, "the clamp of ln(lambda) to [1.5, 8]");
    CHECK(std::fabs(suffix_occurrences(0, 100.0) - 4.6051701859880918) < 1e-12 && suffix_occurrences(5.0, 100.0) == 5.0, "ln(lambda); the option");
    CHECK(kSuffixMinRows == 32768, "shortest suffix");
    struct { ull rows; size_t cols, m, k; bool hp; double opt; Suffix form; ull need; const char *what; } want[] = {
        {1048576, 32, 12, 5, true, 0.01, Suffix::Sparse, 32768, "lambda = 2 exactly (the option keeps the suffix short: need_rows at kSuffixMinRows)"},
        {1048575, 32, 12, 5, true, 0.01, Suffix::None, 0, "lambda just under 2"},
        {1000000, 32, 6, 5, true, 256.0, Suffix::Dense, 32769, "256.008 expected hits (the option pins 256 occurrences)"},
        {1000000, 32, 6, 5, true, 255.99, Suffix::Sparse, 32768, "256.0 expected hits: not above"},
        {1000000, 32, 5, 5, true, 0, Suffix::Dense, 32768, "M = 5: 1 024 expected hits"},
        {1000000, 32, 6, 5, true, 0, Suffix::Sparse, 32768, "M = 6: 256"},
        {131072, 32, 4, 5, true, 0, Suffix::Dense, 32768, "dense: rows / 4 reached"},
        {131071, 32, 4, 5, true, 0, Suffix::None, 0, "dense: one row short of rows / 4"},
        {65536, 32, 6, 5, true, 0, Suffix::Sparse, 32768, "sparse: rows / 2 reached"},
        {65535, 32, 6, 5, true, 0, Suffix::None, 0, "sparse: one row short of rows / 2"},
        {1000000, 32, 0, 5, true, 0, Suffix::None, 0, "M = 0"},
        {1000000, 32, 4, 5, false, 0, Suffix::None, 0, "no prefilter"},
        {1ull << 50, 32, 12, 21, true, 0.1, Suffix::None, 0, "protein, M = 12: 20^12 = 4.096e15 k-mers"},
        {1ull << 44, 32, 11, 21, true, 0.1, Suffix::Sparse, 640000000001ull, "protein, M = 11: 2.048e14"},
        {1ull << 44, 32, 11, 21, true, 0, Suffix::None, 0, "... whose 1.5 occurrences need more than half the rows"},
        {31250000, 32, 8, 5, true, 0, Suffix::Sparse, 32768, "1 Gbp, M = 8"},
        {31250000, 32, 10, 5, true, 0, Suffix::Sparse, 224800, "1 Gbp, M = 10: ln(953.7) = 6.86 occurrences"},
        {3125000, 1, 3, 5, true, 24.0, Suffix::Dense, 32768, "C = 1"},
    };
    for (const auto &w : want) {
        const SuffixChoice s = suffix_choice(w.rows, w.cols, w.m, w.k, w.hp, w.opt);
        CHECK(s.form == w.form && s.rows == w.need, "%s: form %d, %llu rows", w.what, (int)s.form, s.rows);
    }
}

// ---- exact route -------------------------------------------------------------------------------------------------------

static void test_exact_layout()
{
    // results | block records | job table
    const ExactScratch one = exact_scratch(1, 3815), jaspar = exact_scratch(2346, 1000000);
    CHECK(one.off_results == 0 && one.off_blocks == 16 && one.off_jobs == 61056 && one.bytes == 61104, "n = 1: %zu %zu %zu", one.off_blocks, one.off_jobs, one.bytes);
    CHECK(jaspar.off_blocks == 37536 && jaspar.off_jobs == 16037536 && jaspar.bytes == 16150144, "n = 2346: %zu %zu %zu", jaspar.off_blocks, jaspar.off_jobs, jaspar.bytes);
    for (int it = 0; it < 2000; ++it) {
        const size_t n = 1 + rnd() % 300;
        size_t total = 0;  // (the jobs' block records, grid after grid: score_argmax_exact.hip sums them)
        for (size_t i = 0; i < n; ++i)
            total += 1 + (unsigned)(rnd() % (it % 2 ? 5000 : 3));
        const ExactScratch s = exact_scratch(n, total);
        CHECK(s.off_results == 0 && s.off_blocks == 16 * n && s.off_jobs == 16 * n + 16 * total && s.bytes == s.off_jobs + 48 * n, "n %zu, %zu blocks", n, total);
    }
}

static void test_zero_copy()
{
    CHECK(pinned_jobs_off(1) == 64 && pinned_jobs_off(4) == 64 && pinned_jobs_off(5) == 128 && pinned_jobs_off(65536) == 1048576 && pinned_jobs_off(65537) == 1048640,
          "the job table starts on the next 64-byte line");
    // ArgmaxRecord 16 + FinalizeJob 48 = 64 bytes per job and nothing lost to alignment at a multiple of 4: 64 n <= 4 194 304
    size_t edge = 0;
    while (exact_zero_copy(edge + 1))
        ++edge;
    CHECK(edge == kPinBatchBytes / (kRecordBytes + kFinalizeJobBytes) && edge == 65536, "the largest batch delivered in place: %zu", edge);
    CHECK(exact_zero_copy(65536) && !exact_zero_copy(65537) && exact_zero_copy(1) && !exact_zero_copy(1u << 20), "65 536 | 65 537");
    for (size_t n = 1; n <= 70000; n += 7)
        CHECK(exact_zero_copy(n) == (pinned_jobs_off(n) + 48 * n <= (4u << 20)) && pinned_jobs_off(n) % 64 == 0 && pinned_jobs_off(n) >= 16 * n && pinned_jobs_off(n) < 16 * n + 64, "n %zu", n);
}

static void test_delivery()
{
    const ull small = 464165ull * 32, fold_room = kPinFoldBytes / 16 - 1;  // wavefront records that fit beside the first-cell slot
    CHECK(fold_room == 261887, "%llu", fold_room);
    // each of the plan's four forms by the input that should reach it (the tiled store kernel's form stands before the plan:
    // its last condition is what the kernel reports, and tests/test_gpu_pinned_block.py drives it)
    CHECK(pick_delivery(1, 1, true, true, true, small, 4 * 1814) == Delivery::HostFoldRecords, "one job, exact kernel, host_fold");
    CHECK(pick_delivery(1, 1, true, true, false, small, 4 * 1814) == Delivery::PolledRecord, "host_fold = 0");
    CHECK(pick_delivery(1, 1, true, true, true, 1ull << 32, 4 * 1814) == Delivery::PolledRecord, "2^32 cells: the records hold 32-bit cells");
    CHECK(pick_delivery(1, 1, true, true, true, (1ull << 32) - 1, 4 * 1814) == Delivery::HostFoldRecords, "one cell less");
    CHECK(pick_delivery(1, 1, true, true, true, small, fold_room) == Delivery::HostFoldRecords &&
              pick_delivery(1, 1, true, true, true, small, fold_room + 1) == Delivery::PolledRecord, "the records' room in the pinned block");
    CHECK(pick_delivery(1, 1, false, true, true, small, 0) == Delivery::FinalizeInPlace, "one job off the exact kernels");
    CHECK(pick_delivery(2, 1, true, true, true, small, 8) == Delivery::FinalizeInPlace, "two jobs, one group");
    CHECK(pick_delivery(65536, 40, true, exact_zero_copy(65536), true, small, 8) == Delivery::FinalizeInPlace, "65 536 jobs");
    CHECK(pick_delivery(65537, 40, true, exact_zero_copy(65537), true, small, 8) == Delivery::FinalizeStaged, "65 537 jobs");
    // every combination against the flags launch_score_argmax_exact used to carry (fold_in_kernel, fold.records,
    // dv.zero_copy): one form each, the one those flags led to
    const size_t ns[] = {1, 2, 65537}, ngs[] = {1, 2};
    const ull cellss[] = {small, 1ull << 32}, recs[] = {8, fold_room + 1};
    for (size_t n : ns) for (size_t ng : ngs) for (ull cells : cellss) for (ull w : recs) for (int bits = 0; bits < 8; ++bits) {
        const bool exact = bits & 1, zc = bits & 2, hf = bits & 4;
        const bool fold_in_kernel = n == 1 && ng == 1 && exact && zc, records = hf && cells < (1ull << 32) && (w + 1) * 16 <= kPinFoldBytes;
        const Delivery want = fold_in_kernel ? (records ? Delivery::HostFoldRecords : Delivery::PolledRecord)
                              : zc ? Delivery::FinalizeInPlace : Delivery::FinalizeStaged;
        CHECK(pick_delivery(n, ng, exact, zc, hf, cells, (size_t)w) == want, "n %zu groups %zu cells %llu records %llu bits %d", n, ng, cells, w, bits);
    }
}

// ---- threshold map -----------------------------------------------------------------------------------------------------

static void test_threshold_map()
{
    // offset 0, factor 1, emax 0: scaled = floor(t) - 1
    CHECK(discrete_threshold(1.99, 0, 1, 0) == 0, "scaled = 0: below the scan's range");
    CHECK(discrete_threshold(2.0, 0, 1, 0) == 1 && discrete_threshold(2.99, 0, 1, 0) == 1 && discrete_threshold(3.0, 0, 1, 0) == 2, "scaled = 1, 1, 2");
    CHECK(discrete_threshold(65535.0, 0, 1, 0) == 65534 && discrete_threshold(65536.0, 0, 1, 0) == 65535, "scaled = 65 534, 65 535");
    CHECK(discrete_threshold(65537.0, 0, 1, 0) == 65535 && discrete_threshold(1e9, 0, 1, 0) == 65535 && discrete_threshold(1e300, 0, 1, 0) == 65535, "clamped");
    CHECK(discrete_threshold(-10.0, -40.5, 0.01, 0.2) == 3029 && discrete_threshold(-50.0, -40.5, 0.01, 0.2) == 0, "negative offset");
    CHECK(discrete_threshold(12.5, -37.25, 0.0009765625, 0.0107421875) == 50932, "a power-of-two factor");
    CHECK(discrete_threshold(std::nan(""), 0, 1, 0) == 0 && discrete_threshold(-INFINITY, 0, 1, 0) == 0, "NaN, -inf");
    // against the expression launch_score_threshold_batch held
    long rejected = 0, clamped = 0;
    for (int it = 0; it < 10000; ++it) {
        const double offset = -80.0 * unit(), factor = std::ldexp(0.5 + unit(), -(int)(rnd() % 14)), emax = factor * 40 * unit();
        const double t = it % 5 == 0 ? offset + factor * (std::floor(70000 * unit()) + (it % 2 ? 0.0 : 1e-9))  // on and next to whole steps
                                     : offset - 5.0 + (it % 3 ? 60.0 : 70000.0 * factor) * unit();
        const double scaled = std::floor(((double)(float)t - offset) / factor) - std::ceil(emax / factor) - 1.0;
        const unsigned want = scaled >= 1.0 ? (scaled > 65535.0 ? 65535u : (unsigned)scaled) : 0u;
        CHECK(discrete_threshold((double)(float)t, offset, factor, emax) == want, "t %.17g offset %.17g factor %.17g emax %.17g", t, offset, factor, emax);
        rejected += want == 0;
        clamped += want == 65535;
    }
    CHECK(rejected > 100 && clamped > 100 && rejected + clamped < 9000, "the sweep reaches all three outcomes: %ld rejected, %ld clamped", rejected, clamped);
}

int main()
{
    test_candidate_gates();
    test_sample_geometry();
    test_candidate_head();
    test_suffix();
    test_exact_layout();
    test_zero_copy();
    test_delivery();
    test_threshold_map();
    printf("test_argmax_plan: all checks passed (%ld)\n", g_checks);
    return 0;
}
