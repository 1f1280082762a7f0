// argmax_plan.hpp -- the host arithmetic of the fused argmax (score_argmax.hip, score_argmax_exact.hip, score_argmax_cand.hip):
// which job takes which route, the candidate route's sample geometry and list capacities, the layouts of the scratch blocks
// and of the job table in the pinned block, the exact route's delivery form.  Pure functions of plain numbers and booleans, no
// HIP include (tests/cpp/test_argmax_plan.cpp); static_asserts in the .hip files tie the constants repeated here to their types.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace lm {
namespace argmax {

constexpr size_t kRecordBytes = 16, kFinalizeJobBytes = 48;  // = sizeof(ArgmaxRecord), sizeof(FinalizeJob)
constexpr size_t kSampleJobBytes = 72, kRescoreJobBytes = 40, kBatchParamsBytes = 32;  // = sizeof(SampleJob), (RescoreJob), (BatchParams)
constexpr int kPlanBlock = 256;    // = kBlock
constexpr size_t kListHead = 256;  // = kHitListHead: the counters' bytes at the start of the hit lists' block
constexpr size_t kPinBatchBytes = 4u << 20, kPinFoldBytes = (4u << 20) - 4096;  // = kPinArgmaxBatch.cap, kPinFoldRecords.cap

inline size_t align16(size_t x) { return (x + 15) / 16 * 16; }

// distinct k-mers of a motif of m rows over an alphabet whose last symbol is the wildcard: (K-1)^M
inline double kmer_count(size_t k, size_t m) { return std::pow((double)(k - 1), (double)m); }

// f32 threshold -> threshold of the 16-bit discrete prefilter scan: 1 ... 65 535, or 0 = below the scan's range (the exact
// kernel takes the job).  The host's one definition (score_threshold.hip calls it); the kernel argmax_prepare
// (score_argmax_cand.hip) keeps the same map in its own words, because calling this function there changed its instructions.
inline unsigned discrete_threshold(double t, double offset, double factor, double emax)
{
    const double scaled = std::floor((t - offset) / factor) - std::ceil(emax / factor) - 1.0;
    if (scaled >= 1.0)
        return scaled > 65535.0 ? 65535u : (unsigned)scaled;
    return 0u;
}

// ---- candidate route (score_argmax_cand.hip) ---------------------------------------------------------------------------

// The route has ~60 us of fixed cost per call (sample, five small launches): it pays from ~100 M cells per call on
// (measured crossover at M = 20), whether in one job or in a batch.
constexpr unsigned long long kPrefilterArgmaxMinCells = 8ull << 20;            // per job
constexpr unsigned long long kPrefilterArgmaxMinTotal = 100ull * 1000 * 1000;  // per call
constexpr unsigned long long kListRecordsPerJob = 8192;

// Short motifs have few distinct scores: the best k-mer alone occurs cells / (K-1)^M times and every occurrence is a hit --
// worth it while that stays within the list's 8 192 records per job (100 Mbp: M >= 7; the 801 JASPAR motifs of length 7 and
// 8 take 23 / 13 us each on this route against 60 / 50 us on the exact kernel).  `scan_fits()`: the one-symbol or the pair
// scan takes the job's shape (plan_c32); asked last, and only about jobs whose numbers qualify.
template <class ScanFits>
inline bool cand_job_qualifies(unsigned long long cells, size_t m, size_t k, bool has_prefilter, ScanFits scan_fits)
{
    return has_prefilter && m >= 2 && cells >= kPrefilterArgmaxMinCells && cells < (1ull << 40) &&
           kmer_count(k, m) >= (double)cells / (double)kListRecordsPerJob && scan_fits();
}
inline bool cand_call_qualifies(size_t picked_jobs, unsigned long long picked_cells)
{
    return picked_jobs != 0 && picked_jobs <= (1u << 20) && picked_cells >= kPrefilterArgmaxMinTotal;
}

// The sample: exact scores of `nchunks` chunks of kSampleRows rows, chunk c starting at row c * stride.
constexpr unsigned kSampleRows = kPlanBlock / 32;  // one row per half-wave: a chunk is one pass of the block
struct SampleGeometry {
    unsigned long long nchunks, stride;
};
inline SampleGeometry sample_geometry(unsigned long long rows, size_t picked_jobs, unsigned num_cus)
{
    // 1/1024 of the rows, in chunks of kSampleRows rows spread evenly
    unsigned long long nchunks = std::max<unsigned long long>(rows / 1024 / kSampleRows, 32);
    // a lone job: at most one chunk per workgroup of the sample's grid (1 Gbp: 2 048 chunks instead of 3 815 -- one
    // chain of loads per workgroup instead of two, 19 -> 14 us; the bound of a smaller sample is lower, ~1 900 cells
    // tie or beat it instead of ~1 000, which the re-scoring does not notice).  More workgroups instead: 24 -> 33 us.
    if (picked_jobs == 1)
        nchunks = std::min<unsigned long long>(nchunks, (unsigned long long)num_cus * 8);
    return SampleGeometry{nchunks, (rows - kSampleRows) / (nchunks - 1)};
}

// grid.x of the sample over `npos` positions (grid.y) whose largest sample has `max_chunks` chunks; the list capacities
struct CandLists {
    unsigned sgrid;
    unsigned long long cap, ccap;  // hit records, candidate pieces
};
inline CandLists cand_lists(size_t npos, unsigned long long max_chunks, unsigned num_cus)
{
    CandLists l;
    l.sgrid = (unsigned)std::min<unsigned long long>(max_chunks, std::max<unsigned long long>((unsigned long long)num_cus * 8 / npos, 16));
    // ~1024 cells tie with or beat the bound of a 1/1024 sample; leave room for 8x that (bounded at 32 M / 128 M records =
    // 2.5 GB for very large batches: lists that overflow send the batch to the exact kernel, they never change a result)
    l.cap = std::min<unsigned long long>(npos * kListRecordsPerJob + (1 << 16), 32ull << 20);
    l.ccap = 4 * l.cap;
    return l;
}

// head of the scratch block: counters | best values | best keys | RescoreJob, BatchParams, SampleJob tables in launch
// order | results (not uploaded); the lists start at `off_hits`
struct CandHead {
    size_t off_bval, off_bkey, off_rj, off_bp, off_sj, off_res, off_hits;
};
inline CandHead cand_head(size_t npos, size_t rescore_job_bytes, size_t batch_params_bytes, size_t sample_job_bytes)
{
    CandHead h;
    h.off_bval = kListHead;
    h.off_bkey = align16(h.off_bval + npos * 4);
    h.off_rj = h.off_bkey + npos * 8;
    h.off_bp = h.off_rj + align16(npos * rescore_job_bytes);
    h.off_sj = h.off_bp + align16(npos * batch_params_bytes);
    h.off_res = h.off_sj + align16(npos * sample_job_bytes);
    h.off_hits = h.off_res + npos * kRecordBytes;
    return h;
}
// tail of the block, behind the candidates: the sample's partial maxima, one u32 per workgroup
inline size_t cand_tail_bytes(size_t npos, unsigned sgrid) { return npos * sgrid * sizeof(unsigned); }

// ---- suffix route (score_argmax.hip) -----------------------------------------------------------------------------------

constexpr unsigned long long kSuffixMinRows = 1ull << 15;  // keeps the streams long enough

// How many best k-mers the suffix should hold on average.  With lambda = cells / (K-1)^M expected in the whole range,
// scanning a fraction f costs f + exp(-lambda * f) of a full scan (the miss falls back to the usual routes), minimal at
// f = ln(lambda) / lambda: the suffix holds ln(lambda) occurrences, between 1.5 (a miss every fifth motif, still a net gain)
// and 8.  Round 1 used a flat 24: never a miss, four times the rows (JASPAR batch 14.0-14.7 -> 11.0 ms; the context option
// "suffix_occurrences" pins the value for A/B runs).
inline double suffix_occurrences(double option, double lambda)
{
    return option > 0 ? option : std::min(8.0, std::max(1.5, std::log(std::max(lambda, 1.0))));
}

// Two ways to look at a suffix.  Where a best k-mer is dense in it (short motifs) the exact argmax kernel scores it.  Where
// it is sparse, the suffix may be long (up to half the range) and the fused THRESHOLD at t = B scans it instead: the packed
// pair scan flags the cells that can reach B, the exact re-scoring keeps those that do, and the last hit in row-major order
// is the argmax.
enum class Suffix { None, Dense, Sparse };
struct SuffixChoice {
    Suffix form = Suffix::None;
    unsigned long long rows = 0;  // the last `rows` rows of the range
};
inline SuffixChoice suffix_choice(unsigned long long rows, size_t cols, size_t m, size_t k, bool has_prefilter,
                                  double occurrences_option)
{
    SuffixChoice s;
    const double kmers = kmer_count(k, m);
    if (!has_prefilter || m < 1 || !(kmers < 1e15))  // has_prefilter: no NaN / +inf weights
        return s;
    const double lambda = (double)rows * (double)cols / kmers;
    if (lambda < 2.0)
        return s;  // a best k-mer is not expected in the range at all
    const double need_cells = suffix_occurrences(occurrences_option, lambda) * kmers;
    const unsigned long long need_rows =
        std::max<unsigned long long>((unsigned long long)(need_cells / (double)cols) + 1, kSuffixMinRows);
    const bool dense = (double)need_rows * (double)cols / kmers > 256.0;  // expected hits at t = B
    if (need_rows <= (dense ? rows / 4 : rows / 2))
        s = SuffixChoice{dense ? Suffix::Dense : Suffix::Sparse, need_rows};
    return s;
}

// ---- exact route (score_argmax_exact.hip) ------------------------------------------------------------------------------

// device scratch: results | block records | job table
struct ExactScratch {
    size_t off_results = 0, off_blocks = 0, off_jobs = 0, bytes = 0;
};
inline ExactScratch exact_scratch(size_t n, size_t total_blocks)
{
    ExactScratch s;
    s.off_blocks = kRecordBytes * n;
    s.off_jobs = s.off_blocks + kRecordBytes * total_blocks;
    s.bytes = s.off_jobs + kFinalizeJobBytes * n;
    return s;
}
// the pinned block (kPinArgmaxBatch): ArgmaxRecord[n], then the job table on the next 64-byte line
constexpr size_t pinned_jobs_off(size_t n) { return (kRecordBytes * n + 63) / 64 * 64; }
// the job table fits the pinned block: the finalize kernel reads it there and writes the results in front of it
constexpr bool exact_zero_copy(size_t n) { return pinned_jobs_off(n) + kFinalizeJobBytes * n <= kPinBatchBytes; }

// How the scoring kernels' result reaches the host (a fifth form, the tiled store kernel of one small job with the host's
// fold, stands before the plan: its last condition is what that kernel reports, argmax_tiled_host_fold).
//   HostFoldRecords: one job, exact kernel, few wavefronts, 32-bit cell indices: their records go unfolded into the pinned
//                    block (kPinFoldRecords) and the host folds them
//   PolledRecord:    one job, exact kernel: its last workgroup writes the result there and raises the word the host polls
//   FinalizeInPlace: the finalize launch reads the job table in the pinned block and writes the results in front of it
//   FinalizeStaged:  the table does not fit there: table and results live in the device scratch and travel by copies
enum class Delivery { HostFoldRecords, PolledRecord, FinalizeInPlace, FinalizeStaged };

// `first_exact`: the first group takes an exact C = 32 kernel; `wave_records`: its wavefronts, one record each
inline Delivery pick_delivery(size_t n, size_t ngroups, bool first_exact, bool zero_copy, bool host_fold,
                              unsigned long long cells, size_t wave_records)
{
    // one job through the exact kernel: one launch instead of two (a small scan is launch-latency bound)
    if (n == 1 && ngroups == 1 && first_exact && zero_copy)
        return host_fold && cells < (1ull << 32) && (wave_records + 1) * 16 <= kPinFoldBytes ? Delivery::HostFoldRecords
                                                                                              : Delivery::PolledRecord;
    return zero_copy ? Delivery::FinalizeInPlace : Delivery::FinalizeStaged;
}

}  // namespace argmax
}  // namespace lm
