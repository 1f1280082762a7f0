// score_argmax.hip -- fused score + Maximum (pli/mod.rs:135-160 over scores that are never written): the entry points,
// which try the suffix route of short motifs (here), then the candidate route through the discrete prefilter
// (score_argmax_cand.hip), and leave the rest to the exact kernels (score_argmax_exact.hip).  Who takes what: argmax_plan.hpp.
#include <cmath>

#include "argmax_plan.hpp"
#include "score_launch.hpp"

namespace lm {

// ---- fused argmax of short motifs: the last rows suffice -----------------------------------------
//
// A short motif's best k-mer occurs all over a long sequence, and the Generic argmax is the LAST
// maximal cell in (row, col) order (pli/mod.rs:144-151).  B = the sequential f32 sum of the row
// maxima of the PSSM is an upper bound of every score (rounding is monotone, so the sum of
// termwise larger weights in the same order is not smaller) and IS the score of the cells that
// hold a best k-mer.  So: score only the last rows of the range -- enough cells that a best
// k-mer is expected ~24 times, (K-1)^M * 24 -- and if their maximum equals B bit for bit, their
// argmax is the answer: no later cell exists, and no earlier cell can beat B.  Otherwise (the
// best k-mer is absent from the suffix) the job takes the usual routes.  On the JASPAR batch
// the motifs up to length 9 (61 % of them) are settled from ~5 % of the rows or less.
// (how many rows, and which of the two ways to look at them: argmax_plan.hpp, suffix_choice)
static int argmax_by_suffix(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n, ArgmaxRecord *out,
                            char *done)
{
    std::vector<ScoreArgs> subs, tsubs;
    std::vector<size_t> idx, tidx;
    std::vector<float> bound, tbound;
    for (size_t i = 0; i < n; ++i) {
        const ScoreArgs &a = jobs[i];
        const lm_hip_pssm *p = a.pssm;
        if (done[i])
            continue;
        const argmax::SuffixChoice sc = argmax::suffix_choice(a.row_end - a.row_begin, a.cols, p->m, p->k, p->has_prefilter, ctx->suffix_occurrences);
        if (sc.form == argmax::Suffix::None)
            continue;
        const float b = best_kmer_score(p);
        if (!std::isfinite(b))
            continue;
        const bool dense = sc.form == argmax::Suffix::Dense;
        ScoreArgs sub = a;
        sub.row_begin = a.row_end - sc.rows;
        (dense ? subs : tsubs).push_back(sub);
        (dense ? idx : tidx).push_back(i);
        (dense ? bound : tbound).push_back(b);
    }
    if (!subs.empty()) {
        std::vector<ArgmaxRecord> recs(subs.size());
        LM_TRY(launch_score_argmax_exact(ctx, subs.data(), subs.size(), 0, recs.data()));
        for (size_t q = 0; q < subs.size(); ++q) {
            const ArgmaxRecord &r = recs[q];
            if (!r.found || !(r.value == bound[q]))
                continue;  // no best k-mer among the last rows
            const size_t i = idx[q];
            out[i] = r;
            out[i].index += (long long)((subs[q].row_begin - jobs[i].row_begin) * jobs[i].cols);
            done[i] = 1;
        }
    }
    if (!tsubs.empty()) {
        // (the list-size memory of the threshold calls belongs to the caller's threshold scans)
        const unsigned long long keep_hits = ctx->last_hit_count, keep_cands = ctx->last_cand_count;
        HitOutput ho;
        const int st = launch_score_threshold_batch(ctx, tsubs.data(), tbound.data(), tsubs.size(), HitKeys::RowMajor, &ho);
        ctx->last_hit_count = keep_hits;
        ctx->last_cand_count = keep_cands;
        if (st != LM_HIP_OK) {
            ho.release();
            return st;
        }
        for (size_t q = 0; q < tsubs.size(); ++q) {
            if (ho.job_start[q + 1] == ho.job_start[q])
                continue;  // no best k-mer among the last rows
            const size_t last = ho.job_start[q + 1] - 1, i = tidx[q];
            out[i].value = ho.values[last];
            out[i].found = 1;
            out[i].index = (long long)((ho.coords[last].row + (tsubs[q].row_begin - jobs[i].row_begin)) * jobs[i].cols +
                                       ho.coords[last].col);
            done[i] = 1;
        }
        ho.release();
    }
    return LM_HIP_OK;
}

// Fused score+argmax of `n` independent jobs: the suffix and candidate routes where they apply, the
// exact kernels for the rest.
int launch_score_argmax_batch(lm_hip_ctx *ctx, const ScoreArgs *jobs, size_t n,
                              int first_cell_rule, ArgmaxRecord *out)
{
    if (n == 0)
        return LM_HIP_OK;
    std::vector<char> done(n, 0);
    if (ctx->use_prefilter && ctx->suffix_argmax)
        LM_TRY(argmax_by_suffix(ctx, jobs, n, out, done.data()));
    if (ctx->use_prefilter)
        LM_TRY(argmax_by_prefilter(ctx, jobs, n, out, done.data()));
    std::vector<ScoreArgs> rest;
    std::vector<size_t> rest_idx;
    for (size_t i = 0; i < n; ++i)
        if (!done[i]) {
            rest.push_back(jobs[i]);
            rest_idx.push_back(i);
        }
    if (rest.empty())
        return LM_HIP_OK;
    if (rest.size() == n)
        return launch_score_argmax_exact(ctx, jobs, n, first_cell_rule, out);
    std::vector<ArgmaxRecord> recs(rest.size());
    LM_TRY(launch_score_argmax_exact(ctx, rest.data(), rest.size(), first_cell_rule, recs.data()));
    for (size_t k = 0; k < rest.size(); ++k)
        out[rest_idx[k]] = recs[k];
    return LM_HIP_OK;
}

int launch_score_argmax(lm_hip_ctx *ctx, const ScoreArgs &a, int first_cell_rule,
                        ArgmaxRecord *out)
{
    return launch_score_argmax_batch(ctx, &a, 1, first_cell_rule, out);
}

}  // namespace lm
