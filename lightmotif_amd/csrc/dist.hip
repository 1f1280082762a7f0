// dist.hip -- the score distributions of a whole motif batch, built and queried on the device.
//
// lightmotif turns `--pvalue` into a threshold, and a hit's score into its p-value, through the MEME-style discretised
// score distribution of a ScoringMatrix (pwm/dist.rs:129-225; lightmotif_amd/dist.py restates it in numpy f64 and is the
// specification here, cell for cell).  Per motif of M rows over an alphabet of k symbols:
//
//   discretise   small / large = the least / greatest finite weight; small == large: small = large - 1;
//                offset = floor(small), scale = floor(1000 / (large - offset)),
//                s[i][a] = round_half_away((w[i][a] - offset) * scale); a -inf weight skips its symbol   (dist.rs:133-161)
//   convolve     pdf[0] = 1; step i: new[t] = 0.0, then for a = 0 .. k-1 IN ORDER, where the symbol is not skipped and
//                0 <= t - s <= 1000 i:  new[t] = new[t] + old[t - s] * bg[a]                             (dist.rs:164-191)
//   survive      from the top index down: sf[t] = min(pdf[t] + sf[t + 1], 1.0); max_score = the highest index >= 1 with
//                mass, min_score = the lowest index <= size - 2 with mass, 0 where there is none        (dist.rs:194-213)
//
// The reference scatters (`pdf_new[k + s] += pdf_old[k] * bg[a]`, symbol after symbol); a cell's terms arrive in symbol
// order, so the gather above adds the same f64 numbers in the same order and the tables are bit-equal.  Every term is one
// f64 multiply followed by one f64 add (the unit is built with -ffp-contract=off like the rest: no fused multiply-add).
//
// THE KERNELS
//   dist_build     ONE launch for the batch.  The discretisation (M x k numbers per motif) is done by the host with
//                  std::floor and the rounding rule of dist.py, and uploaded as i32 steps (-1 = skipped).  A workgroup
//                  takes the motifs blockIdx.x, blockIdx.x + gridDim.x, ... of the list sorted by length, longest first
//                  (the cost grows with M^2), with no atomic deciding anything: a call repeats byte for byte.  The two
//                  buffers of the convolution are the motif's own table and ONE spare table per workgroup, sized for its
//                  longest motif; the parity of M decides where step 0 starts so that the last step lands in the table.
//                  A step writes exactly the cells the next one reads (0 .. 1000 (i + 1)), so nothing is cleared.
//                  The survival function is a sequential f64 chain and stays one (a parallel scan would round
//                  differently): the workgroup stages kDistTile cells in LDS, finds the lowest / highest cell with mass
//                  on the way, ONE lane walks the tile from the top carrying the running sum, and the workgroup writes
//                  the tile back over the pdf.
//   dist_scores    one lane per motif: the binary search of dist.rs:104-116 with the reference's probe sequence (it
//                  decides which index of a run of equal values comes back).  The f32 `unscale` is the host's.
//   dist_pvalues   one lane per score (dist.rs:77-101): the motif of lane h is found in the prefix sums of the counts,
//                  then scaled = round((score - M offset) * scale) as Rust's saturating `as i32` (NaN -> 0) and one
//                  gather from the resident table.
//
// MEMORY.  8 * (1000 * sum(M) + n) bytes of tables stay resident (177 MB for the 2 346 matrices of JASPAR 2024), plus
// 40 bytes per motif.  lm_hip_dists_create holds the spare tables of its workgroups on top while it runs.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <numeric>
#include <vector>

#include "lm_internal.hpp"

namespace lm {

constexpr int kDistBlock = 256;
constexpr int kDistRange = 1000;  // CDF_RANGE, dist.rs:47
constexpr int kDistTile = 2048;   // cells of the survival chain staged in LDS at a time
constexpr int kDistMaxK = 64;     // alphabet sizes are 5 and 21
constexpr int kDistCells = 4;     // cells of a convolution step one lane carries at a time

struct DistJob {                  // one motif of the build, in launch order
    unsigned long long table;     // its first cell in the tables
    unsigned long long spare;     // the spare table of the workgroup that takes it
    unsigned long long steps;     // its rows x k discretised weights
    unsigned bg, motif;           // its k background values; its index in the batch
    int rows, k;
};

struct DistMeta {                 // what the queries need of one motif
    unsigned long long table;
    double scale, shift;          // shift = rows * offset
    int len, pad;
};

__global__ __launch_bounds__(kDistBlock) void dist_build(const DistJob *__restrict__ jobs, const unsigned njobs,
                                                        const int *__restrict__ steps, const double *__restrict__ bgs,
                                                        double *tables, double *spares, int2 *__restrict__ bounds)
{
    __shared__ double s_tile[kDistTile];
    __shared__ double s_bg[kDistMaxK];
    __shared__ int s_step[kDistMaxK];
    __shared__ int s_lo, s_hi;
    const int tid = (int)threadIdx.x;
    for (unsigned j = blockIdx.x; j < njobs; j += gridDim.x) {
        const DistJob job = jobs[j];
        const int rows = job.rows, k = job.k;
        const int size = rows * kDistRange + 1;
        double *const table = tables + job.table, *const spare = spares + job.spare;
        double *old = (rows & 1) ? spare : table;  // the last step writes the table
        if (tid == 0) {
            old[0] = 1.0;
            s_lo = INT_MAX;
            s_hi = 0;
        }
        if (tid < k)
            s_bg[tid] = bgs[job.bg + tid];
        __syncthreads();
        for (int i = 0; i < rows; ++i) {
            double *const nw = old == table ? spare : table;
            if (tid < k)
                s_step[tid] = steps[job.steps + (unsigned long long)i * k + tid];
            __syncthreads();
            const int mx = i * kDistRange;
            const double *__restrict__ src = old;  // (two different buffers: the loads of the next cell need not wait for this store)
            double *__restrict__ dst = nw;
            // kDistCells cells per lane and pass, so that as many loads are in flight; each cell's terms stay in symbol order
            for (int t0 = tid; t0 <= mx + kDistRange; t0 += kDistCells * kDistBlock) {
                double acc[kDistCells];
#pragma unroll
                for (int q = 0; q < kDistCells; ++q)
                    acc[q] = 0.0;
                for (int a = 0; a < k; ++a) {
                    const int s = s_step[a];
                    const double b = s_bg[a];
                    if (s < 0)
                        continue;
#pragma unroll
                    for (int q = 0; q < kDistCells; ++q) {
                        // the load is unconditional, from a clamped index, and the term is kept or dropped by a select: the
                        // loads of the kDistCells cells then issue together (u <= mx also keeps t within the step: s <= 1000)
                        const int u = t0 + q * kDistBlock - s;
                        const double term = acc[q] + src[min(max(u, 0), mx)] * b;
                        acc[q] = (u >= 0 && u <= mx) ? term : acc[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < kDistCells; ++q)
                    if (t0 + q * kDistBlock <= mx + kDistRange)
                        dst[t0 + q * kDistBlock] = acc[q];
            }
            __syncthreads();  // the step's cells are the next step's input
            old = nw;
        }

        int lo = INT_MAX, hi = 0;
        double carry = 0.0;  // sf[top], lane 0
        for (int top = size; top > 0; top -= kDistTile) {
            const int base = max(top - kDistTile, 0), cnt = top - base;
            for (int c = tid; c < cnt; c += kDistBlock) {
                const double p = table[base + c];
                s_tile[c] = p;
                if (p > 0.0) {
                    const int idx = base + c;
                    if (idx >= 1)
                        hi = max(hi, idx);
                    if (idx <= size - 2)
                        lo = min(lo, idx);
                }
            }
            __syncthreads();
            if (tid == 0) {
                for (int c = cnt - 1; c >= 0; --c) {
                    const double x = s_tile[c] + carry;
                    carry = x > 1.0 ? 1.0 : x;
                    s_tile[c] = carry;
                }
            }
            __syncthreads();
            for (int c = tid; c < cnt; c += kDistBlock)
                table[base + c] = s_tile[c];
            __syncthreads();
        }
        if (lo != INT_MAX)
            atomicMin(&s_lo, lo);
        if (hi != 0)
            atomicMax(&s_hi, hi);
        __syncthreads();
        if (tid == 0)
            bounds[job.motif] = make_int2(s_lo == INT_MAX ? 0 : s_lo, s_hi);
        __syncthreads();  // s_lo / s_hi / s_bg are the next motif's
    }
}

__global__ __launch_bounds__(kDistBlock) void dist_scores(const DistMeta *__restrict__ meta, const int2 *__restrict__ bounds,
                                                         const unsigned n, const double *__restrict__ tables,
                                                         const double *__restrict__ pvalues, int *__restrict__ index)
{
    const unsigned i = blockIdx.x * (unsigned)kDistBlock + threadIdx.x;
    if (i >= n)
        return;
    const double p = pvalues[i];
    const double *sf = tables + meta[i].table;
    int at;
    if (p >= 1.0) {
        at = bounds[i].x;
    } else if (p <= 0.0) {
        at = bounds[i].y;
    } else {  // slice::binary_search_by with cmp = p.partial_cmp(x) on the descending table
        int lo = 0, hi = meta[i].len;
        at = -1;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const double x = sf[mid];
            if (p == x) {
                at = mid;
                break;
            }
            if (p < x)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (at < 0)
            at = lo;
    }
    index[i] = at;
}

__global__ __launch_bounds__(kDistBlock) void dist_pvalues(const DistMeta *__restrict__ meta, const int2 *__restrict__ bounds,
                                                          const unsigned n, const unsigned long long *__restrict__ starts,
                                                          const double *__restrict__ tables, const float *__restrict__ scores,
                                                          const unsigned long long total, double *__restrict__ out)
{
    const unsigned long long h = (unsigned long long)blockIdx.x * kDistBlock + threadIdx.x;
    if (h >= total)
        return;
    unsigned lo = 0, hi = n - 1;  // the motif whose scores hold h: the first i with starts[i + 1] > h
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (starts[mid + 1] <= h)
            lo = mid + 1;
        else
            hi = mid;
    }
    const DistMeta m = meta[lo];
    const double x = ((double)scores[h] - m.shift) * m.scale;
    const double r = copysign(floor(fabs(x) + 0.5), x);  // the rounding of dist.py: half away from zero
    int scaled;                                          // Rust's `as i32`: saturating, NaN -> 0
    if (r != r)
        scaled = 0;
    else if (r >= 2147483647.0)
        scaled = INT_MAX;
    else if (r <= -2147483648.0)
        scaled = INT_MIN;
    else
        scaled = (int)r;
    double p;
    if (scaled < bounds[lo].x)
        p = 1.0;
    else if (scaled >= m.len)
        p = 0.0;
    else
        p = tables[m.table + (unsigned long long)scaled];
    out[h] = p;
}

}  // namespace lm

struct lm_hip_dists {
    int device = 0;
    size_t n = 0;
    double *d_tables = nullptr;
    lm::DistMeta *d_meta = nullptr;
    int2 *d_bounds = nullptr;
    std::vector<size_t> rows;
    std::vector<unsigned long long> table;  // first cell of each motif's table
    std::vector<double> scale, offset;
    std::vector<int> min_score, max_score;
};

namespace lm {
namespace {

// dist.rs:133-161 for one matrix (weights m x k, dense): offset, scale and the m x k steps, -1 for a skipped symbol.
int discretise(const char *what, size_t motif, const float *w, size_t m, size_t k, double *scale, double *offset, int *steps)
{
    double small = std::numeric_limits<double>::infinity(), large = -small;
    for (size_t i = 0; i < m * k; ++i) {
        const double x = (double)w[i];
        if (x != x || x == std::numeric_limits<double>::infinity())
            return fail(LM_HIP_ERR_BAD_ARGS, "%s: matrix %zu holds a %s weight (row %zu)", what, motif, x != x ? "NaN" : "+inf", i / k);
        if (std::isfinite(x)) {
            small = std::min(small, x);
            large = std::max(large, x);
        }
    }
    if (!(small <= large))
        return fail(LM_HIP_ERR_BAD_ARGS, "%s: matrix %zu has no finite weight", what, motif);
    if (small == large)
        small = large - 1.0;
    *offset = std::floor(small);
    *scale = std::floor((double)kDistRange / (large - *offset));
    for (size_t i = 0; i < m * k; ++i) {
        const double x = (double)w[i];
        if (!std::isfinite(x)) {
            steps[i] = -1;
            continue;
        }
        const double y = (x - *offset) * *scale;
        const double r = std::copysign(std::floor(std::fabs(y) + 0.5), y);
        if (!(r >= 0.0 && r <= (double)kDistRange))  // (cannot happen: offset <= w <= large, scale <= 1000 / (large - offset))
            return fail(LM_HIP_ERR_BAD_ARGS, "%s: matrix %zu discretises a weight to %g, outside 0 .. %d", what, motif, r, kDistRange);
        steps[i] = (int)r;
    }
    return LM_HIP_OK;
}

struct DistTemps {
    lm_hip_ctx *ctx;
    void *d_jobs = nullptr, *d_steps = nullptr, *d_bgs = nullptr, *d_spares = nullptr;
    lm_hip_dists *d = nullptr;
    explicit DistTemps(lm_hip_ctx *c) : ctx(c) {}
    ~DistTemps()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : {d_jobs, d_steps, d_bgs, d_spares})
            if (p)
                (void)hipFree(p);
        if (d)
            lm_hip_dists_destroy(d);
    }
};

int dists_build(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const float *const *backgrounds, lm_hip_dists **out)
{
    DistTemps t(ctx);
    t.d = new (std::nothrow) lm_hip_dists();
    if (!t.d)
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    lm_hip_dists *d = t.d;
    d->device = ctx->device;
    d->n = n;
    if (n == 0) {
        *out = d;
        t.d = nullptr;
        return LM_HIP_OK;
    }
    std::vector<DistJob> jobs;
    std::vector<DistMeta> meta;
    std::vector<int> steps;
    std::vector<double> bgs;
    std::vector<unsigned> order;
    unsigned long long cells = 0;
    try {
        d->rows.resize(n), d->table.resize(n), d->scale.resize(n), d->offset.resize(n);
        d->min_score.assign(n, 0), d->max_score.assign(n, 0);
        jobs.resize(n), meta.resize(n), order.resize(n);
        size_t nsteps = 0;
        for (size_t i = 0; i < n; ++i)
            nsteps += pssms[i]->m * pssms[i]->k;
        steps.resize(nsteps);
        std::vector<unsigned long long> step_at(n);
        std::vector<unsigned> bg_at(n);
        nsteps = 0;
        for (size_t i = 0; i < n; ++i) {
            const lm_hip_pssm *p = pssms[i];
            LM_TRY(discretise("dists_create", i, p->host.data(), p->m, p->k, &d->scale[i], &d->offset[i], steps.data() + nsteps));
            step_at[i] = nsteps;
            nsteps += p->m * p->k;
            bg_at[i] = (unsigned)bgs.size();
            for (size_t a = 0; a < p->k; ++a) {
                // abc.rs:473-487: 1 / (K - 1) for every symbol but the default one, which gets 0
                const float u = a + 1 < p->k ? 1.0f / (float)(p->k - 1) : 0.0f;
                bgs.push_back((double)(backgrounds && backgrounds[i] ? backgrounds[i][a] : u));
            }
            d->rows[i] = p->m;
            d->table[i] = cells;
            cells += (unsigned long long)p->m * kDistRange + 1;
            meta[i] = DistMeta{d->table[i], d->scale[i], (double)p->m * d->offset[i], (int)(p->m * kDistRange + 1), 0};
        }
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return d->rows[a] > d->rows[b]; });
        // workgroup g takes order[g], order[g + grid], ...: its spare table is sized for the first, its longest
        const unsigned grid = (unsigned)std::min<size_t>(n, (size_t)std::max(ctx->num_cus, 1) * 4);
        std::vector<unsigned long long> spare_at(grid);
        unsigned long long spare_cells = 0;
        for (unsigned g = 0; g < grid; ++g) {
            spare_at[g] = spare_cells;
            spare_cells += (unsigned long long)d->rows[order[g]] * kDistRange + 1;
        }
        for (size_t j = 0; j < n; ++j) {
            const unsigned i = order[j];
            jobs[j] = DistJob{d->table[i], spare_at[j % grid], step_at[i], bg_at[i], i, (int)d->rows[i], (int)pssms[i]->k};
        }

        LM_HIP_TRY(hipMalloc(&d->d_tables, cells * sizeof(double)));
        LM_HIP_TRY(hipMalloc(&d->d_meta, n * sizeof(DistMeta)));
        LM_HIP_TRY(hipMalloc(&d->d_bounds, n * sizeof(int2)));
        LM_HIP_TRY(hipMalloc(&t.d_jobs, n * sizeof(DistJob)));
        LM_HIP_TRY(hipMalloc(&t.d_steps, std::max<size_t>(steps.size(), 1) * sizeof(int)));
        LM_HIP_TRY(hipMalloc(&t.d_bgs, bgs.size() * sizeof(double)));
        LM_HIP_TRY(hipMalloc(&t.d_spares, spare_cells * sizeof(double)));
        LM_HIP_TRY(hipMemcpyAsync(d->d_meta, meta.data(), n * sizeof(DistMeta), hipMemcpyHostToDevice, ctx->stream));
        LM_HIP_TRY(hipMemcpyAsync(t.d_jobs, jobs.data(), n * sizeof(DistJob), hipMemcpyHostToDevice, ctx->stream));
        if (!steps.empty())
            LM_HIP_TRY(hipMemcpyAsync(t.d_steps, steps.data(), steps.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        LM_HIP_TRY(hipMemcpyAsync(t.d_bgs, bgs.data(), bgs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(dist_build, dim3(grid), dim3(kDistBlock), 0, ctx->stream, static_cast<const DistJob *>(t.d_jobs),
                           (unsigned)n, static_cast<const int *>(t.d_steps), static_cast<const double *>(t.d_bgs), d->d_tables,
                           static_cast<double *>(t.d_spares), d->d_bounds);
        LM_HIP_TRY(hipGetLastError());
        ctx->last_kernel = "dist_build";
        std::vector<int2> bounds(n);
        LM_HIP_TRY(hipMemcpyAsync(bounds.data(), d->d_bounds, n * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i)
            d->min_score[i] = bounds[i].x, d->max_score[i] = bounds[i].y;
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    *out = d;
    t.d = nullptr;
    return LM_HIP_OK;
}

}  // namespace
}  // namespace lm

using namespace lm;

extern "C" {

int lm_hip_dists_create(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, size_t n, const float *const *backgrounds,
                        lm_hip_dists **out)
{
    if (!ctx || !out)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_create: null argument");
    *out = nullptr;
    if (n && !pssms)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_create: null matrix list with %zu matrices", n);
    if (n > 0x7fffffffu)
        return fail(LM_HIP_ERR_CAPACITY, "dists_create: %zu matrices are more than one batch takes", n);
    for (size_t i = 0; i < n; ++i) {
        if (!pssms[i])
            return fail(LM_HIP_ERR_BAD_ARGS, "dists_create: matrix %zu is null", i);
        if (pssms[i]->m == 0 || pssms[i]->k == 0 || pssms[i]->k > (size_t)kDistMaxK)
            return fail(LM_HIP_ERR_BAD_ARGS, "dists_create: matrix %zu has %zu rows over %zu symbols", i, pssms[i]->m, pssms[i]->k);
        if (pssms[i]->m > (size_t)(INT_MAX / kDistRange) - 1)
            return fail(LM_HIP_ERR_CAPACITY, "dists_create: matrix %zu has %zu rows, too many for a table", i, pssms[i]->m);
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    return dists_build(ctx, pssms, n, backgrounds, out);
}

size_t lm_hip_dists_len(const lm_hip_dists *dists) { return dists ? dists->n : 0; }

int lm_hip_dists_info(const lm_hip_dists *dists, size_t motif, size_t *rows, double *scale, double *offset, int64_t *min_score,
                      int64_t *max_score, size_t *sf_len)
{
    if (!dists)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_info: null distributions");
    if (motif >= dists->n)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_info: motif %zu of %zu", motif, dists->n);
    if (rows) *rows = dists->rows[motif];
    if (scale) *scale = dists->scale[motif];
    if (offset) *offset = dists->offset[motif];
    if (min_score) *min_score = dists->min_score[motif];
    if (max_score) *max_score = dists->max_score[motif];
    if (sf_len) *sf_len = dists->rows[motif] * (size_t)kDistRange + 1;
    return LM_HIP_OK;
}

int lm_hip_dists_sf(lm_hip_ctx *ctx, const lm_hip_dists *dists, size_t motif, double *dst, size_t capacity)
{
    if (!ctx || !dists || !dst)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_sf: null argument");
    if (dists->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_sf: the distributions live on device %d, the context on %d", dists->device, ctx->device);
    if (motif >= dists->n)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_sf: motif %zu of %zu", motif, dists->n);
    const size_t len = dists->rows[motif] * (size_t)kDistRange + 1;
    if (capacity < len)
        return fail(LM_HIP_ERR_CAPACITY, "dists_sf: room for %zu of %zu cells", capacity, len);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    LM_HIP_TRY(hipMemcpyAsync(dst, dists->d_tables + dists->table[motif], len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LM_HIP_OK;
}

int lm_hip_dists_scores(lm_hip_ctx *ctx, const lm_hip_dists *dists, const double *pvalues, float *scores)
{
    if (!ctx || !dists)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_scores: null argument");
    if (dists->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_scores: the distributions live on device %d, the context on %d", dists->device, ctx->device);
    const size_t n = dists->n;
    if (n == 0)
        return LM_HIP_OK;
    if (!pvalues || !scores)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_scores: null array for %zu motifs", n);
    std::vector<int> index;
    try {
        index.resize(n);
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    // scratch: p-values (8 n) | indices (4 n)
    LM_TRY(ctx->scratch.reserve(n * (sizeof(double) + sizeof(int))));
    double *d_p = static_cast<double *>(ctx->scratch.ptr);
    int *d_index = reinterpret_cast<int *>(d_p + n);
    LM_HIP_TRY(hipMemcpyAsync(d_p, pvalues, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dist_scores, dim3((unsigned)((n + kDistBlock - 1) / kDistBlock)), dim3(kDistBlock), 0, ctx->stream,
                       dists->d_meta, dists->d_bounds, (unsigned)n, dists->d_tables, d_p, d_index);
    LM_HIP_TRY(hipGetLastError());
    ctx->last_kernel = "dist_scores";
    LM_HIP_TRY(hipMemcpyAsync(index.data(), d_index, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i)  // unscale, dist.rs:84-88, in f32: one correctly rounded division, one addition
        scores[i] = (float)index[i] / (float)dists->scale[i] + (float)((double)dists->rows[i] * dists->offset[i]);
    return LM_HIP_OK;
}

int lm_hip_dists_pvalues(lm_hip_ctx *ctx, const lm_hip_dists *dists, const size_t *counts, const float *scores,
                         size_t score_stride_bytes, double *pvalues)
{
    if (!ctx || !dists)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_pvalues: null argument");
    if (dists->device != ctx->device)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_pvalues: the distributions live on device %d, the context on %d", dists->device, ctx->device);
    const size_t n = dists->n;
    if (n && !counts)
        return fail(LM_HIP_ERR_BAD_ARGS, "dists_pvalues: null counts for %zu motifs", n);
    std::vector<unsigned long long> starts;
    std::vector<float> packed;
    try {
        starts.assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            if (counts[i] > (size_t)1 << 40)
                return fail(LM_HIP_ERR_CAPACITY, "dists_pvalues: %zu scores for motif %zu", counts[i], i);
            starts[i + 1] = starts[i] + counts[i];
        }
        const size_t total = (size_t)starts[n];
        if (total == 0)
            return LM_HIP_OK;
        if (!scores || !pvalues)
            return fail(LM_HIP_ERR_BAD_ARGS, "dists_pvalues: null array for %zu scores", total);
        if (score_stride_bytes < sizeof(float))
            return fail(LM_HIP_ERR_BAD_ARGS, "dists_pvalues: a stride of %zu bytes between f32 scores", score_stride_bytes);
        const unsigned long long blocks = ((unsigned long long)total + kDistBlock - 1) / kDistBlock;
        if (blocks > 0x7fffffffull)
            return fail(LM_HIP_ERR_CAPACITY, "dists_pvalues: %zu scores are more than one launch takes", total);
        const float *src = scores;
        if (score_stride_bytes != sizeof(float)) {
            packed.resize(total);
            const char *at = reinterpret_cast<const char *>(scores);
            for (size_t h = 0; h < total; ++h, at += score_stride_bytes)
                memcpy(&packed[h], at, sizeof(float));
            src = packed.data();
        }
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard guard(ctx->device);
        // scratch: p-values (8 total) | starts (8 (n + 1)) | scores (4 total)
        LM_TRY(ctx->scratch.reserve(total * (sizeof(double) + sizeof(float)) + (n + 1) * sizeof(unsigned long long)));
        double *d_out = static_cast<double *>(ctx->scratch.ptr);
        unsigned long long *d_starts = reinterpret_cast<unsigned long long *>(d_out + total);
        float *d_scores = reinterpret_cast<float *>(d_starts + n + 1);
        LM_HIP_TRY(hipMemcpyAsync(d_starts, starts.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
        LM_HIP_TRY(hipMemcpyAsync(d_scores, src, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(dist_pvalues, dim3((unsigned)blocks), dim3(kDistBlock), 0, ctx->stream, dists->d_meta, dists->d_bounds,
                           (unsigned)n, d_starts, dists->d_tables, d_scores, (unsigned long long)total, d_out);
        LM_HIP_TRY(hipGetLastError());
        ctx->last_kernel = "dist_pvalues";
        LM_HIP_TRY(hipMemcpyAsync(pvalues, d_out, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    }
    return LM_HIP_OK;
}

int lm_hip_dists_destroy(lm_hip_dists *dists)
{
    if (!dists)
        return LM_HIP_OK;
    {
        DeviceGuard guard(dists->device);
        for (void *p : {static_cast<void *>(dists->d_tables), static_cast<void *>(dists->d_meta), static_cast<void *>(dists->d_bounds)})
            if (p)
                (void)hipFree(p);
    }
    delete dists;
    return LM_HIP_OK;
}

}  // extern "C"
