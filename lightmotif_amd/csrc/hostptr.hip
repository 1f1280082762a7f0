// hostptr.hip -- the host-pointer entry points: what the reference-side shim binds.
//
//   lm_hip_score_f32      Score::score_rows_into on host matrices   (pli/mod.rs:72-106, avx2.rs:889-904)
//   lm_hip_score_u8_host  the same with a DiscreteMatrix, u8 scores   (avx2.rs:294-347, 921-931; scan.rs:174-178)
//   lm_hip_argmax_f32     StripedScores::argmax                     (scores.rs:181-186, pli/mod.rs:135-155)
//   lm_hip_max_f32        StripedScores::max                        (scores.rs:188-192, pli/mod.rs:158-160)
//   lm_hip_threshold_f32  StripedScores::threshold                  (scores.rs:207-213, pli/mod.rs:210-221)
//
// The caller's matrices are pageable host memory (a Rust Vec); every call moves 1 B per position up and 4 B per
// position down over PCIe, so the link is the floor.  What this path is about is paying nothing else:
//
//  * LANES (host_lane.hip).  Every host thread that calls in gets a lane of its own -- a context (its own stream), device
//    staging buffers that persist between calls, and a small cache of device-side PSSM tables keyed on the weights -- so the
//    CLI's worker threads (main.rs:270) and GIL-released Python threads (lightmotif-py lib.rs:865) overlap instead of
//    queueing on one context, and a loop over one motif (lightmotif-bench dna.rs:104-107) builds its tables once.
//    A lane whose thread has exited is handed to the next new thread.  New lanes go to the process's HOME device (the HIP
//    device current in the thread that made the first unbound call); with lm_hip_host_spread_lanes(1) they are dealt
//    round-robin over the usable devices (eight worker threads on an 8-GPU node then use eight GPUs and eight PCIe
//    links); $LM_HIP_DEVICE (read once) pins every lane to one ordinal, lm_hip_host_bind_thread one thread.
//  * SMALL calls (the reference's own bench: 464 165 positions; a Scanner block: 256 rows) are latency-bound:
//    one pageable copy up, one kernel, one pageable copy down, one synchronisation; no allocation, no table build.
//    The tiniest (<= 128 KB each way) skip the copy commands altogether: the kernel reads the symbols from and writes
//    the scores to pinned host memory (tools/kbench/hostpipe_bench.hip: 15.9 us against 27.8 us per iteration).
//  * LARGE calls (>= 96 MB of scores) are link-bound and run as a three-stage pipeline over row tiles through a ring of
//    pinned buffers that exists once per device (host_pipe.hip).
// The Dispatch::Hip cost model that tells a shim which calls to send here is host_cost.hip.
#include "host_lane.hpp"

using namespace lm;
using namespace lm::host;

namespace {

void copy_rows(char *dst, size_t dst_pitch, const char *src, size_t src_pitch, size_t width, size_t nrows)
{
    if (dst_pitch == width && src_pitch == width) {
        memcpy(dst, src, width * nrows);
        return;
    }
    for (size_t r = 0; r < nrows; ++r)
        memcpy(dst + r * dst_pitch, src + r * src_pitch, width);
}

// One Score::score_rows_into call on host matrices, f32 (a PSSM) or u8 (a DiscreteMatrix): `launch` enqueues the store
// kernels of `rows` rows whose first sequence row is at `d_seq`, dense output rows (stride = cols) at `d_out`.
struct ScoreCall {
    const uint8_t *seq;  // row `row_begin` of the caller's striped matrix
    size_t seq_stride, cols, nrows, halo;
    char *out;           // the caller's score matrix, row 0 of the range
    size_t out_stride;   // in elements
    size_t elem;         // bytes per score: 4 (f32) or 1 (u8)
    std::function<int(lm_hip_ctx *ctx, const uint8_t *d_seq, size_t rows, void *d_out)> launch;
};

// Rows [r0, r1) of the call on the lane's own buffers: copy up, score, copy down (the copies of pageable memory
// return when they are done), or for the tiniest pieces no copy command at all.  `*dev`: where the piece's (dense) scores
// are on the device.
int score_piece(HostLane *lane, const ScoreCall &c, size_t r0, size_t r1, const void **dev)
{
    lm_hip_ctx *ctx = lane->ctx;
    const size_t w = r1 - r0, in_bytes = (w + c.halo) * c.seq_stride, row_bytes = c.cols * c.elem, out_bytes = w * row_bytes;
    const uint8_t *src = c.seq + r0 * c.seq_stride;
    char *dst = c.out + r0 * c.out_stride * c.elem;
    if (lane->zc && in_bytes <= kZeroCopyBytes && out_bytes <= kZeroCopyBytes) {
        char *zout = reinterpret_cast<char *>(lane->zc_out());
        memcpy(lane->zc, src, in_bytes);
        LM_TRY(c.launch(ctx, lane->zc, w, zout));
        LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        copy_rows(dst, c.out_stride * c.elem, zout, row_bytes, row_bytes, w);
        *dev = zout;
        return LM_HIP_OK;
    }
    LM_TRY(lane->d_in.reserve(in_bytes + 64));
    LM_TRY(lane->d_out.reserve(out_bytes));
    uint8_t *d_in = static_cast<uint8_t *>(lane->d_in.ptr);
    char *d_out = static_cast<char *>(lane->d_out.ptr);
    LM_HIP_TRY(hipMemcpyAsync(d_in, src, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    LM_TRY(c.launch(ctx, d_in, w, d_out));
    // only the `cols` scored cells of each row: the caller's alignment padding is left as it was (pli/mod.rs:103)
    LM_HIP_TRY(c.out_stride == c.cols
                   ? hipMemcpyAsync(dst, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream)
                   : hipMemcpy2DAsync(dst, c.out_stride * c.elem, d_out, row_bytes, row_bytes, w, hipMemcpyDeviceToHost,
                                      ctx->stream));
    LM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *dev = d_out;
    return LM_HIP_OK;
}

// Link-bound: large calls of several threads take turns on the device's ring (run side by side through the runtime's
// pageable copies they were 2.2 x slower than one after the other -- profiles/r04_host_pointer.json).
int score_pipelined(HostLane *lane, const ScoreCall &c)
{
    lm_hip_ctx *ctx = lane->ctx;
    BigPipe &bp = big_pipe(ctx->device);
    std::lock_guard<std::mutex> pipe(bp.mu);
    LM_TRY(pipe_prepare(bp, ctx->device));
    const size_t tile_bytes = pipe_shape().tile_bytes, row_bytes = c.cols * c.elem;
    const TilePlan plan = plan_tiles(c.nrows, c.cols, c.elem, c.seq_stride, c.halo, tile_bytes);
    const size_t tr = plan.tr, in_tile = plan.in_tile, out_tile = plan.out_tile;
    if (!plan.fits)
        return LM_HIP_ERR_CAPACITY;
    LM_TRY(bp.d_in.reserve(kInSlots * in_tile + 64));
    LM_TRY(bp.d_out.reserve((size_t)pipe_shape().out_slots * out_tile));
    uint8_t *d_in = static_cast<uint8_t *>(bp.d_in.ptr);
    char *d_out = static_cast<char *>(bp.d_out.ptr);
    TileJob job;
    job.ntiles = plan.ntiles;
    auto width = [&](size_t t) { return std::min(tr, c.nrows - t * tr); };
    job.upload = [&](size_t t, int slot) {
        hipError_t e = hipMemcpyAsync(d_in + (size_t)slot * in_tile, c.seq + t * tr * c.seq_stride,
                                      (width(t) + c.halo) * c.seq_stride, hipMemcpyHostToDevice, bp.s_up);
        return e == hipSuccess ? hipStreamSynchronize(bp.s_up) : e;
    };
    job.compute = [&](size_t t, int is, int os) {
        return c.launch(ctx, d_in + (size_t)is * in_tile, width(t), d_out + (size_t)os * out_tile);
    };
    job.download = [&](size_t t, int slot) {
        return hipMemcpyAsync(bp.pinned + (size_t)slot * tile_bytes, d_out + (size_t)slot * out_tile, width(t) * row_bytes,
                              hipMemcpyDeviceToHost, bp.s_dn);
    };
    job.copy_out = [&](size_t t, int slot, int j, int n) {
        const size_t w = width(t), a = w * (size_t)j / (size_t)n, b = w * (size_t)(j + 1) / (size_t)n;
        copy_rows(c.out + (t * tr + a) * c.out_stride * c.elem, c.out_stride * c.elem,
                  bp.pinned + (size_t)slot * tile_bytes + a * row_bytes, row_bytes, row_bytes, b - a);
    };
    const int st = run_pipeline(ctx, bp, job);
    trim_if_large(bp.d_in);
    return st;
}

// The whole call: the tile pipeline for large score matrices, piece by piece on the lane otherwise.  `*whole`: where the
// call left its whole (dense) result on the device -- the lane's output buffer -- if it did, else nullptr.
int score_call(HostLane *lane, const ScoreCall &c, const void **whole)
{
    int st = LM_HIP_ERR_CAPACITY;
    *whole = nullptr;
    lane->kept.forget();  // the lane's buffers are about to be overwritten: whatever was kept is gone
    if (c.nrows * c.cols * c.elem >= kPipeMinOutBytes)
        st = score_pipelined(lane, c);
    if (st == LM_HIP_ERR_CAPACITY) {  // small (or a shape the tiles do not fit): piece by piece on this lane
        const size_t piece = piece_rows(c.cols, c.elem);
        st = LM_HIP_OK;
        for (size_t r0 = 0; r0 < c.nrows && st == LM_HIP_OK; r0 += piece)
            st = score_piece(lane, c, r0, std::min(c.nrows, r0 + piece), whole);
        if (st != LM_HIP_OK || c.nrows > piece)
            *whole = nullptr;
    }
    return st;
}

// The caller's score matrix on the device, dense (stride == cols): `*d` points into the lane's staging buffer.
int stage_scores(HostLane *lane, const float *scores, size_t rows, size_t stride, size_t cols, const float **d)
{
    hipStream_t stream = lane->ctx->stream;
    LM_TRY(lane->d_in.reserve(rows * cols * sizeof(float)));
    float *dev = static_cast<float *>(lane->d_in.ptr);
    LM_HIP_TRY(stride == cols ? hipMemcpyAsync(dev, scores, rows * cols * sizeof(float), hipMemcpyHostToDevice, stream)
                              : hipMemcpy2DAsync(dev, cols * sizeof(float), scores, stride * sizeof(float),
                                                 cols * sizeof(float), rows, hipMemcpyHostToDevice, stream));
    *d = dev;
    return LM_HIP_OK;
}

// The caller's StripedSequence on the lane's staging buffer, as a (borrowed) resident sequence: 1 B per position up.
int stage_sequence(HostLane *lane, const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols, size_t wrap,
                   size_t length, size_t k, lm_hip_seq *out)
{
    if (!seq || cols == 0 || seq_stride < cols || wrap > seq_rows_total)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan: bad sequence matrix (%zu rows, stride %zu, %zu columns, wrap %zu)",
                    seq_rows_total, seq_stride, cols, wrap);
    lm_hip_ctx *ctx = lane->ctx;
    const size_t bytes = seq_rows_total * seq_stride;
    LM_TRY(lane->d_in.reserve(bytes + 64));
    LM_HIP_TRY(hipMemcpyAsync(lane->d_in.ptr, seq, bytes, hipMemcpyHostToDevice, ctx->stream));
    out->device = ctx->device;
    out->d_data = static_cast<uint8_t *>(lane->d_in.ptr);
    out->capacity_rows = seq_rows_total;
    out->rows = seq_rows_total - wrap;
    out->wrap = wrap;
    out->stride = seq_stride;
    out->cols = cols;
    out->length = length;
    out->k = k;
    out->owns = false;
    return LM_HIP_OK;
}

}  // namespace

extern "C" {

// (Not through lane_call: what is remembered afterwards depends on what the end of the call -- lane_finish -- left on the lane.)
int lm_hip_score_f32(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols,
                     size_t wrap, size_t length, const float *pssm, size_t m, size_t pssm_stride,
                     size_t k, size_t row_begin, size_t row_end, float *out, size_t out_stride,
                     size_t *out_rows, size_t *max_index)
{
    return guarded("score", [&]() -> int {
        HostLane *lane = nullptr;
        LM_TRY(acquire_lane(&lane));
        lm_hip_ctx *ctx = lane->ctx;  // the lane is this thread's alone: nothing to lock
        DeviceGuard guard(ctx->device);
        lm_hip_pssm *p = nullptr;
        LM_TRY(lane_pssm(lane, pssm, m, pssm_stride, k, &p));
        LM_TRY(check_score_args(p, seq_rows_total, seq_stride, cols, wrap, row_begin, row_end));
        if (length < m || row_begin >= row_end) {  // pli/mod.rs:85-88
            if (out_rows) *out_rows = 0;
            if (max_index) *max_index = 0;
            return LM_HIP_OK;
        }
        if (!seq || !out || out_stride < cols)
            return fail(LM_HIP_ERR_BAD_ARGS, "score: null buffer or out stride %zu < columns %zu", out_stride, cols);
        // only the rows the range needs travel: [row_begin, row_end + m - 1)
        ScoreCall c{seq + row_begin * seq_stride, seq_stride, cols, row_end - row_begin, m ? m - 1 : 0,
                    reinterpret_cast<char *>(out), out_stride, sizeof(float), nullptr};
        // (lm_hip_host_reuse_scores: a matrix the tracking store kernel covers -- one piece, below 8 M cells -- is scored
        //  through the lane's own scores record, so that the argmax that follows reads the kernel's records)
        lm_hip_scores *t = c.nrows * cols < (8u << 20) ? lane->kept.tracker(ctx, cols) : nullptr;
        c.launch = [p, seq_stride, cols, t, whole = c.nrows](lm_hip_ctx *cx, const uint8_t *d_seq, size_t rows, void *d_out) {
            ScoreArgs a{p, d_seq, seq_stride, cols, 0, rows, static_cast<float *>(d_out), cols};
            if (!t || rows != whole)
                return launch_score_store(cx, a);
            t->d_data = static_cast<float *>(d_out);
            t->rows = rows;
            return score_store_tracked(cx, a, t);
        };
        const void *dev = nullptr;
        const int st = lane_finish(lane, score_call(lane, c, &dev));  // (dev stays nullptr when it fails)
        lane->kept.remember(*lane, static_cast<const float *>(dev), out, c.nrows, out_stride, cols);
        LM_TRY(st);
        if (out_rows) *out_rows = c.nrows;       // pli/mod.rs:91
        if (max_index) *max_index = length + 1 - m;
        return LM_HIP_OK;
    });
}

// Score<u8, A, C>::score_rows_into with a DiscreteMatrix on host matrices (pli/mod.rs:437-476 is the AVX2 impl; what
// Scanner::next calls per 256-row block, scan.rs:174-178).  `saturate`: avx2.rs:336 (adds_epu8) or Generic's wrapping `+=`.
int lm_hip_score_u8_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols, size_t wrap,
                         size_t length, const uint8_t *weights, size_t m, size_t weights_stride, size_t k,
                         size_t row_begin, size_t row_end, int saturate, uint8_t *out, size_t out_stride,
                         size_t *out_rows, size_t *max_index)
{
    return guarded("score_u8", [&]() -> int {
        if (!weights || m == 0 || k == 0 || k > 256 || weights_stride < k)
            return fail(LM_HIP_ERR_BAD_ARGS, "score_u8: bad discrete matrix (%zu x %zu, stride %zu)", m, k, weights_stride);
        lm_hip_pssm shape;  // the geometry checks only look at the motif length
        shape.m = m;
        shape.k = k;
        LM_TRY(check_score_args(&shape, seq_rows_total, seq_stride, cols, wrap, row_begin, row_end));
        if (length < m || row_begin >= row_end) {  // pli/mod.rs:85-88
            if (out_rows) *out_rows = 0;
            if (max_index) *max_index = 0;
            return LM_HIP_OK;
        }
        if (!seq || !out || out_stride < cols)
            return fail(LM_HIP_ERR_BAD_ARGS, "score_u8: null buffer or out stride %zu < columns %zu", out_stride, cols);
        ScoreCall c{seq + row_begin * seq_stride, seq_stride, cols, row_end - row_begin, m - 1, reinterpret_cast<char *>(out),
                    out_stride, 1, nullptr};
        c.launch = [=](lm_hip_ctx *cx, const uint8_t *d_seq, size_t rows, void *d_out) {
            // (the device tables of the matrix are kept by the lane's context until the weights change: launch_score_u8)
            DiscreteArgs a{weights, m, weights_stride, k, d_seq, seq_stride, cols, 0, rows, static_cast<uint8_t *>(d_out), cols,
                           saturate != 0};
            return launch_score_u8(cx, a);
        };
        const void *dev = nullptr;
        LM_TRY(lane_call("score_u8", [&](HostLane *lane, lm_hip_ctx *) { return score_call(lane, c, &dev); }));
        if (out_rows) *out_rows = c.nrows;
        if (max_index) *max_index = length + 1 - m;
        return LM_HIP_OK;
    });
}

// What the host-pointer path keeps between calls -- the pinned ring (128 MB), its device tiles, the staging buffers of
// lanes whose threads have exited and of the calling thread's own lane -- handed back; the next call sets them up again.
// Contexts, streams and cached PSSM tables stay.  Waits for a large call in flight on another thread.
int lm_hip_host_trim(void)
{
    return guarded("host_trim", [&]() -> int {
        trim_pipes();
        trim_lanes();
        return LM_HIP_OK;
    });
}

int lm_hip_host_reuse_count(size_t *count)
{
    return guarded("host_reuse_count", [&]() -> int {
        if (!count)
            return fail(LM_HIP_ERR_BAD_ARGS, "host_reuse_count: null argument");
        HostLane *lane = nullptr;
        LM_TRY(acquire_lane(&lane));
        *count = lane->reuses;
        return LM_HIP_OK;
    });
}

int lm_hip_host_lane_info(int *device, int *numa_node, int *helper_cpus)
{
    return guarded("host_lane_info", [&]() -> int {
        if (!device && !numa_node && !helper_cpus)
            return fail(LM_HIP_ERR_BAD_ARGS, "host_lane_info: no output asked for");
        HostLane *lane = nullptr;
        LM_TRY(acquire_lane(&lane));
        const NodeCpus &n = device_node(lane->ctx->device);
        if (device) *device = lane->ctx->device;
        if (numa_node) *numa_node = n.node;
        if (helper_cpus) *helper_cpus = n.valid ? CPU_COUNT(&n.set) : 0;
        return LM_HIP_OK;
    });
}

int lm_hip_argmax_f32(const float *scores, size_t rows, size_t stride, size_t cols, int *found,
                      lm_hip_coords *best, float *value)
{
    if (!found)
        return fail(LM_HIP_ERR_BAD_ARGS, "argmax: null argument");
    *found = 0;
    if (rows == 0)  // pli/mod.rs:136-138
        return LM_HIP_OK;
    if (!scores || cols == 0 || stride < cols)
        return fail(LM_HIP_ERR_BAD_ARGS, "argmax: bad matrix");
    return lane_call("argmax", [&](HostLane *lane, lm_hip_ctx *ctx) -> int {
        ScratchTrim scratch_trim(ctx);
        const float *d = lane->kept.lookup(*lane, scores, rows, stride, cols);
        if (lm_hip_scores *t = lane->kept.tracked_for(d, rows)) {
            // the store kernel that wrote the kept matrix tracked its best cell: fold / read its records (handles.hip)
            lm_hip_coords cell{0, 0};
            float v = 0.0f;
            LM_TRY(lm_hip_argmax(ctx, t, found, &cell, &v));
            if (*found) {
                if (best) *best = cell;
                if (value) *value = v;
            }
            return LM_HIP_OK;
        }
        ArgmaxRecord rec{};
        if (!d)
            LM_TRY(stage_scores(lane, scores, rows, stride, cols, &d));
        LM_TRY(launch_argmax(ctx, d, rows, cols, cols, 1, &rec));
        record_to_coords(rec, cols, found, best, value);
        return LM_HIP_OK;
    });
}

int lm_hip_max_f32(const float *scores, size_t rows, size_t stride, size_t cols, int *found, float *value)
{
    lm_hip_coords c{0, 0};
    return lm_hip_argmax_f32(scores, rows, stride, cols, found, &c, value);
}

int lm_hip_threshold_f32(const float *scores, size_t rows, size_t stride, size_t cols, float t,
                         lm_hip_coords **coords, size_t *n)
{
    if (!coords || !n)
        return fail(LM_HIP_ERR_BAD_ARGS, "threshold: null argument");
    *coords = nullptr;
    *n = 0;
    if (rows == 0)
        return LM_HIP_OK;
    if (!scores || cols == 0 || stride < cols)
        return fail(LM_HIP_ERR_BAD_ARGS, "threshold: bad matrix");
    return lane_call("threshold", [&](HostLane *lane, lm_hip_ctx *ctx) -> int {
        // a dense list grows ctx->scratch / scratch2 to 16 B per hit: handed back when the call ends (score_api.hip does the same)
        ScratchTrim scratch_trim(ctx);
        const float *d = lane->kept.lookup(*lane, scores, rows, stride, cols);
        if (!d)
            LM_TRY(stage_scores(lane, scores, rows, stride, cols, &d));
        return launch_threshold(ctx, d, rows, cols, cols, t, coords, n);
    });
}

// ---- Scanner on host matrices (scan.rs:166-249) ------------------------------------------------------------------------

int lm_hip_scan_f32_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols, size_t wrap, size_t length,
                         const float *pssm, size_t m, size_t pssm_stride, size_t k, float threshold, lm_hip_hit **hits,
                         size_t *n)
{
    if (!hits || !n)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan: null argument");
    *hits = nullptr;
    *n = 0;
    return lane_call("scan", [&](HostLane *lane, lm_hip_ctx *ctx) -> int {
        lm_hip_pssm *p = nullptr;
        LM_TRY(lane_pssm(lane, pssm, m, pssm_stride, k, &p));
        lm_hip_seq view;
        LM_TRY(stage_sequence(lane, seq, seq_rows_total, seq_stride, cols, wrap, length, k, &view));
        return lm_hip_scan_f32(ctx, p, &view, threshold, hits, n);  // synchronises
    });
}

int lm_hip_scan_max_f32_host(const uint8_t *seq, size_t seq_rows_total, size_t seq_stride, size_t cols, size_t wrap,
                             size_t length, const float *pssm, size_t m, size_t pssm_stride, size_t k,
                             const uint8_t *dweights, size_t dweights_stride, int saturate, unsigned level, int have,
                             size_t position, float score, size_t first_row, int *found, lm_hip_hit *best)
{
    if (!found || !best || !dweights)
        return fail(LM_HIP_ERR_BAD_ARGS, "scan_max: null argument");
    *found = 0;
    return lane_call("scan_max", [&](HostLane *lane, lm_hip_ctx *ctx) -> int {
        lm_hip_pssm *p = nullptr;
        LM_TRY(lane_pssm(lane, pssm, m, pssm_stride, k, &p));
        lm_hip_seq view;
        LM_TRY(stage_sequence(lane, seq, seq_rows_total, seq_stride, cols, wrap, length, k, &view));
        return lm_hip_scan_max_f32(ctx, p, &view, dweights, dweights_stride, saturate, level, have, position, score, first_row,
                                   found, best);
    });
}

}  // extern "C"
