// host_lane.hpp -- what the units of the host-pointer path share (not installed): the per-thread lane with its kept
// scores (host_lane.hip), the per-device tile pipeline of large calls (host_pipe.hip) and the scaffold of an entry point
// (hostptr.hip).  Declarations only, bar the two templates and the one-line inlines.
#pragma once

#include <functional>
#include <new>

#include "host_plan.hpp"
#include "lm_internal.hpp"

namespace lm::host {

struct HostLane;

// The f32 score matrix the last lm_hip_score_f32 of a lane left on the device, dense (lm_hip_host_reuse_scores): where it
// is, whose it was on the host, and a digest of a sample of what the caller got.  For matrices small enough for the
// tracking store kernel also the best cell that kernel found on the way: `track`, an lm_hip_scores record whose d_data is
// BORROWED from the lane's staging, never owned -- lm_hip_argmax_f32 on the kept matrix is then the fold of a few
// records, like lm_hip_argmax on a handle.
// INVARIANT: track->d_data is nullptr or dev, and "tracked" IS track->d_data == dev != nullptr: there is no flag beside the
// borrowed pointer that could disagree with it.  Only the operations below write the members.
struct KeptScores {
    // Nothing is kept, nothing tracked, no borrowed pointer left: before the lane's staging is overwritten, when the lane
    // changes hands, when what was kept turns out to be gone.
    void forget();
    // The lane's scores record readied for a store of `cols` dense columns (forgets what was kept); nullptr when the
    // switch is off or the record cannot be had -- the plain store runs then.
    lm_hip_scores *tracker(lm_hip_ctx *ctx, size_t cols);
    // After lm_hip_score_f32: its scores are at `dev` in one piece (nullptr: they are not, or the call failed); the store
    // kernel tracked them if it wrote them through tracker().  Kept if the switch is on and `dev` is still the lane's.
    void remember(const HostLane &lane, const float *dev, const float *host, size_t rows, size_t stride, size_t cols);
    // The device copy of `host` if the lane's previous score call produced exactly this matrix (same pointer and shape,
    // same sampled contents) and the buffer is still there -- counted in lane.reuses; nullptr otherwise.
    const float *lookup(HostLane &lane, const float *host, size_t rows, size_t stride, size_t cols);
    // The record of the store kernel that wrote `d` (a lookup's answer), if it tracked the best cell of these `rows` rows.
    lm_hip_scores *tracked_for(const float *d, size_t rows) const;

private:
    const float *dev = nullptr, *host = nullptr;
    size_t rows = 0, cols = 0, stride = 0;
    uint64_t digest = 0;
    lm_hip_scores *track = nullptr;
};

struct CachedPssm {
    uint64_t hash = 0, stamp = 0;
    lm_hip_pssm *p = nullptr;
};

struct HostLane {
    lm_hip_ctx *ctx = nullptr;  // (its device is the lane's)
    Scratch d_in, d_out;
    uint8_t *zc = nullptr;  // 2 x kZeroCopyBytes, pinned and device-visible: symbols in the first half, scores in the second
    std::vector<CachedPssm> pssms;
    uint64_t stamp = 0, trim_epoch = 0;  // the LRU clock of `pssms`; the trim epoch as of this lane's last trim
    KeptScores kept;
    size_t reuses = 0;

    uint8_t *zc_out() const { return zc + kZeroCopyBytes; }
    // is `dev` where a score call of this lane leaves its result: the zero-copy output half, or the output staging as it is now
    bool is_output(const void *dev) const { return (zc && dev == zc_out()) || dev == d_out.ptr; }
};

int acquire_lane(HostLane **out);
// The lane's device tables for this matrix: built on first sight, found again by hash + full comparison.
int lane_pssm(HostLane *lane, const float *w, size_t m, size_t stride, size_t k, lm_hip_pssm **out);
// lm_hip_host_trim: everything the idle lanes and the calling thread's own hold on the device but context, stream and PSSM
// tables goes back; every other lane owes the same at the end of its next call
void trim_lanes();
inline void trim_if_large(Scratch &s) { if (s.bytes > kKeepBytes) s.release(); }

struct NodeCpus {
    int node = -1;
    bool valid = false;  // `set` = the node's CPUs inside the process's own affinity mask, non-empty
    cpu_set_t set;
};
const NodeCpus &device_node(int device);

// ---- the tile pipeline of large calls (host_pipe.hip) -------------------------------------------------------------------

constexpr int kInSlots = 3, kOutSlots = 4, kCopiers = 4;
constexpr int kMaxOutSlots = 8;

// Shape of the pipeline.  Shipped: the constants above; a -DLM_HIP_DEV_SWITCHES build (tools/build_variant.py) reads
// LM_HIP_PIPE_{TILE_MB,OUT_SLOTS,COPIERS} once, for sweeps (tools/hostpipe_sweep.sh).
struct PipeShape {
    size_t tile_bytes = kTileBytes;
    int out_slots = kOutSlots, copiers = kCopiers;
};
const PipeShape &pipe_shape();

struct BigPipe {
    std::mutex mu;  // one large call at a time
    int device = -1;
    hipStream_t s_up = nullptr, s_dn = nullptr;
    hipEvent_t events[kInSlots + kMaxOutSlots] = {};
    hipEvent_t *const kdone = events, *const landed = events + kInSlots;  // per input slot / per output slot
    Scratch d_in, d_out;
    char *pinned = nullptr;  // out_slots x tile_bytes
};
// one per device (process lifetime)
BigPipe &big_pipe(int device);
// Streams, events and the pinned ring of `bp` on `device`; pipe_release is the inverse (both under bp.mu).
int pipe_prepare(BigPipe &bp, int device);
void pipe_release(BigPipe &bp);
// lm_hip_host_trim: pipe_release on every device's pipe (waits for a large call in flight)
void trim_pipes();

// One pipelined job: `upload` (uploader thread; blocks until tile t is in input slot `slot`), `compute` (calling
// thread: enqueues tile t's kernels on the lane's stream), `download` (calling thread: enqueues the copy of output
// slot `slot` into the pinned slot on bp.s_dn) and `copy_out` (copier j of n: its share of tile t, pinned -> caller).
struct TileJob {
    size_t ntiles = 0;
    std::function<hipError_t(size_t t, int slot)> upload;
    std::function<int(size_t t, int in_slot, int out_slot)> compute;
    std::function<hipError_t(size_t t, int slot)> download;
    std::function<void(size_t t, int slot, int j, int n)> copy_out;
};
int run_pipeline(lm_hip_ctx *ctx, BigPipe &bp, const TileJob &job);

// ---- the scaffold of an entry point --------------------------------------------------------------------------------------

// No C++ exception may cross the C ABI (std::bad_alloc from a table cache or a job closure, std::system_error from a thread).
template <class Body>
int guarded(const char *what, Body body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(LM_HIP_ERR_OOM, "%s: out of host memory", what);
    } catch (const std::exception &ex) {
        return fail(LM_HIP_ERR_HIP, "%s: %s", what, ex.what());
    }
}

// How every call on a lane ends: nothing of a failed call stays in flight; staging above the keep threshold goes back and,
// after an lm_hip_host_trim on another thread, everything does.  -> st
int lane_finish(HostLane *lane, int st);

// One call on the calling thread's lane (the lane is this thread's alone: nothing to lock): body(lane, ctx) -> status,
// with the lane's device current.
template <class Body>
int lane_call(const char *what, Body body)
{
    return guarded(what, [&]() -> int {
        HostLane *lane = nullptr;
        LM_TRY(acquire_lane(&lane));
        DeviceGuard guard(lane->ctx->device);
        return lane_finish(lane, body(lane, lane->ctx));
    });
}

}  // namespace lm::host
