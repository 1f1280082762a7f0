// host_pipe.hip -- the tile pipeline of large host-pointer calls (hostptr.hip: >= 96 MB of scores, link-bound).
//
// Three stages over row tiles: an uploader thread copies tile t + 1 .. t + 3 (pageable H2D, 56 GB/s) while the store kernel
// of tile t runs and tile t - 1 travels back.  The way back is the long one (4 B per position): the runtime's pageable D2H
// reaches 48 GB/s, a copy into pinned memory 56.6 GB/s -- so tiles land in a ring of four pinned 32 MB buffers and four
// copier threads move them into the caller's matrix while the next tiles are in flight (measured: hostpipe_bench,
// profiles/r04_hostpipe_bench.txt).  The ring, its streams and the device tile buffers exist once per DEVICE: large calls
// of several threads on one device take turns on it (the link is the bound; side by side they only get in each other's
// way), calls on different devices run side by side.  The ring is allocated, and the uploader / copier threads run, on the
// CPUs of the GPU's NUMA node (/sys/bus/pci/devices/<bdf>/numa_node), inside the affinity mask the process already has.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <thread>

#include <pthread.h>

#include "host_lane.hpp"

namespace lm::host {

const PipeShape &pipe_shape()
{
    static const PipeShape shape = [] {
        PipeShape s;
#ifdef LM_HIP_DEV_SWITCHES
        if (const char *e = getenv("LM_HIP_PIPE_TILE_MB"))
            s.tile_bytes = (size_t)std::max(1, std::min(atoi(e), 256)) << 20;
        if (const char *e = getenv("LM_HIP_PIPE_OUT_SLOTS"))
            s.out_slots = std::max(2, std::min(atoi(e), kMaxOutSlots));
        if (const char *e = getenv("LM_HIP_PIPE_COPIERS"))
            s.copiers = std::max(1, std::min(atoi(e), 32));
#endif
        return s;
    }();
    return shape;
}

namespace {
struct Pipes {
    std::mutex mu;
    std::vector<BigPipe *> list;
};
Pipes &pipes()
{
    static Pipes *p = new Pipes();
    return *p;
}

// helper threads only (never the caller's own thread)
void bind_this_thread_to_node(int device)
{
    const NodeCpus &n = device_node(device);
    if (n.valid)
        (void)pthread_setaffinity_np(pthread_self(), sizeof n.set, &n.set);
}
}  // namespace

BigPipe &big_pipe(int device)
{
    std::lock_guard<std::mutex> lock(pipes().mu);
    std::vector<BigPipe *> &v = pipes().list;
    if ((size_t)device >= v.size())
        v.resize((size_t)device + 1, nullptr);
    if (!v[(size_t)device])
        v[(size_t)device] = new BigPipe();
    return *v[(size_t)device];
}

int pipe_prepare(BigPipe &bp, int device)
{
    if (bp.device == device)
        return LM_HIP_OK;
    if (bp.device >= 0)  // (cannot happen: one pipe per device) -- the caller falls back to pieces on its own lane
        return LM_HIP_ERR_CAPACITY;
    bp.device = device;  // (made in place: pipe_release undoes whatever part of it exists)
    hipError_t e = hipStreamCreateWithFlags(&bp.s_up, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&bp.s_dn, hipStreamNonBlocking);
    for (hipEvent_t &ev : bp.events)
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) {
        // the ring's pages come from the node of the thread that allocates them (first touch under the default policy):
        // allocate from a thread that sits on the GPU's node, so the DMA writes and the copiers' reads stay on one socket
        const size_t bytes = (size_t)pipe_shape().out_slots * pipe_shape().tile_bytes;
        auto alloc = [&] {
            if (hipSetDevice(device) != hipSuccess) {
                e = hipGetLastError();
                return;
            }
            bind_this_thread_to_node(device);
            e = hipHostMalloc(reinterpret_cast<void **>(&bp.pinned), bytes, hipHostMallocDefault);
        };
        if (device_node(device).valid) {
            try {
                std::thread(alloc).join();
            } catch (const std::exception &) {
                alloc();  // no thread to be had: from here, wherever this thread runs
            }
        } else {
            e = hipHostMalloc(reinterpret_cast<void **>(&bp.pinned), bytes, hipHostMallocDefault);
        }
    }
    if (e != hipSuccess) {  // nothing half-made is kept
        pipe_release(bp);
        return fail(e == hipErrorOutOfMemory ? LM_HIP_ERR_OOM : LM_HIP_ERR_HIP, "host pipeline set-up failed: %s",
                    hipGetErrorString(e));
    }
    return LM_HIP_OK;
}

void pipe_release(BigPipe &bp)
{
    if (bp.device < 0)
        return;
    DeviceGuard guard(bp.device);
    for (hipStream_t s : {bp.s_up, bp.s_dn})
        if (s)
            (void)hipStreamSynchronize(s);
    bp.d_in.release();
    bp.d_out.release();
    for (hipEvent_t &ev : bp.events) {
        if (ev)
            (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    for (hipStream_t s : {bp.s_up, bp.s_dn})
        if (s)
            (void)hipStreamDestroy(s);
    (void)hipHostFree(bp.pinned);  // (nullptr: nothing happens)
    bp.s_up = bp.s_dn = nullptr;
    bp.pinned = nullptr;
    bp.device = -1;
}

void trim_pipes()
{
    std::vector<BigPipe *> all;
    {
        std::lock_guard<std::mutex> lock(pipes().mu);
        all = pipes().list;
    }
    for (BigPipe *bp : all)
        if (bp) {
            std::lock_guard<std::mutex> pipe(bp->mu);
            pipe_release(*bp);
        }
}

int run_pipeline(lm_hip_ctx *ctx, BigPipe &bp, const TileJob &job)
{
    struct Shared {
        std::mutex mu;
        std::condition_variable cv;
        size_t uploaded = 0, launched = 0, issued = 0, copied = 0;
        unsigned done[kMaxOutSlots] = {};
        int status = LM_HIP_OK;
        char err[256] = "";
    } sh;
    auto raise_text = [&](int status, const char *fmt, auto... args) {  // the first error stands; everyone wakes up
        std::lock_guard<std::mutex> lock(sh.mu);
        if (sh.status == LM_HIP_OK) {
            sh.status = status;
            snprintf(sh.err, sizeof sh.err, fmt, args...);
        }
        sh.cv.notify_all();
    };
    auto raise = [&](int status, const char *what, hipError_t e) { raise_text(status, "%s failed: %s", what, hipGetErrorString(e)); };
    const int device = ctx->device, out_slots = pipe_shape().out_slots, ncopiers = pipe_shape().copiers;
    const size_t n = job.ntiles;
#ifdef LM_HIP_DEV_SWITCHES  // where the wall time of a large call goes (LM_HIP_PIPE_TRACE=1)
    std::atomic<long long> ns_up_wait{0}, ns_up_copy{0}, ns_main_wait{0}, ns_cp_wait{0}, ns_cp_copy{0};
    auto tick = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t0) {
        return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    };
    const auto t_start = tick();
#define LM_PIPE_T0 const auto _t0 = tick()
#define LM_PIPE_ADD(counter) counter += since(_t0)
#else
#define LM_PIPE_T0 (void)0
#define LM_PIPE_ADD(counter) (void)0
#endif
    std::thread uploader;
    std::vector<std::thread> copiers;
    auto abandon = [&](const char *why) {  // a helper thread could not be started: stop the ones that were, report
        raise_text(LM_HIP_ERR_OOM, "host pipeline: %s", why);
        if (uploader.joinable())
            uploader.join();
        for (std::thread &c : copiers)
            if (c.joinable())
                c.join();
        return fail(LM_HIP_ERR_OOM, "%s", sh.err);
    };
    auto upload_loop = [&] {
        if (hipSetDevice(device) != hipSuccess)
            return raise(LM_HIP_ERR_HIP, "hipSetDevice", hipGetLastError());
        bind_this_thread_to_node(device);
        for (size_t t = 0; t < n; ++t) {
            hipError_t e = hipSuccess;
            {   // input slot t % kInSlots was read by tile t - kInSlots: its kernel must have been launched ...
                LM_PIPE_T0;
                std::unique_lock<std::mutex> lock(sh.mu);
                sh.cv.wait(lock, [&] { return sh.launched + kInSlots > t || sh.status != LM_HIP_OK; });
                if (sh.status != LM_HIP_OK)
                    return;
                lock.unlock();
                e = t >= (size_t)kInSlots ? hipEventSynchronize(bp.kdone[t % kInSlots]) : hipSuccess;  // ... and have finished
                LM_PIPE_ADD(ns_up_wait);
            }
            if (e == hipSuccess) {
                LM_PIPE_T0;
                e = job.upload(t, (int)(t % kInSlots));
                LM_PIPE_ADD(ns_up_copy);
            }
            if (e != hipSuccess)
                return raise(e == hipErrorOutOfMemory ? LM_HIP_ERR_OOM : LM_HIP_ERR_HIP, "tile upload", e);
            std::lock_guard<std::mutex> lock(sh.mu);
            sh.uploaded = t + 1;
            sh.cv.notify_all();
        }
    };
    auto copy_loop = [&](int j) {
        if (hipSetDevice(device) != hipSuccess)
            return raise(LM_HIP_ERR_HIP, "hipSetDevice", hipGetLastError());
        bind_this_thread_to_node(device);
        for (size_t t = 0; t < n; ++t) {
            const int slot = (int)(t % (size_t)out_slots);
            {
                LM_PIPE_T0;
                std::unique_lock<std::mutex> lock(sh.mu);
                sh.cv.wait(lock, [&] { return sh.issued > t || sh.status != LM_HIP_OK; });
                if (sh.status != LM_HIP_OK)
                    return;
                lock.unlock();
                const hipError_t e = hipEventSynchronize(bp.landed[slot]);
                if (e != hipSuccess)
                    return raise(LM_HIP_ERR_HIP, "tile read-back", e);
                LM_PIPE_ADD(ns_cp_wait);
            }
            {
                LM_PIPE_T0;
                job.copy_out(t, slot, j, ncopiers);
                LM_PIPE_ADD(ns_cp_copy);
            }
            std::lock_guard<std::mutex> lock(sh.mu);
            if (++sh.done[slot] == (unsigned)ncopiers) {
                sh.done[slot] = 0;
                sh.copied = t + 1;
                sh.cv.notify_all();
            }
        }
    };
    try {
        uploader = std::thread(upload_loop);
        for (int j = 0; j < ncopiers; ++j)
            copiers.emplace_back(copy_loop, j);
    } catch (const std::exception &ex) {  // std::system_error: no more threads
        return abandon(ex.what());
    }
    for (size_t t = 0; t < n; ++t) {
        {   // tile t is on the device, and output slot t % out_slots (device + pinned) has been emptied into the caller's matrix
            LM_PIPE_T0;
            std::unique_lock<std::mutex> lock(sh.mu);
            sh.cv.wait(lock, [&] { return (sh.uploaded > t && sh.copied + (size_t)out_slots > t) || sh.status != LM_HIP_OK; });
            if (sh.status != LM_HIP_OK)
                break;
            LM_PIPE_ADD(ns_main_wait);
        }
        const int is = (int)(t % kInSlots), os = (int)(t % (size_t)out_slots);
        const int st = job.compute(t, is, os);
        if (st != LM_HIP_OK) {
            raise_text(st, "%s", lm_hip_last_error());
            break;
        }
        hipError_t e = hipEventRecord(bp.kdone[is], ctx->stream);
        if (e == hipSuccess) {
            std::lock_guard<std::mutex> lock(sh.mu);
            sh.launched = t + 1;
            sh.cv.notify_all();
        }
        if (e == hipSuccess)
            e = hipStreamWaitEvent(bp.s_dn, bp.kdone[is], 0);
        if (e == hipSuccess)
            e = job.download(t, os);
        if (e == hipSuccess)
            e = hipEventRecord(bp.landed[os], bp.s_dn);
        if (e != hipSuccess) {
            raise(LM_HIP_ERR_HIP, "tile launch", e);
            break;
        }
        std::lock_guard<std::mutex> lock(sh.mu);
        sh.issued = t + 1;
        sh.cv.notify_all();
    }
    uploader.join();
    for (std::thread &c : copiers)
        c.join();
    // whatever happened, nothing may still be in flight into the ring or out of the tile buffers when this returns
    (void)hipStreamSynchronize(bp.s_up);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(bp.s_dn);
#ifdef LM_HIP_DEV_SWITCHES
    if (getenv("LM_HIP_PIPE_TRACE"))
        fprintf(stderr, "[lm_hip pipe] %zu tiles in %.2f ms: uploader waits %.2f copies %.2f | caller waits %.2f | copiers (each of %d) wait %.2f copy %.2f\n",
                n, since(t_start) * 1e-6, ns_up_wait * 1e-6, ns_up_copy * 1e-6, ns_main_wait * 1e-6, ncopiers,
                ns_cp_wait * 1e-6 / ncopiers, ns_cp_copy * 1e-6 / ncopiers);
#endif
#undef LM_PIPE_T0
#undef LM_PIPE_ADD
    if (sh.status != LM_HIP_OK)
        return fail(sh.status, "%s", sh.err);
    return LM_HIP_OK;
}

}  // namespace lm::host
