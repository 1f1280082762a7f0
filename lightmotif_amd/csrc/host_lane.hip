// host_lane.hip -- the lanes of the host-pointer path (hostptr.hip): which device a lane lives on, what it keeps between
// calls (staging, device PSSM tables, the last score matrix) and when it hands that back, and the NUMA node of a device.
//
// Every host thread that calls in gets a lane of its own; a lane whose thread has exited is handed to the next new thread.
// New lanes go to the process's HOME device -- the HIP device current in the thread that made the first unbound call --
// unless lm_hip_host_spread_lanes(1) deals them round-robin over the usable devices (a single process driving a whole
// node: the reference CLI's worker threads over (motif, sequence) jobs, lightmotif-cli main.rs:240-378, 502-524);
// $LM_HIP_DEVICE (read once) pins every lane to one ordinal, lm_hip_host_bind_thread one thread.
#include <atomic>
#include <cctype>
#include <cstdio>

#include "host_lane.hpp"

namespace lm::host {
namespace {

constexpr size_t kPssmCache = 16;

// lm_hip_host_reuse_scores: off unless the embedder asks for it
std::atomic<bool> g_reuse_scores{false};

// lm_hip_host_trim bumps it: a lane that belongs to a live thread hands its staging back at the end of its next call
std::atomic<uint64_t> g_trim_epoch{0};

// process lifetime (never destroyed: host threads may still be inside the library when the process exits)
struct IdleLanes {
    std::mutex mu;
    std::vector<HostLane *> list;
};
IdleLanes &idle_lanes()
{
    static IdleLanes *idle = new IdleLanes();
    return *idle;
}

struct LaneRef {
    HostLane *lane = nullptr;
    int want_device = -1;  // lm_hip_host_bind_thread
    ~LaneRef()
    {
        if (lane) {  // the thread is gone; its lane (stream idle: every call synchronises) serves the next one
            std::lock_guard<std::mutex> lock(idle_lanes().mu);
            idle_lanes().list.push_back(lane);
        }
    }
};
thread_local LaneRef t_lane;

// $LM_HIP_DEVICE, read ONCE per process: every lane on that ordinal (-1: not set, -2: set to something that is no ordinal)
int env_device()
{
    static const int dev = [] {
        const char *e = getenv("LM_HIP_DEVICE");
        if (!e || !*e)
            return -1;
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        return (end && *end == 0 && v >= 0 && v < 4096) ? (int)v : -2;
    }();
    return dev;
}

// HIP ordinals of the usable (gfx950) devices, in ordinal order
const std::vector<int> &usable_devices()
{
    static const std::vector<int> *list = [] {
        auto *v = new std::vector<int>();
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess)
            n = 0;
        for (int d = 0; d < n; ++d) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
                v->push_back(d);
        }
        return v;
    }();
    return *list;
}

bool is_usable(int dev)
{
    const std::vector<int> &devs = usable_devices();
    return std::find(devs.begin(), devs.end(), dev) != devs.end();
}

// lm_hip_host_spread_lanes: new lanes are dealt over every usable device in turn (a single process driving a whole node:
// the reference CLI's worker threads, main.rs:240-378).  Off by default: a job of one process per GPU with every GPU visible
// must not open contexts, pinned rings and PSSM caches on its neighbours' devices just because it scores from two threads.
std::atomic<int> g_spread{0};

// Device of a NEW lane: the thread's binding, else $LM_HIP_DEVICE, else -- spread on -- the next usable device in turn, else
// the process's host-pointer device: the HIP device current in the thread that made the FIRST unbound call (what a rank set
// with hipSetDevice / torch.cuda.set_device before it started scoring; ordinal 0 if it never did).
int pick_device(int *out)
{
    static std::atomic<unsigned> next{0};
    static std::atomic<int> home{-1};
    if (t_lane.want_device >= 0) {
        *out = t_lane.want_device;
    } else if (env_device() != -1) {
        if (env_device() < 0 || !is_usable(env_device()))
            return fail(LM_HIP_ERR_NO_DEVICE, "LM_HIP_DEVICE does not name a usable gfx950 device (lm_hip_device_ordinal lists them)");
        *out = env_device();
    } else {
        const std::vector<int> &devs = usable_devices();
        if (devs.empty())
            return fail(LM_HIP_ERR_NO_DEVICE, "no gfx950 device available");
        if (g_spread.load(std::memory_order_relaxed)) {
            *out = devs[next.fetch_add(1, std::memory_order_relaxed) % devs.size()];
        } else {
            int h = home.load(std::memory_order_acquire);
            if (h < 0) {
                int cur = 0;
                if (hipGetDevice(&cur) != hipSuccess || !is_usable(cur))
                    cur = devs[0];
                int expected = -1;
                home.compare_exchange_strong(expected, cur, std::memory_order_acq_rel);
                h = home.load(std::memory_order_acquire);
            }
            *out = h;
        }
    }
    return LM_HIP_OK;
}

NodeCpus probe_node(int device)
{
    NodeCpus out;
    CPU_ZERO(&out.set);
    char bdf[64] = "";
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) {
        (void)hipGetLastError();
        return out;
    }
    for (char *c = bdf; *c; ++c)
        *c = (char)tolower((unsigned char)*c);
    char path[160], text[4096] = "";
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    if (!f)
        return out;
    if (fscanf(f, "%d", &out.node) != 1)
        out.node = -1;
    fclose(f);
    if (out.node < 0)
        return out;  // the platform reports no affinity (single node, or a VM): nothing to bind to
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", out.node);
    f = fopen(path, "r");
    if (!f)
        return out;
    const bool got = fgets(text, sizeof text, f) != nullptr;
    fclose(f);
    cpu_set_t node_set, mine;
    if (!got || !parse_cpulist(text, &node_set) || sched_getaffinity(0, sizeof mine, &mine) != 0)
        return out;
    CPU_AND(&out.set, &node_set, &mine);  // never outside what the process was given (taskset, cgroup cpusets)
    out.valid = CPU_COUNT(&out.set) > 0;
    return out;
}

}  // namespace

// ---- the kept scores of a lane ------------------------------------------------------------------------------------------

void KeptScores::forget()
{
    dev = nullptr;
    if (track)
        track->d_data = nullptr;
}

lm_hip_scores *KeptScores::tracker(lm_hip_ctx *ctx, size_t ncols)
{
    forget();
    if (!g_reuse_scores.load(std::memory_order_relaxed))
        return nullptr;
    if (!track && lm_hip_scores_create(ctx, ncols, &track) != LM_HIP_OK)
        return nullptr;  // (track is still nullptr)
    track->cols = track->stride = ncols;  // (d_data: nullptr since forget(), or from the start)
    track->capacity_rows = 0;  // (nothing of its own to free or to grow)
    track->rows = 0;
    return track->d_best ? track : nullptr;
}

void KeptScores::remember(const HostLane &lane, const float *d, const float *h, size_t nrows, size_t nstride, size_t ncols)
{
    if (!g_reuse_scores.load(std::memory_order_relaxed) || !d || !lane.is_output(d))  // (the call's own trim handed the buffer back)
        return forget();
    dev = d;
    host = h;
    rows = nrows;
    cols = ncols;
    stride = nstride;
    digest = sample_digest(h, nrows, nstride, ncols);
}

const float *KeptScores::lookup(HostLane &lane, const float *h, size_t nrows, size_t nstride, size_t ncols)
{
    if (!dev || !g_reuse_scores.load(std::memory_order_relaxed) || host != h || rows != nrows || cols != ncols || stride != nstride)
        return nullptr;  // nothing kept, or another matrix: uploaded to the lane's INPUT staging, what is kept stays
    if (!lane.is_output(dev) ||  // (trimmed or re-allocated since)
        digest != sample_digest(h, nrows, nstride, ncols)) {
        forget();
        return nullptr;
    }
    ++lane.reuses;
    return dev;
}

lm_hip_scores *KeptScores::tracked_for(const float *d, size_t nrows) const
{
    return d && d == dev && track && track->d_data == d && track->rows == nrows ? track : nullptr;
}

// ---- lanes --------------------------------------------------------------------------------------------------------------

int acquire_lane(HostLane **out)
{
    const int demanded = t_lane.want_device >= 0 ? t_lane.want_device : env_device();
    if (t_lane.lane && demanded >= 0 && t_lane.lane->ctx->device != demanded) {  // re-bound: this lane serves someone else
        std::lock_guard<std::mutex> lock(idle_lanes().mu);
        idle_lanes().list.push_back(t_lane.lane);
        t_lane.lane = nullptr;
    }
    if (!t_lane.lane) {
        {
            std::lock_guard<std::mutex> lock(idle_lanes().mu);
            std::vector<HostLane *> &idle = idle_lanes().list;
            for (size_t i = idle.size(); i-- > 0;)
                if (demanded < 0 || idle[i]->ctx->device == demanded) {
                    t_lane.lane = idle[i];
                    t_lane.lane->kept.forget();  // (what another thread's call left behind is not this thread's)
                    t_lane.lane->reuses = 0;
                    idle.erase(idle.begin() + (long)i);
                    break;
                }
        }
        if (!t_lane.lane) {
            int dev = 0;
            LM_TRY(pick_device(&dev));
            lm_hip_ctx *ctx = nullptr;
            LM_TRY(lm_hip_ctx_create(dev, &ctx));
            HostLane *lane = new (std::nothrow) HostLane();
            if (!lane) {
                lm_hip_ctx_destroy(ctx);
                return fail(LM_HIP_ERR_OOM, "out of host memory");
            }
            lane->ctx = ctx;
            lane->trim_epoch = g_trim_epoch.load(std::memory_order_acquire);
            DeviceGuard guard(ctx->device);
            if (hipHostMalloc(reinterpret_cast<void **>(&lane->zc), 2 * kZeroCopyBytes, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                lane->zc = nullptr;  // tiny calls take the copy path then
            }
            t_lane.lane = lane;
        }
    }
    *out = t_lane.lane;
    return LM_HIP_OK;
}

int lane_pssm(HostLane *lane, const float *w, size_t m, size_t stride, size_t k, lm_hip_pssm **out)
{
    if (!w && m)
        return fail(LM_HIP_ERR_BAD_ARGS, "score: null pssm");
    if (k == 0 || k > 256 || stride < k)
        return fail(LM_HIP_ERR_BAD_ARGS, "score: bad alphabet size %zu / pssm stride %zu", k, stride);
    const uint64_t h = hash_weights(w, m, stride, k);
    for (CachedPssm &e : lane->pssms) {
        if (e.hash != h || e.p->m != m || e.p->k != k)
            continue;
        bool same = true;
        for (size_t j = 0; j < m && same; ++j)
            same = memcmp(&e.p->host[j * k], &w[j * stride], k * sizeof(float)) == 0;
        if (same) {
            e.stamp = ++lane->stamp;
            *out = e.p;
            return LM_HIP_OK;
        }
    }
    if (lane->pssms.size() >= kPssmCache) {  // the stream is idle between calls: safe to destroy
        size_t oldest = 0;
        for (size_t i = 1; i < lane->pssms.size(); ++i)
            if (lane->pssms[i].stamp < lane->pssms[oldest].stamp)
                oldest = i;
        lm_hip_pssm_destroy(lane->pssms[oldest].p);
        lane->pssms.erase(lane->pssms.begin() + (long)oldest);
    }
    lm_hip_pssm *p = nullptr;
    LM_TRY(lm_hip_pssm_create(lane->ctx, w, m, stride, k, &p));
    lane->pssms.push_back(CachedPssm{h, ++lane->stamp, p});
    *out = p;
    return LM_HIP_OK;
}

// Everything a lane holds on the device but its context, stream and PSSM tables (the stream is idle).
static void release_all(HostLane *lane)
{
    lane->d_in.release();
    lane->d_out.release();
    // the lane context's own scratch: reduction partials / hit lists, the chunk of a sliced u8 store
    lane->ctx->scratch.release();
    lane->ctx->scratch2.release();
    lane->ctx->chunk_scores.release();
    lane->ctx->scan_buf.release();
}

static void lane_trim(HostLane *lane)
{
    const uint64_t epoch = g_trim_epoch.load(std::memory_order_acquire);
    if (lane->trim_epoch != epoch) {
        lane->trim_epoch = epoch;
        release_all(lane);
        return;
    }
    trim_if_large(lane->d_in);
    trim_if_large(lane->d_out);
}

int lane_finish(HostLane *lane, int st)
{
    if (st != LM_HIP_OK)
        (void)hipStreamSynchronize(lane->ctx->stream);
    lane_trim(lane);
    return st;
}

void trim_lanes()
{
    {
        std::lock_guard<std::mutex> lock(idle_lanes().mu);
        std::vector<HostLane *> lanes = idle_lanes().list;  // idle: no thread owns them; they stay on the list
        if (t_lane.lane)
            lanes.push_back(t_lane.lane);
        for (HostLane *lane : lanes) {
            DeviceGuard guard(lane->ctx->device);
            (void)hipStreamSynchronize(lane->ctx->stream);
            release_all(lane);
        }
    }
    // lanes of threads that are still alive cannot be touched from here (their streams may be busy): they trim
    // themselves at the end of their next call
    g_trim_epoch.fetch_add(1, std::memory_order_release);
}

// ---- NUMA placement of the pipeline's helper threads and its pinned ring ------------------------------------------------

const NodeCpus &device_node(int device)
{
    static std::mutex mu;
    static std::vector<NodeCpus *> *cache = new std::vector<NodeCpus *>();
    std::lock_guard<std::mutex> lock(mu);
    if ((size_t)device >= cache->size())
        cache->resize((size_t)device + 1, nullptr);
    if (!(*cache)[(size_t)device])
        (*cache)[(size_t)device] = new NodeCpus(probe_node(device));
    return *(*cache)[(size_t)device];
}

}  // namespace lm::host

using namespace lm;
using namespace lm::host;

extern "C" {

int lm_hip_host_bind_thread(int device)
{
    return guarded("host_bind_thread", [&]() -> int {
        if (device >= 0 && !is_usable(device))
            return fail(LM_HIP_ERR_NO_DEVICE, "host_bind_thread: %d is not a usable (gfx950) device ordinal", device);
        t_lane.want_device = device < 0 ? -1 : device;  // takes effect at the thread's next host-pointer call
        return LM_HIP_OK;
    });
}

int lm_hip_host_spread_lanes(int enabled)
{
    g_spread.store(enabled != 0, std::memory_order_relaxed);  // lanes that exist stay where they are
    return LM_HIP_OK;
}

int lm_hip_host_reuse_scores(int enabled)
{
    g_reuse_scores.store(enabled != 0, std::memory_order_relaxed);
    return LM_HIP_OK;
}

}  // extern "C"
