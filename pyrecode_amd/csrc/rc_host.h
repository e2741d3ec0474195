// rc_host.h - host-side plumbing shared by the translation units behind the C ABI (rc_api.hip: contexts and seam 1;
// rc_reader.hip: the batched reader; rc_codec_api.hip: the stateless codec seams): status / error text, device guard, the owners of
// device and page-locked memory (DevMem / PinMem: every allocation of a ctx or a utility context is on its owner's list, so none can be
// forgotten when it is freed) with their growable buffers (DevBuf / PinBuf), the per-GPU utility context the stateless entry points
// share, and the staging helpers of those entry points (stage_in, StagedOut, HostView).  The few globals are defined in rc_api.hip.
// The library has no experiment switches.  What it reads from the environment are settings that tests use and that cannot produce a
// wrong record - RC_REDUCE_GUARDED_LOADS, RC_ZSTD_LITS_ALWAYS / RC_ZSTD_SEQ_ALWAYS - and plain tuning / measurement settings - RC_DEVICE,
// RC_DECODE_THREADS, RC_READ_THREADS, RC_PROFILE_ALL_STAGES, RC_READ_TIMING, RC_READ_SERIAL.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <algorithm>
#include <string>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <thread>
#include <sched.h>
#include <unistd.h>
#include <vector>

#include "../../include/recode_hip.h"
#include "rc_expand.h"
#include "rc_launch.h"
#include "rc_read_plan.h"
#include "rc_zstd_block.h"
#include "rc_zstd_dec.h"

#define RC_EXPORT extern "C" __attribute__((visibility("default")))

extern thread_local std::string g_last_error;   // rc_last_error(): one per thread, whichever translation unit failed

inline int fail(int code, const char *what)
{
    g_last_error = what ? what : "";
    return code;
}
inline int hip_fail(hipError_t e, const char *where)
{
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    if (e == hipErrorOutOfMemory) {   // the workspace does not fit this GPU's free memory: a status of its own, and no sticky HIP error left behind
        (void)hipGetLastError();
        return RC_ERR_WORKSPACE;
    }
    return RC_ERR_DEVICE;
}
#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);     \
    } while (0)

// ---- owners of device and page-locked memory -----------------------------------------------------------------------------
// Everything one object (a ctx, a utility context, a PinnedVec) allocated, as a list: alloc() writes the pointer into a plain field - a
// rc::Scratch member, say: the kernel argument stays a POD and its owner sits beside it -, free_one() gives one allocation back and
// clears the field, release_all() gives back the rest.  No destructor: rc_ctx_destroy releases a ctx's memory explicitly, behind its
// device guard and stream synchronisation, and the utility contexts (g_utils) are never freed - no HIP call may run during static
// destruction.
template <bool Device>
struct MemOwner {
    std::vector<void *> held;
    template <class T>
    hipError_t try_alloc(T *&field, uint64_t bytes, unsigned flags = hipHostMallocDefault)   // (flags: page-locked memory only)
    {
        void *p = nullptr;
        hipError_t e = Device ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) return e;
        held.push_back(p);
        field = static_cast<T *>(p);
        return hipSuccess;
    }
    // what: names the buffer in rc_last_error() when the allocation fails (RC_ALLOC passes the field and its size as written)
    template <class T>
    int alloc(T *&field, uint64_t bytes, const char *what = "a growable buffer", unsigned flags = hipHostMallocDefault)
    {
        hipError_t e = try_alloc(field, bytes, flags);
        return e == hipSuccess ? RC_OK : hip_fail(e, (std::string(Device ? "hipMalloc(" : "hipHostMalloc(") + what + ")").c_str());
    }
    static void release(void *p) { if (Device) (void)hipFree(p); else (void)hipHostFree(p); }
    template <class T>
    void free_one(T *&field)
    {
        auto it = std::find(held.begin(), held.end(), (void *)field);
        if (it != held.end()) { release(*it); held.erase(it); }
        field = nullptr;
    }
    void release_all()
    {
        for (void *p : held) release(p);
        held.clear();
    }
};
using DevMem = MemOwner<true>;
using PinMem = MemOwner<false>;

// A buffer of its owner that grows on demand and keeps its capacity: ensure(m, need) leaves at least `need` bytes (contents are not
// kept; a new allocation is need + extra bytes, so that a slowly growing demand does not allocate every call).
template <class Mem>
struct Buf {
    uint8_t *p = nullptr;
    uint64_t cap = 0;
    int ensure(Mem &m, uint64_t need, uint64_t extra = 0)
    {
        if (p && need <= cap) return RC_OK;
        m.free_one(p);
        cap = 0;
        int r = m.alloc(p, (need + extra) ? (need + extra) : 16);
        if (r == RC_OK) cap = need + extra;
        return r;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
using DevBuf = Buf<DevMem>;
using PinBuf = Buf<PinMem>;
#define RC_ALLOC(owner, field, bytes)                         \
    do {                                                      \
        int r_ = (owner).alloc(field, bytes, #field ", " #bytes); \
        if (r_ != RC_OK) return r_;                           \
    } while (0)

namespace {
// true when p is memory the GPU kernels can dereference (device or managed); false for ordinary host memory
bool is_device_ptr(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // unregistered host pointer: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

int copy_out(void *dst, const void *src_dev, uint64_t bytes, hipStream_t s)
{
    if (!bytes) return RC_OK;
    HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return RC_OK;
}

// CPUs this process may REALLY use: the scheduler affinity capped by the cgroup's CPU bandwidth quota (cgroup v2 cpu.max, v1
// cpu.cfs_quota_us / cpu.cfs_period_us) - the GPU boxes show 256 cores and grant 16; a pool sized from hardware_concurrency() spends the
// quota early in every accounting period and is throttled for the rest of it (pyrecode_amd/misc.py::effective_cpus is the Python twin).
uint32_t usable_cpus()
{
    static const uint32_t n = [] {
        uint32_t vis = 0;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) vis = (uint32_t)CPU_COUNT(&set);
        if (!vis) vis = std::max(1u, std::thread::hardware_concurrency());
        double quota = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0};
            long long period = 0;
            if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) quota = atof(q) / (double)period;
            fclose(f);
        } else {
            long long q = -1, period = 0;
            if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &q) != 1) q = -1; fclose(g); }
            if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &period) != 1) period = 0; fclose(g); }
            if (q > 0 && period > 0) quota = (double)q / (double)period;
        }
        if (quota > 0) vis = std::max(1u, std::min(vis, (uint32_t)(quota + 0.999)));
        return vis;
    }();
    return n;
}

// Every entry point runs on its ctx's (or the utility context's) device and puts the caller's current device back on
// return: in a one-process-per-GPU job the thread's current device belongs to the caller (torch, RCCL), not to this library.
struct DeviceGuard {
    int prev = -1;
    bool moved = false;
    hipError_t enter(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev == dev) return hipSuccess;
        hipError_t e = hipSetDevice(dev);
        moved = e == hipSuccess && prev >= 0;
        return e;
    }
    ~DeviceGuard() { if (moved) (void)hipSetDevice(prev); }
};
#define RC_ON_DEVICE(dev) DeviceGuard dev_guard_; HIP_TRY(dev_guard_.enter(dev))
}  // namespace

// ---- utility contexts for the stateless seams (2 and 3) ----------------------------------------------------------
// One per GPU, created on first use.  A call runs on RC_DEVICE (env) when that is set, otherwise on the CALLER'S CURRENT
// device - in a one-process-per-GPU job that is the rank's own GPU - and leaves the current device as it found it.
// (types with one shared instance each - defined in rc_api.hip - live at namespace scope; the helpers around them are per-TU)
// A few worker threads that stay around between calls (rc_expand_frames indexes its frames on them: starting 15 threads per call
// cost more than the indexing itself - 0.5 of 0.7 ms for 64 frames).  run(n, fn) calls fn(0..n-1), fn(0) on the calling thread, and
// returns when all are done; runs are serialised (callers on different devices share the pool).  Never destroyed: the workers sleep
// on a condition variable and end with the process.  A forked child starts its own.
struct WorkerPool {
    std::mutex mu, run_mu;
    std::condition_variable cv_go, cv_done;
    std::function<void(uint32_t)> fn;
    uint64_t generation = 0;
    uint32_t want = 0, done = 0;
    int started = 0;
    pid_t pid = 0;
    void worker(uint32_t id)
    {
        uint64_t seen = 0;
        for (;;) {
            std::function<void(uint32_t)> f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return generation != seen; });
                seen = generation;
                if (id >= want) continue;
                f = fn;
            }
            f(id);
            {
                std::lock_guard<std::mutex> lk(mu);
                ++done;
            }
            cv_done.notify_one();
        }
    }
    void run(uint32_t n, const std::function<void(uint32_t)> &f)
    {
        if (n <= 1) { if (n) f(0); return; }
        std::lock_guard<std::mutex> one_run(run_mu);
        {
            std::lock_guard<std::mutex> lk(mu);
            if (pid != getpid()) { started = 0; pid = getpid(); }   // (after a fork the parent's workers do not exist here)
            for (; started + 1 < (int)n; ++started) std::thread(&WorkerPool::worker, this, (uint32_t)started + 1).detach();
            fn = f;
            want = n;
            done = 1;   // id 0 runs here
            ++generation;
        }
        cv_go.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return done >= want; });
    }
};
extern WorkerPool *g_pool;

// Growable array in page-locked host memory (a hipMemcpyAsync from it is a real asynchronous copy; capacity is kept).
template <class T>
struct PinnedVec {
    PinMem mem;                         // its own owner: the indexing threads grow their vectors side by side
    T *p = nullptr; size_t n = 0, cap = 0;
    bool ok = true;                     // false: an allocation failed (checked by the caller after the indexing threads have joined)
    void clear() { n = 0; ok = true; }
    size_t size() const { return n; }
    const T *data() const { return p; }
    bool grow(size_t nc)
    {
        T *q = nullptr;
        if (mem.try_alloc(q, nc * sizeof(T), hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); ok = false; return false; }
        if (n) memcpy(q, p, n * sizeof(T));
        mem.free_one(p);
        p = q; cap = nc;
        return true;
    }
    // room for `want` entries up front: every doubling is a page-locked allocation (about a millisecond), and a reader's first
    // batches otherwise pay five or six of them per indexing thread
    void reserve(size_t want) { if (want > cap) (void)grow(want); }
    void push_back(const T &v)
    {
        if (n == cap && !grow(cap ? cap * 2 : 8192)) return;
        p[n++] = v;
    }
};
constexpr int RC_READ_THREADS = 16;
constexpr int RC_READ_SLOTS = 2;

// Everything one batch of the batched reader owns while it is in flight (rc_expand_frames uses slot 0; rc_expand_frames_submit /
// _wait alternate between the slots, so that the host walk and copy-in of one batch run while the device decodes the other).
// Kept between calls: no allocation and no first-touch page faults in steady state.
struct ReadRes {
    hipStream_t stream = nullptr, stream2 = nullptr;       // the two streams' decoders run side by side
    hipEvent_t ev_a = nullptr, ev_b = nullptr, done = nullptr;
    DevBuf d_stats;                                        // level-2 statistics staged for a host caller (rc_expand_frames_l2)
    DevBuf d_data, d_streams, d_head, d_counters, d_triplets;   // device (the utility context's DevMem): the stored bytes, the decoded streams,
                                                           // tables + per-frame index arrays, per-block counters, triplets staged for a host caller
    PinnedVec<rc::ZdBlock> rd_bm[RC_READ_THREADS], rd_pv[RC_READ_THREADS], rd_raw[RC_READ_THREADS];   // per indexing thread, page-locked
    std::vector<rc::ZdBlock> rd_tmp[RC_READ_THREADS];
    PinnedVec<uint32_t> rd_off[RC_READ_THREADS];           // compact lists of uniform binary-map streams: one header offset per block (k_bitmap_decode_c)
    PinBuf rd_head;                                        // page-locked (the utility context's PinMem): decoding tables + per-frame index arrays
    PinBuf h_res;                                          // ... nnz prefix (n + 1) and the error word, as the device left them (uint64)
    PinBuf h_blob;                                         // ... host copy of a DEVICE-resident input, for the header walk
    DevBuf d_inf;                                          // device inflate (rc_inflate.hip): stream descriptors, candidate / link / unit tables
    PinBuf h_inf;                                          // ... the descriptors as the host wrote them
    DevBuf d_count;                                        // electron counting (rc_count.hip): directory, union-find nodes, per-component sums, event counters
    // a submitted batch waiting for its rc_expand_frames_wait
    bool pending = false;
    uint32_t n = 0;
    rc::ReadKind kind = rc::RK_TRIPLETS;                   // what the batch leaves behind: the verdict's capacity rule and the copy-back plan follow from it
    uint64_t cap = 0, cell_bytes = 0;                      // (rc_read_plan.h; cell_bytes: a dense, trace, corr or bins output's size)
    uint8_t *late_dst = nullptr;                           // page-locked output rc_expand_frames_wait fills from d_triplets once the batch is known to be good
};

struct Util {
    std::mutex mu;
    int device = -1;
    hipStream_t stream = nullptr;
    DevMem dmem;                                // owns every device allocation below and in rr[]; never released (see MemOwner)
    PinMem hmem;                                // ... and the page-locked ones
    DevBuf a, b, o, w;                          // input 1, input 2, output, work
    uint64_t *h_scalar = nullptr;               // pinned
    void *ztab = nullptr;                       // zstd FSE tables (zstd_encoder_tables)
    DevBuf zd_out, zd_blocks, zd_tables, zd_ctl;   // rc_decompress(zstd): decoded bytes, block lists, the frame's tables, lists / base / error / produced
    void *zd_predef = nullptr;                  // predefined zstd decoding tables (zstd_predefined_tables)
    ReadRes rr[RC_READ_SLOTS + 1];              // the submit / wait form's two slots, then the synchronous rc_expand_frames' own:
                                                // a synchronous call (e.g. the reader's fallback for ONE batch) never meets a queued batch
};
constexpr int RC_MAX_DEV = 64;
extern Util g_utils[RC_MAX_DEV];
extern thread_local Util *t_util;
namespace {
#define g_util (*t_util)

struct UtilScope {
    DeviceGuard guard;
    std::unique_lock<std::mutex> lock;
    int enter()
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
            (void)hipGetLastError();
            return fail(RC_ERR_DEVICE, "no HIP device visible (this library has no CPU path)");
        }
        int dev = 0;
        const char *env = getenv("RC_DEVICE");
        if (env) dev = atoi(env);
        else if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
        if (dev < 0 || dev >= ndev || dev >= RC_MAX_DEV) return fail(RC_ERR_BAD_ARG, "RC_DEVICE out of range");
        t_util = &g_utils[dev];
        lock = std::unique_lock<std::mutex>(t_util->mu);
        HIP_TRY(guard.enter(dev));
        if (t_util->device < 0) {
            HIP_TRY(hipStreamCreateWithFlags(&t_util->stream, hipStreamNonBlocking));
            RC_ALLOC(t_util->hmem, t_util->h_scalar, 64);
            t_util->device = dev;
        }
        return RC_OK;
    }
};

// device-visible view of caller memory: the pointer itself, or a staged copy in `buf`
template <class T>
int stage_in(const T *src, uint64_t bytes, DevBuf &buf, const T *&dev, uint64_t pad = 0)
{
    if (is_device_ptr(src) && pad == 0) {
        dev = src;
        return RC_OK;
    }
    int r = buf.ensure(g_util.dmem, bytes + pad);
    if (r != RC_OK) return r;
    if (pad) HIP_TRY(hipMemsetAsync(buf.p + bytes, 0, pad, g_util.stream));
    if (bytes)
        HIP_TRY(hipMemcpyAsync(buf.p, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               g_util.stream));
    dev = reinterpret_cast<const T *>(buf.p);
    return RC_OK;
}

// Where a kernel of the utility context writes `bytes` of result the caller wants at `dst`: dst itself when the GPU can address it,
// otherwise the staging buffer g_util.o; finish() copies a staged result back and waits for the stream either way.
struct StagedOut {
    void *dev = nullptr;
    bool host = false;
    int begin(void *dst, uint64_t bytes)
    {
        host = !is_device_ptr(dst);
        dev = dst;
        if (!host) return RC_OK;
        int r = g_util.o.ensure(g_util.dmem, bytes);
        dev = g_util.o.p;
        return r;
    }
    template <class T> T *as() const { return static_cast<T *>(dev); }
    int finish(void *dst, uint64_t bytes)
    {
        if (host) HIP_TRY(hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, g_util.stream));
        HIP_TRY(hipStreamSynchronize(g_util.stream));
        return RC_OK;
    }
};

// Host view of a source that may lie in device memory (frame and block headers are walked on the host: sequential by format, a few
// bytes per block), with a little-endian dword reader.
struct HostView {
    std::vector<uint8_t> copy;
    const uint8_t *h = nullptr;
    int open(const uint8_t *src, uint64_t n)
    {
        h = src;
        if (!is_device_ptr(src)) return RC_OK;
        copy.resize(n);
        HIP_TRY(hipMemcpy(copy.data(), src, n, hipMemcpyDeviceToHost));
        h = copy.data();
        return RC_OK;
    }
    uint8_t operator[](uint64_t p) const { return h[p]; }
    uint32_t rd32(uint64_t p) const { return (uint32_t)h[p] | ((uint32_t)h[p + 1] << 8) | ((uint32_t)h[p + 2] << 16) | ((uint32_t)h[p + 3] << 24); }
};

// The zstd encoder's FSE tables (rc_zstd_block.h) in device memory of `m`, uploaded when `tab` is still empty: a ctx has its own copy,
// the utility context one per GPU.
int zstd_encoder_tables(DevMem &m, void *&tab)
{
    if (tab) return RC_OK;
    std::vector<uint8_t> t(rc::zstd_tables_bytes());
    rc::zstd_tables_host(t.data());
    void *d = nullptr;
    int r = m.alloc(d, t.size(), "the zstd encoder tables");
    if (r != RC_OK) return r;
    HIP_TRY(hipMemcpy(d, t.data(), t.size(), hipMemcpyHostToDevice));
    tab = d;
    return RC_OK;
}
// The predefined zstd decoding tables (rc_zstd_dec.h) of the utility context, uploaded on first use.
int zstd_predefined_tables(Util &u)
{
    if (u.zd_predef) return RC_OK;
    std::vector<uint8_t> t(rc::zd_tables_bytes());
    rc::zd_predefined_tables(t.data());
    void *d = nullptr;
    int r = u.dmem.alloc(d, t.size(), "the predefined zstd decoding tables");
    if (r != RC_OK) return r;
    HIP_TRY(hipMemcpy(d, t.data(), t.size(), hipMemcpyHostToDevice));
    u.zd_predef = d;
    return RC_OK;
}
}  // namespace
