// Host section of ssamd_api.hip (first): last error, options, scratch, profiler, the per-device context and lock, the host-buffer route.
namespace {
thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#include "ssamd_options.h"
#include "asw_plan.h"
#include "gsw_plan.h"
#include "ftp_plan.h"
#include "np_unwrap_plan.h"

// Experiment / test hooks (declared in ssamd_options.h).  The SSAMD_* environment variables are read ONCE, when
// the library is loaded; afterwards the table only changes through ssamd_set_option (tests, tools).  The host path of an operator
// call never calls getenv: it reads a thread-local snapshot that is refreshed when the table's version moves.
std::mutex g_tune_mutex;
std::atomic<unsigned> g_tune_version{1};

std::map<std::string, std::string> g_tuning_env;      // what the process was started with: ssamd_set_option(name, NULL) goes back to THIS
Tuning tuning_from_env()
{
    Tuning t;
    for (const char *n : kTuningNames)
        if (const char *v = getenv(n)) {      // the only getenv calls of the library
            g_tuning_env[n] = v;
            (void)tuning_assign(t, n, v);
        }
    return t;
}
Tuning g_tuning = tuning_from_env();

const Tuning &tune()
{
    thread_local Tuning snap;
    thread_local unsigned seen = 0;
    const unsigned v = g_tune_version.load(std::memory_order_acquire);
    if (v != seen) {
        std::lock_guard<std::mutex> lk(g_tune_mutex);
        snap = g_tuning;
        seen = v;
    }
    return snap;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SSAMD_ENOMEM : SSAMD_EHIP, "%s failed: %s",    \
                        #expr, hipGetErrorString(e_));                                             \
    } while (0)

// ------------------------------------------------------------------ scratch
struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SSAMD_OK;
        if (ptr) { (void)hipFree(ptr); ptr = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&ptr, want);
        if (e != hipSuccess) {
            ptr = nullptr;
            (void)hipGetLastError();      // ROCm 7 keeps the failure as the thread's last error: a caller that falls back must not see it again
            return fail(SSAMD_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return SSAMD_OK;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
    }
};

struct Profile {
    bool on = false;
    struct Pair { hipEvent_t a, b; int slot; };
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    double ms[SSAMD_K_COUNT] = {0};
    long long n[SSAMD_K_COUNT] = {0};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void drain()
    {
        for (auto &p : pending) {
            float t = 0.f;
            if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
                ms[p.slot] += t;
                n[p.slot] += 1;
            }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
};

// Small parameter-keyed device tables (ASW proximity weights per (winSize, gammaP), GSW weight table per gamma):
// a matcher that alternates between parameter sets finds its table again instead of re-uploading it behind a
// stream synchronisation.  An entry owns its host copy, so the upload is an ordinary asynchronous copy on the
// calling stream; later calls on other streams are ordered behind it by ScratchOrder.
struct TableEntry {
    int k0 = 0; double k1 = 0;
    DevBuf dev;
    std::vector<unsigned char> host;     // the bytes of the table on the host (floats or doubles, get_table)
};
struct TableCache {
    std::list<TableEntry> entries;       // most recently used first
    size_t max_entries;
    explicit TableCache(size_t n) : max_entries(n) {}
    TableEntry *find(int k0, double k1)
    {
        for (auto it = entries.begin(); it != entries.end(); ++it)
            if (it->k0 == k0 && it->k1 == k1) {
                entries.splice(entries.begin(), entries, it);
                return &entries.front();
            }
        return nullptr;
    }
};

struct Ctx {
    std::mutex mu;                      // serialises the calls on this device
    int dev = -1;
    int cus = 256;                      // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    bool lut_ready = false;
    hipStream_t stream = nullptr;       // used by the host-buffer entry points
    DevBuf imgL, imgR, recL, recR, keyL, keyR, disp, costs, lab, altq, evol, altdisp;
    DevBuf xlabL, xlabR, xflags, xqueue, xcost, xslots, xctr, xraw, xwtab;      // fp64 tie-break pass (asw_exact_kernels.hip.h)
    DevBuf pq;                          // ticket counters of the persistent phase-shifted launch (asw_launch_pipe), zeroed before each one
    DevBuf uwIn, uwOut;                 // host-buffer phase unwrapping (unwrap_kernels.hip.h)
    DevBuf ftpBand, ftpPhase;           // FTP phase (ftp_kernels.hip.h): kept bins per row; the wrapped map on its way to the unwrapper
    std::map<int, DevBuf> ftpTabs;      // twiddle table e^{2 pi i j / w} per width, built on the device
    DevBuf ftpRefTab;                   // FTP reference image (ftp_reference_kernels.hip.h): the bicubic weight table, uploaded once
    bool ftpRefTabReady = false;
    int32_t *ftpBandHost = nullptr;     // pinned staging of the bands: the asynchronous upload reads it after the call returned
    size_t ftpBandHostCap = 0;          // ... in int32 pairs
    hipEvent_t ftp_band_copied = nullptr;   // recorded behind that upload; the next call waits for it before it refills the staging
    AswExactQueue xq[2] = {};           // the final and the raw queue (entries == nullptr: none) of the last exact call
    TableCache proxTabs{8}, gswTabs{4}, proxTabs64{8};
    std::map<const void *, int> max_dyn_lds;   // hipFuncAttributeMaxDynamicSharedMemorySize already granted per kernel
    hipEvent_t scratch_free = nullptr;  // recorded after the last kernel that uses the scratch buffers
    int evol_small_calls = 0;           // consecutive calls that needed less than a quarter of the TAD volume's capacity
    long long evol_fallbacks = 0;       // calls that ran without the volume (in-kernel e tiles) or off the wave kernel for lack of memory
    long long tail_splits = 0;          // phase-shifted launches whose last partial round of workgroups ran as half-width tiles
    long long exact_calls = 0;          // ASW calls that ran the fp64 tie-break pass
    long long persist_launches = 0;     // phase-shifted launches in the persistent form
    long long gsw_plain_calls = 0;      // GSW calls that ran gsw_plain_kernel instead of the tiled kernel (host_gsw.h)
    Profile prof;
};

Ctx g_ctx[16];

// The calling thread's current HIP device is restored when an entry point returns: an operator asked to run on
// device k must not leave the caller's later allocations or launches on device k.
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() { if (hipGetDevice(&saved) != hipSuccess) saved = -1; }
    ~DeviceGuard() { if (saved >= 0) (void)hipSetDevice(saved); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

struct Timed {   // brackets one kernel launch with events when profiling is on
    Ctx &c; hipStream_t s; int slot; hipEvent_t a = nullptr, b = nullptr;
    Timed(Ctx &c_, hipStream_t s_, int slot_) : c(c_), s(s_), slot(slot_)
    {
        if (c.prof.on) { a = c.prof.get(); b = c.prof.get(); (void)hipEventRecord(a, s); }
    }
    ~Timed()
    {
        if (a) { (void)hipEventRecord(b, s); c.prof.pending.push_back({a, b, slot}); }
    }
};

// A locked device context: makes `device` (-1: the calling thread's current one) current for the duration of the
// entry point, takes that device's mutex and restores the caller's device afterwards.
struct CtxLock {
    DeviceGuard guard;                   // destroyed last: restores the caller's device after the unlock
    std::unique_lock<std::mutex> lk;
    Ctx *c = nullptr;
    Ctx *operator->() { return c; }
    Ctx &operator*() { return *c; }
};

int get_ctx(int device, CtxLock &out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SSAMD_ENODEVICE, "no HIP device visible: libssamd has no CPU fallback");
    if (device < 0) device = out.guard.saved >= 0 ? out.guard.saved : 0;
    if (device >= n || device >= 16) return fail(SSAMD_EINVAL, "device ordinal %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    Ctx &c = g_ctx[device];
    out.lk = std::unique_lock<std::mutex>(c.mu);
    out.c = &c;
    if (c.dev < 0) {
        c.dev = device;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c.cus = cus;
        else (void)hipGetLastError();
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c.scratch_free, hipEventDisableTiming));
    }
    if (!c.lut_ready) {
        // sRGB byte -> linear*100 in the reference's float arithmetic (colorconversion.hpp:19-37); powf = glibc's algorithm restated
        // (glibc_math.hip.h, host side), NOT the host's libm: the same 256 floats on any host (oracle/libm_check.c proves them equal
        // to glibc's, tests/test_gpu_libm_independence.py runs the path with the process's exp / powf replaced by garbage)
        float lut[256];
        for (int v = 0; v < 256; ++v) {
            float x = v / 255.0;
            if (x > 0.04045) x = glibc_powf_pos((float)((x + 0.055) / 1.055), (float)2.4);
            else x /= 12.92;
            x *= 100;
            lut[v] = x;
        }
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_lin100), lut, sizeof(lut)));
        c.lut_ready = true;
    }
    return SSAMD_OK;
}

// hipFuncSetAttribute costs a runtime round trip: ask only when a launch needs more dynamic LDS than the kernel
// has been granted on this device so far
int grant_dyn_lds(Ctx &c, const void *kernel, int bytes)
{
    int &granted = c.max_dyn_lds[kernel];
    if (bytes <= granted || bytes <= 48 * 1024) return SSAMD_OK;     // 48 KiB need no opt-in
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    granted = bytes;
    return SSAMD_OK;
}

// The scratch buffers (pixel records, WTA keys, tables) are shared by every call on a device.  Calls are
// serialised on the host by the device's mutex; across streams the next call's stream waits for the previous call's
// last kernel, so callers may use any stream without synchronising between operators.
struct ScratchOrder {
    Ctx &c; hipStream_t s;
    ScratchOrder(Ctx &c_, hipStream_t s_) : c(c_), s(s_) { (void)hipStreamWaitEvent(s, c.scratch_free, 0); }
    ~ScratchOrder() { (void)hipEventRecord(c.scratch_free, s); }
};

int check_common(int H, int W, int win, int minD, int maxD, int row0, int rows)
{
    if (H <= 0 || W <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (!(win > 0 && win % 2 == 1)) return fail(SSAMD_EINVAL, "winSize must be a positive odd number!");
    if (minD < 0) return fail(SSAMD_EINVAL, "minDisparity must be >= 0 (negative values are undefined behaviour in the reference)");
    if (W > 32767 || maxD > 32767) return fail(SSAMD_ELIMIT, "width / maxDisparity exceed the int16 disparity range");
    if (row0 < 0 || rows < 0 || row0 + rows > H) return fail(SSAMD_EINVAL, "output row range [%d,%d) outside the image (height %d)", row0, row0 + rows, H);
    if (win > 255) return fail(SSAMD_ELIMIT, "winSize %d > 255 not supported", win);
    if (rows > 65535) return fail(SSAMD_ELIMIT, "more than 65535 output rows per call: split the image into row strips");
    return SSAMD_OK;
}

// ------------------------------------------------------------ parameter-keyed device tables
// One routine behind the three tables: find, or evict the least recently used entry, fill the host copy (fill(T *)), upload.
template <class T, class Fill>
int get_table(TableCache &tc, int k0, double k1, size_t n, const char *what, hipStream_t s, const T **out, Fill fill)
{
    if (TableEntry *e = tc.find(k0, k1)) { *out = (const T *)e->dev.ptr; return SSAMD_OK; }
    if (tc.entries.size() >= tc.max_entries) {
        // evicting frees device memory a launch in flight may still read: the one place that waits (rare: more
        // than eight parameter sets alternating on one device)
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(tc.entries.back().dev.ptr);
        tc.entries.pop_back();
    }
    tc.entries.emplace_front();
    TableEntry &e = tc.entries.front();
    e.k0 = k0; e.k1 = k1;
    e.host.resize(n * sizeof(T));
    fill(reinterpret_cast<T *>(e.host.data()));
    int rc = e.dev.reserve(n * sizeof(T));
    if (rc) { tc.entries.pop_front(); return rc; }
    hipError_t he = hipMemcpyAsync(e.dev.ptr, e.host.data(), n * sizeof(T), hipMemcpyHostToDevice, s);
    if (he != hipSuccess) {
        (void)hipFree(e.dev.ptr);
        tc.entries.pop_front();
        return fail(SSAMD_EHIP, "hipMemcpyAsync(%s) failed: %s", what, hipGetErrorString(he));
    }
    *out = (const T *)e.dev.ptr;
    return SSAMD_OK;
}

// ------------------------------------------------------------ host buffers: the one route through the context's staging buffers
// A host buffer of an entry point and the scratch buffer of the context it is staged in, `at` bytes into it.
struct HostIn { DevBuf Ctx::*buf; const void *host; size_t bytes; size_t at = 0; };
struct HostOut { DevBuf Ctx::*buf; void *host; size_t bytes; size_t at = 0; };
inline char *staged(Ctx &c, DevBuf Ctx::*buf, size_t at = 0) { return (char *)(c.*buf).ptr + at; }

// Lock the context of `device`, reserve the staging buffers (inputs first), order the scratch on the context's stream, copy the
// inputs up, launch(Ctx &, hipStream_t) -- which finds its device pointers with staged() --, copy the output down, wait.
template <class Launch>
int host_route(int device, std::initializer_list<HostIn> in, const HostOut &out, Launch launch)
{
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    for (const HostIn &i : in)
        if ((rc = ((*c).*i.buf).reserve(i.at + i.bytes))) return rc;
    if ((rc = ((*c).*out.buf).reserve(out.at + out.bytes))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    for (const HostIn &i : in) HIP_TRY(hipMemcpyAsync(staged(*c, i.buf, i.at), i.host, i.bytes, hipMemcpyHostToDevice, s));
    if ((rc = launch(*c, s))) return rc;
    HIP_TRY(hipMemcpyAsync(out.host, staged(*c, out.buf, out.at), out.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}
}  // namespace
