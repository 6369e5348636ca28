// libssamd.so: host side of the C ABI declared in include/ssamd.h (gfx950 / ROCm).
// Owns device scratch, chooses launch geometry, launches the HIP kernels.
// There is deliberately no CPU code path for the operators in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <list>
#include <map>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ssamd.h"
#include "asw_shared.hip.h"
#include "asw_kernels.hip.h"
#include "asw_pipe_kernel.hip.h"
#include "asw_wave_kernel.hip.h"
#include "asw_wave6_kernel.hip.h"
#include "asw_alt_kernels.hip.h"
#include "asw_prepass_kernels.hip.h"
#include "asw_finalize_kernels.hip.h"
// the phase-shifted and the six-per-lane kernels are instantiated in translation units of their own (asw_pipe_tu.hip, asw_wave6_tu.hip)
namespace ssamd {
#define SSAMD_PIPE_INSTANCE(C, SL, SR, SE) extern template __global__ void asw_aggregate_pipe_kernel<C, SL, SR, SE>(const AswArgs);
#define SSAMD_WAVE6_INSTANCE(C, K, CREG) extern template __global__ void asw_aggregate_wave6_kernel<C, K, CREG>(const AswWaveArgs);
#include "asw_instances.inc"
#undef SSAMD_PIPE_INSTANCE
#undef SSAMD_WAVE6_INSTANCE
}  // namespace ssamd
#include "gsw_kernels.hip.h"
#include "lab_kernels.hip.h"
#include "asw_exact_kernels.hip.h"
#include "rig_kernels.hip.h"
#include "unwrap_kernels.hip.h"
#include "np_unwrap_kernels.hip.h"
#include "ftp_kernels.hip.h"
#include "ftp_cloud_kernels.hip.h"

using namespace ssamd;

namespace {

thread_local std::string g_err;
// Locking: every device has its own context and its own mutex (Ctx::mu), so one process can drive several GPUs
// concurrently through the operators (ssamd_*_multi does, one host thread per device).  g_geom_mutex guards the
// small process-wide launch-geometry caches only and is never held across a HIP call.
std::mutex g_geom_mutex;

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
    int32_t *ftpBandHost = nullptr;     // pinned staging of the bands: the asynchronous upload reads it after the call returned
    size_t ftpBandHostCap = 0;          // ... in int32 pairs
    hipEvent_t ftp_band_copied = nullptr;   // recorded behind that upload; the next call waits for it before it refills the staging
    unsigned int xcap = 0, xrawcap = 0; // queue capacities of the last exact call
    TableCache proxTabs{8}, gswTabs{4}, proxTabs64{8};
    std::map<const void *, int> max_dyn_lds;   // hipFuncAttributeMaxDynamicSharedMemorySize already granted per kernel
    hipEvent_t scratch_free = nullptr;  // recorded after the last kernel that uses the scratch buffers
    int evol_small_calls = 0;           // consecutive calls that needed less than a quarter of the TAD volume's capacity
    long long evol_fallbacks = 0;       // calls that ran without the volume (in-kernel e tiles) or off the wave kernel for lack of memory
    long long tail_splits = 0;          // phase-shifted launches whose last partial round of workgroups ran as half-width tiles
    long long exact_calls = 0;          // ASW calls that ran the fp64 tie-break pass
    long long persist_launches = 0;     // phase-shifted launches in the persistent form
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

// hipFuncSetAttribute costs a runtime round trip: ask only when a launch needs more dynamic LDS than the kernel
// has been granted on this device so far
int grant_dyn_lds(Ctx &c, const void *kernel, int bytes);

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

// ------------------------------------------------------------ launch geometry: caches around the planners (asw_plan.h, gsw_plan.h)
// The planners are functions of their arguments and know no error codes: their verdicts become the operators' errors here.
int asw_search(AswGeom &best, const PlanOptions &po, int W, int rows, int win, int nD, std::vector<AswGeom> *shortlist = nullptr)
{
    const PlanResult r = asw_search_geometry(best, po, W, rows, win, nD, shortlist);
    if (r == PLAN_FORCED_UNUSABLE) return fail(SSAMD_ELIMIT, "SSAMD_ASW_GEOM does not fit LDS");
    return r == PLAN_OK ? SSAMD_OK : fail(SSAMD_ELIMIT, "no ASW launch geometry fits LDS for winSize=%d nD=%d", win, nD);
}

int gsw_search(GswGeom &best, const std::string &forced, int W, int rows, int win, int nD)
{
    const PlanResult r = gsw_search_geometry(best, forced, W, rows, win, nD);
    if (r == PLAN_FORCED_UNUSABLE) return fail(SSAMD_EINVAL, "SSAMD_GSW_GEOM=%s is not a usable geometry", forced.c_str());
    return r == PLAN_OK ? SSAMD_OK : fail(SSAMD_ELIMIT, "no GSW launch geometry fits LDS for winSize=%d nD=%d", win, nD);
}

// The search walks a few thousand candidate tiles (0.1-0.3 ms on the host): remember the answer per problem shape,
// a video stream asks the same question every frame.  (All four maps are guarded by g_geom_mutex.)
using ShapeKey = std::array<int, 4>;      // W, workgroup rows, winSize, nD
template <class Geom> struct GeomCache {
    std::map<ShapeKey, Geom> geom;
    std::map<ShapeKey, bool> tuned;       // shapes whose cached geometry was picked by measurement
};
GeomCache<AswGeom> g_asw_geom;
GeomCache<GswGeom> g_gsw_geom;
// autotuning mode: 1 always, 0 never, -1 (default) only for small problems, where the ~50 trial launches cost
// at most about 0.4 s once and where the cost model is least reliable
std::atomic<int> g_autotune{g_tuning.autotune_env != -2 ? g_tuning.autotune_env : -1};
constexpr double ASW_AUTOTUNE_SMALL_TAPS = 6.0e10;      // window taps per call (about 6-8 ms of kernel time; 3e10 until round 4)

// forced (tuning hooks: asw_geometry_forced, SSAMD_GSW_GEOM): never cached
template <class Geom, class Search>
int choose_geometry(GeomCache<Geom> &cache, bool forced, const ShapeKey &key, Geom &best, Search search)
{
    if (forced) return search(best);
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    auto it = cache.geom.find(key);
    if (it != cache.geom.end()) { best = it->second; return SSAMD_OK; }
    const int rc = search(best);
    if (rc == SSAMD_OK) {
        if (cache.geom.size() > 256) { cache.geom.clear(); cache.tuned.clear(); }
        cache.geom[key] = best;
    }
    return rc;
}

int asw_choose_geometry(AswGeom &best, const PlanOptions &po, int W, int rows, int win, int nD)
{
    return choose_geometry(g_asw_geom, asw_geometry_forced(po.t), {W, rows, win, nD}, best,
                           [&](AswGeom &g) { return asw_search(g, po, W, rows, win, nD); });
}

int gsw_choose_geometry(GswGeom &best, const Tuning &t, int W, int rows, int win, int nD)
{
    return choose_geometry(g_gsw_geom, !t.gsw_geom.empty(), {W, rows, win, nD}, best,
                           [&](GswGeom &g) { return gsw_search(g, t.gsw_geom, W, rows, win, nD); });
}

// Autotuning (ssamd_autotune): is this call the one that times the candidates of its shape?
template <class Geom> bool autotune_due(GeomCache<Geom> &cache, const ShapeKey &shape, double call_taps)
{
    const int mode = g_autotune.load();
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    return (mode > 0 || (mode < 0 && call_taps <= ASW_AUTOTUNE_SMALL_TAPS)) && cache.tuned.count(shape) == 0;
}
// ... the trial launches: round-robin over the n candidates, `rounds` rounds, fastest launch of each (round 0 is warm-up) -- clocks
// ramp up during the first launches after an idle period, so timing the candidates one after the other would favour the late ones.
// run(ci) prepares and launches candidate ci; anything that fails costs it the round (and clears *ok, when asked).
// prune: a candidate that is twice as slow as the best one in the warm-up round (very narrow tiles can be several times slower than
// the model's choice) is not timed again: bounds what the first call of a shape costs.
// The verdict: the model's own choice (first) keeps the job unless another candidate is clearly faster.  -1: none was timed
template <class Run> int autotune_rounds(size_t n, int rounds, bool prune, hipEvent_t e0, hipEvent_t e1, hipStream_t s, bool *ok, Run run)
{
    std::vector<float> cand_ms(n, 3.0e38f), warm_ms(n, 3.0e38f);
    std::vector<char> alive(n, 1);
    for (int round = 0; round < rounds; ++round) {
        for (size_t ci = 0; ci < n; ++ci) {
            if (!alive[ci]) continue;
            float ms = 3.0e38f;
            if (hipEventRecord(e0, s) == hipSuccess && run(ci) && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess)
                (void)hipEventElapsedTime(&ms, e0, e1);
            else if (ok)
                *ok = false;
            if (round > 0) cand_ms[ci] = std::min(cand_ms[ci], ms);
            else warm_ms[ci] = ms;
        }
        if (round == 0 && prune) {
            const float wbest = *std::min_element(warm_ms.begin(), warm_ms.end());
            for (size_t ci = 1; ci < n; ++ci) alive[ci] = warm_ms[ci] <= 2.0f * wbest;
        }
    }
    int fastest = -1;
    float best_ms = 3.0e38f;
    for (size_t ci = 0; ci < n; ++ci)
        if (cand_ms[ci] < best_ms * (ci == 0 ? 1.0f : 0.985f)) { best_ms = cand_ms[ci]; fastest = (int)ci; }
    return fastest;
}
template <class Geom> void autotune_keep(GeomCache<Geom> &cache, const ShapeKey &shape, const Geom &fastest)
{
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    cache.geom[shape] = fastest;
    cache.tuned[shape] = true;
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

// Proximity weights exp(-|t|/gammaP) of the window taps (_passive.cpp:360-364), cached per (winSize, gammaP).
int get_prox(Ctx &c, int win, double gammaP, hipStream_t s, const float **out)
{
    return get_table(c.proxTabs, win, gammaP, (size_t)win * win, "proximity table", s, out, [&](float *host) {
        const int p = win / 2;
        for (int i = 0; i < win; ++i)
            for (int j = 0; j < win; ++j) {
                const double di = i - p, dj = j - p;
                host[(size_t)i * win + j] = (float)glibc_exp(-std::sqrt(di * di + dj * dj) / gammaP);      // (restated exp: see get_prox64)
            }
    });
}

// The same table in fp64 for the tie-break pass -- the reference's expression (_passive.cpp:360-364:
// exp(-sqrt(pow(i-padding,2) + pow(j-padding,2))/gammaP)) with glibc's exp restated on the host side (round 6: rounds 1-5 called the
// host's libm here, which made the exact mode's bit-identity a property of the host).
int get_prox64(Ctx &c, int win, double gammaP, hipStream_t s, const double **out)
{
    return get_table(c.proxTabs64, win, gammaP, (size_t)win * win, "fp64 proximity table", s, out, [&](double *host) {
        const int p = win / 2;
        for (int i = 0; i < win; ++i)
            for (int j = 0; j < win; ++j)
            {
                // exp: glibc's algorithm restated (glibc_math.hip.h), not the host's libm -- bit-identical to glibc's on every argument
                // oracle/libm_check.c tries, and the same on a host that runs another libm.  pow(int, 2) is exact, sqrt and the
                // division are IEEE operations (one correctly rounded result on any conforming host)
                const double di = i - p, dj = j - p;
                host[(size_t)i * win + j] = glibc_exp(-std::sqrt(di * di + dj * dj) / gammaP);
            }
    });
}

// support weight as a function of the integer squared colour distance, in the reference's
// arithmetic: fl32 distance (sqrt in double), float division by gamma, float exp (_passive.cpp:457-463, 495)
int get_gsw_table(Ctx &c, int gamma, hipStream_t s, const float **out)
{
    return get_table(c.gswTabs, gamma, 0.0, (size_t)GSW_TAB_SIZE, "GSW weight table", s, out, [&](float *host) {
        for (int v = 0; v < GSW_TAB_SIZE; ++v) {
            const float dist = (float)(0.0f + std::sqrt((double)v));
            host[v] = expf(-dist / gamma);
        }
    });
}

// WTA keys of a call start as all ones: any (cost, disparity) key is smaller
int reset_keys(DevBuf &keys, size_t nout, hipStream_t s)
{
    if (int rc = keys.reserve(nout * 8)) return rc;
    HIP_TRY(hipMemsetAsync(keys.ptr, 0xFF, nout * 8, s));
    return SSAMD_OK;
}

// fp64 tie-break pass (asw_exact_kernels.hip.h), part 1 -- BEFORE the aggregation: queue, pixel flags and counters of this call;
// fills the AswExactQueue the aggregation kernels append their near-ties to (round 6: no cost-image volume).
int asw_exact_prepare(Ctx &c, int W, int rows, int win, int nD, double gammaC, bool consistent, bool direct, hipStream_t s,
                      AswExactQueue &q, AswExactQueue &raw, AswExactQueue &kernel_q)
{
    const size_t nout = (size_t)rows * W;
    if (nout >= ((size_t)1 << 32)) return fail(SSAMD_ELIMIT, "exact mode: more than 2^32 output pixels per call");
    // queue: room for a few candidates of every pixel, bounded (a frame of saturated noise can flag every candidate of every
    // pixel; an overflow leaves the fp32 map and is reported: `exact_overflow`); frames of up to 4M candidates in all get room
    // for every one of them on both sides -- a flat test image cannot overflow
    // (a candidate can be queued once per side -- by a select and by a merge, or by the left and the right escalation)
    const size_t all_cands = 2 * (nout * (size_t)nD + nout);
    size_t cap = std::min<size_t>(std::max<size_t>(4 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (tune().exact_cap) cap = (size_t)tune().exact_cap;
    // raw queue of merging calls (12 B per entry): what workgroups select against their tile-local winners
    size_t rawcap = direct ? 0 : std::min<size_t>(std::max<size_t>(2 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (!direct && tune().exact_cap) rawcap = std::max<size_t>(rawcap, cap);
    if (!direct && tune().exact_rawcap) rawcap = (size_t)tune().exact_rawcap;
    int rc;
    // [64 B counters][flagL][flagR][zeroL][zeroR] (nout bytes each) [zrow rows]: one buffer, one memset
    if ((rc = c.xqueue.reserve(cap * 8)) || (rc = c.xcost.reserve(cap * 8)) || (rc = c.xflags.reserve(64 + 4 * nout + (size_t)rows)) ||
        (rc = c.xslots.reserve(nout * 32)) || (rawcap && (rc = c.xraw.reserve(rawcap * 12))))
        return rc;
    c.xcap = (unsigned int)cap;
    c.xrawcap = (unsigned int)rawcap;
    HIP_TRY(hipMemsetAsync(c.xflags.ptr, 0, 64 + 4 * nout + (size_t)rows, s));
    q.entries = (u64 *)c.xqueue.ptr;
    q.ekeys = nullptr;
    q.counter = (unsigned int *)c.xflags.ptr;
    q.flagL = (unsigned char *)c.xflags.ptr + 64;
    q.flagR = consistent ? q.flagL + nout : nullptr;
    q.zeroL = q.flagL + 2 * nout;
    q.zeroR = consistent ? q.flagL + 3 * nout : nullptr;
    q.zrow = q.flagL + 4 * nout;
    q.W = (unsigned int)W;
    q.cap = (unsigned int)cap;
    // Near-tie band.  128 ulps = 1.5e-5 relative at gammaC = 5 and a 35 x 35 window: the kernels' support weights inherit the
    // rounding of the Lab records to float (|dLab| <= ~1.3e-5 per colour distance), i.e. a relative error of ~2.6e-5 / gammaC on a
    // weight product -- scaled up for smaller gammaC; and the (N, S') sums are fp32 sums of win^2 products whose rounding errors
    // add up like a random walk (~win ulps): scaled up with the window beyond 35 (a fixed band ignored the tap
    // count; tests/test_gpu_exact.py::test_large_windows_against_the_oracle)
    q.tol = (uint32_t)std::min(1.0e6, (double)tune().exact_tol * std::max(1.0, 5.0 / gammaC) * std::max(1.0, win / 35.0));
    // rounding noise of the reference's fp64 quotient sum(w e) / sum(w) over n = win^2 taps: <= ~(n + 3) u relative on numerator and
    // denominator each, u = 2^-53, i.e. 2 (n + 3) u 40 absolute near the cap; two candidates can swap places when they are
    // closer than twice that (x 1.5 margin)
    q.sat_abs = (float)(1.5 * 2.0 * 2.0 * ((double)win * win + 3.0) * 1.1102230246251565e-16 * 40.0);
    q.deep = 0xffffffffu;
    raw = AswExactQueue{};
    if (!direct) {
        raw = q;
        union { float f; uint32_t u; } sa; sa.f = q.sat_abs;
        raw.deep = 0xC0000000u - sa.u;                                   // images with 40 - cost <= sat_abs stay out of the raw queue
        raw.entries = (u64 *)c.xraw.ptr;
        raw.ekeys = (uint32_t *)((u64 *)c.xraw.ptr + rawcap);
        raw.counter = q.counter + 4;
        raw.flagL = raw.flagR = nullptr;
        raw.cap = (unsigned int)rawcap;
    }
    kernel_q = direct ? q : raw;
    return SSAMD_OK;
}

// ... part 2 -- AFTER the aggregation: the queue holds the near-ties of every winner, c.keyL / c.keyR (or the map itself when the
// aggregation wrote it: `direct`) the fp32 winners.  Rewrites the winners of pixels whose near-ties fp64 decides differently.
int asw_exact_pass(Ctx &c, const AswExactQueue &q, const AswExactQueue &raw, int H, int W, int row0, int rows, int win, int maxD, int minD, double gammaC, double gammaP,
                   bool consistent, bool direct, int16_t *d_disp, hipStream_t s)
{
    const int p = win / 2;
    const size_t nout = (size_t)rows * W, npix = (size_t)H * W;
    int rc;
    const double *d_prox = nullptr;
    if ((rc = get_prox64(c, win, gammaP, s, &d_prox))) return rc;
    if ((rc = c.xlabL.reserve(npix * 24)) || (rc = c.xlabR.reserve(npix * 24))) return rc;
    AswExactArgs x;
    x.recL = (const PixRec *)c.recL.ptr; x.recR = (const PixRec *)c.recR.ptr;
    x.labL = (const double *)c.xlabL.ptr; x.labR = (const double *)c.xlabR.ptr;
    x.prox = d_prox;
    x.keyL = direct ? nullptr : (u64 *)c.keyL.ptr; x.keyR = consistent ? (u64 *)c.keyR.ptr : nullptr;
    x.disp = d_disp;
    x.q = q;
    x.raw = raw;
    x.ecost = (double *)c.xcost.ptr;
    x.costL = (u64 *)c.xslots.ptr; x.costR = x.costL + nout;
    x.idxL = (uint32_t *)(x.costR + nout); x.idxR = x.idxL + nout;
    x.wslotL = x.idxR + nout; x.wslotR = x.wslotL + nout;
    // weight tables of flagged pixels: up to 64 MB of them (6 800 pixels at a 35 x 35 window; the bench frame flags 133, the 4K frame 3 044)
    {
        const size_t per = (size_t)win * win * 8;
        size_t wcap = std::min<size_t>(65536, ((size_t)64 << 20) / per);
        if (nout >= ((size_t)1 << 31)) wcap = 0;
        if (wcap && (rc = c.xwtab.reserve(wcap * 8 + wcap * per))) return rc;
        x.wcap = (unsigned int)wcap;
        x.wpix = (uint32_t *)c.xwtab.ptr;
        x.wtab = (double *)((char *)c.xwtab.ptr + wcap * 8);
    }
    x.H = H; x.W = W; x.win = win; x.pad = p; x.minD = minD; x.maxD = maxD; x.row0 = row0; x.rows = rows;
    x.gammaC = gammaC;
    Timed t(c, s, SSAMD_K_ASW_EXACT);
    {
        const int r0 = std::max(0, row0 - p), r1 = std::min(H, row0 + rows + p);
        const long long np2 = (long long)(r1 - r0) * W;
        const int blocks = (int)std::min<long long>((2 * np2 + 255) / 256, 256 * 8);
        hipLaunchKernelGGL(bgr2lab_f64_pair_kernel, dim3(blocks), dim3(256), 0, s, x.recL + (size_t)r0 * W, x.recR + (size_t)r0 * W,
                           (double *)c.xlabL.ptr + 3 * (size_t)r0 * W, (double *)c.xlabR.ptr + 3 * (size_t)r0 * W, np2);
    }
    const int pb = (int)std::min<long long>(((long long)nout + 255) / 256, 256 * 8);
    if (raw.entries) {
        hipLaunchKernelGGL(asw_exact_filter_kernel, dim3(256 * 8), dim3(256), 0, s, x);
        hipLaunchKernelGGL(asw_exact_escalate_kernel, dim3(pb), dim3(256), 0, s, x);
    }
    {
        const int zwin = std::min(win, EXACT_ZWIN_MAX - 1);
        const size_t zlds = (size_t)2 * zwin * (EXACT_ZSEG + 2 * (zwin / 2)) * 4;                      // two window-row tiles (<= 63 x 126 x 4 B x 2)
        if ((rc = grant_dyn_lds(c, (const void *)asw_exact_zero_kernel, (int)zlds))) return rc;
        const long long segs = (long long)rows * ((W + EXACT_ZSEG - 1) / EXACT_ZSEG);
        hipLaunchKernelGGL(asw_exact_zero_kernel, dim3((unsigned)std::min<long long>(segs, 256 * 64)), dim3(256), zlds, s, x);
    }
    hipLaunchKernelGGL(asw_exact_winners_kernel, dim3(pb), dim3(256), 0, s, x);
    if (x.wcap) hipLaunchKernelGGL(asw_exact_wtab_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_eval_kernel, dim3((unsigned)(c.cus * 5)), dim3(64 * EXACT_WAVES), 0, s, x);      // five 4-wave groups per CU are resident (91 VGPRs)
    hipLaunchKernelGGL(asw_exact_resolve_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_patch_kernel, dim3(pb), dim3(256), 0, s, x);
    HIP_TRY(hipGetLastError());
    ++c.exact_calls;
    return SSAMD_OK;
}

// Decode / left-right check of rows [b0, b0 + nb) of a call's key buffers into the same rows of d_disp (row-local:
// _passive.cpp:251-285).  d_raw_right: verification dump, both raw argmins instead of the left-right check and filling.
int launch_finalize(Ctx &c, int slot, bool lrcheck, int b0, int nb, int W, int16_t *d_disp, hipStream_t s,
                    int16_t *d_raw_right = nullptr)
{
    if (nb <= 0) return SSAMD_OK;
    const size_t off = (size_t)b0 * W;
    const long long n = (long long)nb * W;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 256 * 8);
    Timed t(c, s, slot);
    if (d_raw_right) {
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyL.ptr + off, d_disp + off, nb, W, 0);
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyR.ptr + off, d_raw_right + off, nb, W, 1);
    } else if (lrcheck) {
        const size_t lds = (((size_t)W * 2 + 15) & ~(size_t)15) + W;      // up to 96 KiB at the 32767-column limit
        int rc = grant_dyn_lds(c, (const void *)lr_check_fill_kernel, (int)lds);
        if (rc) return rc;
        hipLaunchKernelGGL(lr_check_fill_kernel, dim3(nb), dim3(256), lds, s, (const u64 *)c.keyL.ptr + off,
                           (const u64 *)c.keyR.ptr + off, d_disp + off, nb, W);
    } else {
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyL.ptr + off, d_disp + off, nb, W, 0);
    }
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// ------------------------------------------------------------ ASW: kernel variants, picked from tables generated from asw_instances.inc
// (the list of what the other two translation units compile): what is selected here and what is compiled there cannot disagree
using AswKernel = void (*)(const AswArgs);
using AswWaveKernel = void (*)(const AswWaveArgs);
struct AswPipeVariant { bool costs; int SL, SR, Se; AswKernel kernel; };
const AswPipeVariant kPipeVariants[] = {
#define SSAMD_PIPE_INSTANCE(C, SL, SR, SE) {C, SL, SR, SE, asw_aggregate_pipe_kernel<C, SL, SR, SE>},
#include "asw_instances.inc"
#undef SSAMD_PIPE_INSTANCE
};
// Wave kernels: RD disparities per lane (6: asw_instances.inc; 4: instantiated here), RX columns, and the build rounds known at
// compile time (straight-line build) for the common combinations; KM > 0: merged build of KM rounds, else KL + KR separate rounds
struct AswWaveVariant { int RD; bool costs; int RX, KL, KR, KM; bool creg; AswWaveKernel kernel; };
#define SSAMD_WAVE_VARIANT(RX, KL, KR, KM, CREG) {4, false, RX, KL, KR, KM, CREG, asw_aggregate_wave_kernel<false, RX, KL, KR, KM, CREG>}
const AswWaveVariant kWaveVariants[] = {
#define SSAMD_WAVE6_INSTANCE(C, K, CREG) {6, C, 4, 0, 0, K, CREG, asw_aggregate_wave6_kernel<C, K, CREG>},
#include "asw_instances.inc"
#undef SSAMD_WAVE6_INSTANCE
    SSAMD_WAVE_VARIANT(4, 0, 0, 2, false), SSAMD_WAVE_VARIANT(4, 0, 0, 2, true),      // class default D 0..16 four per lane: 48 + 67 centres
    SSAMD_WAVE_VARIANT(4, 0, 0, 3, false), SSAMD_WAVE_VARIANT(4, 0, 0, 3, true),
    SSAMD_WAVE_VARIANT(4, 0, 0, 4, false), SSAMD_WAVE_VARIANT(4, 0, 0, 4, true),
    SSAMD_WAVE_VARIANT(8, 0, 0, 2, false), SSAMD_WAVE_VARIANT(8, 0, 0, 3, false), SSAMD_WAVE_VARIANT(8, 0, 0, 4, false),
    SSAMD_WAVE_VARIANT(8, 2, 2, 0, false),      // 17..28 disparities (class default)
    SSAMD_WAVE_VARIANT(8, 1, 2, 0, false),      // 29..48
    SSAMD_WAVE_VARIANT(4, 1, 2, 0, false),      // 13..20
    SSAMD_WAVE_VARIANT(4, 2, 2, 0, false),      // 9..12
    SSAMD_WAVE_VARIANT(4, 2, 3, 0, false),      // 5..8
};
#undef SSAMD_WAVE_VARIANT

// Strides known at compile time for the tiles of the headline configurations (immediate offsets in the
// tap steps): 120 x 196 (1080p / D 0..192) and 88 x 260 (4096 x 2160 / D 0..256), 216 x 68 (D 0..64)
// (with the cost / cost-image dump too: exact=True on the headline tiles ran the run-time-stride form, + 0.9 ms at 1080p / 193)
AswKernel asw_pick_pipe_kernel(const AswGeom &g, bool costs, int asw_static)
{
    AswKernel pk = nullptr;
    for (const AswPipeVariant &v : kPipeVariants) {
        if (v.costs != costs) continue;
        if (v.SL == 0 && !pk) pk = v.kernel;                                  // (the generic instantiation, unless a static one matched)
        if (asw_static != 0 && v.SL == g.SL && v.SR == g.SR && v.Se == g.Se) pk = v.kernel;
    }
    return pk;
}

// A miss runs the generic instantiation of the family (no straight-line build, centres in LDS).
AswWaveKernel asw_pick_wave_kernel(const AswWaveGeom &g, bool costs, bool unrolled)
{
    const bool straight = unrolled && !costs;
    const int kl = g.merged ? 0 : (g.Txw + 63) / 64, kr = g.merged ? 0 : (g.nRcw + 63) / 64, km = g.merged ? g.K : 0;
    for (const AswWaveVariant &v : kWaveVariants)
        if (straight && v.RD == g.RD && !v.costs && v.RX == g.RX && v.KL == kl && v.KR == kr && v.KM == km && v.creg == (g.creg != 0)) return v.kernel;
    if (g.RD == 6) return costs ? asw_aggregate_wave6_kernel<true, 0> : asw_aggregate_wave6_kernel<false, 0>;
    return g.RX == 8 ? (costs ? asw_aggregate_wave_kernel<true, 8> : asw_aggregate_wave_kernel<false, 8>)
                     : (costs ? asw_aggregate_wave_kernel<true, 4> : asw_aggregate_wave_kernel<false, 4>);
}

// ------------------------------------------------------------ ASW: one call
// What an entry point asks for.  Images: dL / dR (rectified BGR bytes on the device), or rm: the RAW frames through the rig's maps
// (remap_lab_records_pair_kernel: rectification + Lab in one launch).
// skip > 0: rows [row0 + skip_at, row0 + skip_at + skip) of the range are NOT matched (ssamd_asw_device_rows2: the two border
// bands of a row strip in one launch); buffers stay laid out for the whole range [row0, row0 + rows)
struct AswCall {
    const uint8_t *dL = nullptr, *dR = nullptr;
    const RemapSrc *rm = nullptr;
    int H = 0, W = 0, row0 = 0, rows = 0, skip_at = 0, skip = 0;
    int win = 0, maxD = 0, minD = 0;
    double gammaC = 0, gammaP = 0;
    bool consistent = false, alternate = false, exact = false;
    int16_t *d_disp = nullptr;
    float *d_costs = nullptr;
    int16_t *d_raw_right = nullptr;
    hipStream_t s = nullptr;
};

struct AswRun : AswCall {
    Ctx &c;
    const Tuning &t;                  // (state of a call in flight: the call, the thread's option snapshot, what the steps hand on)
    PlanOptions po;
    int p, nD, grows, r0, r1, lab_blocks;
    size_t nout;
    long long np2;
    ShapeKey shape;           // W, workgroup rows, winSize, nD
    AswGeom geom;                     // the geometry of the (last) launch
    std::vector<AswGeom> trial;       // autotuning candidates, the model's choice first; empty: no trial launches
    bool need_keys = false, lab_pending = false;
    size_t evol_cap_max = 0, evol_limit = 0;      // (evol_limit 0: free memory not asked for yet)
    const float *d_prox = nullptr;
    const unsigned char *evol = nullptr;      // TAD volume of the geometry prepared last (nullptr: none)
    int evolW = 0;
    AswWaveGeom wave;                 // strip of the wave kernel, filled by asw_prepare_volume
    AswExactQueue xq_final{}, xq_raw{}, xq_kernel{};      // exact mode: the final near-tie queue, for merging calls the raw one, and the one the kernels append to
};

// One disparity chunk and no right-referenced pass: each pixel is decided by exactly one workgroup, which then
// writes the disparity itself -- no key buffer, atomics or decode kernel (34 instead of 48+ bytes of HBM per pixel).
bool asw_is_direct(const AswRun &r, const AswGeom &g) { return r.nD >= 1 && (g.nchunks == 1 || g.wave_rx) && !r.consistent; }

// 1: nothing to compute
int asw_check_call(const AswCall &q)
{
    int rc = check_common(q.H, q.W, q.win, q.minD, q.maxD, q.row0, q.rows);
    if (rc) return rc;
    if (q.skip < 0 || q.skip_at < 0 || q.skip_at + q.skip > q.rows) return fail(SSAMD_EINVAL, "bad row gap [%d,%d) in a range of %d rows", q.skip_at, q.skip_at + q.skip, q.rows);
    if (q.skip > 0 && (q.alternate || q.d_costs || q.d_raw_right)) return fail(SSAMD_EINVAL, "two row ranges: plain, consistent and exact matching only");
    if (q.skip == q.rows) return 1;
    if (!(q.gammaC > 0) || !(q.gammaP > 0)) return fail(SSAMD_EINVAL, "gammaC and gammaP must be positive");
    if (q.exact && (q.alternate || q.d_costs)) return fail(SSAMD_EINVAL, "the exact (fp64 tie-break) mode has no alternate-rows form and no cost dump");
    // alternate-rows mode: row0 is matched exactly, then every second row; the range must end with an exact row or with
    // the image (asw_alternate_rows arranges that for strips)
    if (q.alternate && q.d_costs) return fail(SSAMD_EINVAL, "the alternate-rows mode has no cost dump");
    return q.rows == 0 ? 1 : SSAMD_OK;
}

// The TAD volume is scratch of THIS library next to the caller's own allocations (torch's caching allocator on the
// same GPU): never more than 24 GiB and never more than half of what is free right now (plus what the buffer already
// holds).  The phase-shifted kernel builds its e tiles itself when there is no volume; the wave kernel cannot, so
// a range it would serve falls back to the workgroup geometry stored next to it.
// Free memory is only asked for (a driver query, tens of microseconds next to a 0.1 ms Tsukuba call) when a volume
// would have to GROW: what fits the buffer the context already holds fits.
bool asw_volume_fits(AswRun &r, size_t bytes)
{
    if (bytes > r.evol_cap_max) return false;
    if (bytes <= r.c.evol.cap) return true;
    if (!r.evol_limit) {
        size_t free_b = 0, total_b = 0;
        r.evol_limit = r.evol_cap_max;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) r.evol_limit = std::min(r.evol_cap_max, r.c.evol.cap + free_b / 2);
        else (void)hipGetLastError();
    }
    return bytes <= r.evol_limit;
}

bool asw_wave_volume_fits(AswRun &r, const AswGeom &g)
{
    AswWaveGeom wg;
    if (!g.wave_rx || !asw_wave_layout(wg, r.po, r.win, r.nD, g.wave_rx)) return !g.wave_rx;
    const int xt = (r.W + wg.Txw - 1) / wg.Txw, erows = std::min(r.H, r.row0 + r.rows + r.win / 2) - std::max(0, r.row0 - r.win / 2);
    return asw_volume_fits(r, (size_t)erows * (size_t)round_up(xt * wg.Txw + 2 * (r.win / 2), 4) * (size_t)wg.Se + 4096);
}

// Planning: the geometry (cached per shape), the autotuner's trial list, and what of both survives without room for a volume.
int asw_plan_call(AswRun &r)
{
    if (r.nD >= 1)
        if (int rc = asw_choose_geometry(r.geom, r.po, r.W, r.grows, r.win, r.nD)) return rc;
    // Autotuning (ssamd_autotune): the first call for a problem shape times the best geometry of every class of
    // candidates on the real buffers and keeps the fastest.  Every geometry accumulates the same taps in the same
    // order, so the result does not depend on the choice (and the trial launches are idempotent).
    const double call_taps = (double)r.W * r.grows * r.nD * r.win * r.win;
    if (autotune_due(g_asw_geom, r.shape, call_taps) && r.nD >= 1 && !asw_geometry_forced(r.t)) {
        AswGeom tmp;
        if (asw_search(tmp, r.po, r.W, r.grows, r.win, r.nD, &r.trial) != SSAMD_OK || r.trial.size() < 2) r.trial.clear();
    }
    r.evol_cap_max = r.t.evol_max_mb ? std::min((size_t)24 << 30, (size_t)r.t.evol_max_mb << 20) : (size_t)24 << 30;
    if (r.nD >= 1 && r.geom.wave_rx && !asw_wave_volume_fits(r, r.geom)) ++r.c.evol_fallbacks;
    if (r.nD >= 1 && !asw_wave_volume_fits(r, r.geom)) r.geom.wave_rx = 0;
    r.trial.erase(std::remove_if(r.trial.begin(), r.trial.end(), [&](const AswGeom &g) { return !asw_wave_volume_fits(r, g); }), r.trial.end());
    if (r.trial.size() < 2) r.trial.clear();
    r.need_keys = !asw_is_direct(r, r.geom) || r.alternate;  // the alternate mode merges its odd-row jobs through the left keys
    for (const AswGeom &g : r.trial) r.need_keys = r.need_keys || !asw_is_direct(r, g);
    return SSAMD_OK;
}

// Lab records of both images, one launch
int asw_lab_records(AswRun &r)
{
    Ctx &c = r.c;
    Timed t(c, r.s, SSAMD_K_LAB);
    if (r.rm)
        hipLaunchKernelGGL(remap_lab_records_pair_kernel, dim3(r.lab_blocks), dim3(256), 0, r.s, *r.rm, (PixRec *)c.recL.ptr, (PixRec *)c.recR.ptr,
                           (long long)r.r0 * r.W, r.np2);
    else
        hipLaunchKernelGGL(bgr2lab_records_pair_kernel, dim3(r.lab_blocks), dim3(256), 0, r.s, r.dL + (size_t)r.r0 * r.W * 3, r.dR + (size_t)r.r0 * r.W * 3,
                           (PixRec *)c.recL.ptr + (size_t)r.r0 * r.W, (PixRec *)c.recR.ptr + (size_t)r.r0 * r.W, r.np2);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// pre-computed truncated-absolute-difference volume for the phase-shifted and wave kernels (asw_tad_volume_kernel), or -- when the
// Lab records are still pending -- records and volume in one launch (asw_prepass_kernel);
// SSAMD_ASW_EVOL=0 keeps the in-kernel e tiles (experiments / tests)
int asw_prepare_volume(AswRun &r, const AswGeom &g)
{
    Ctx &c = r.c;
    hipStream_t s = r.s;
    r.evol = nullptr;
    int chunks = g.nchunks, Tx = g.Tx, Dc = g.Dc, Se = g.Se;
    if (g.wave_rx) {
        if (!asw_wave_layout(r.wave, r.po, r.win, r.nD, g.wave_rx, !r.d_costs && r.t.wave_unroll != 0))
            return fail(SSAMD_ELIMIT, "wave kernel geometry does not fit LDS");
        chunks = 1; Tx = r.wave.Txw; Dc = r.wave.Dc; Se = r.wave.Se;
    } else if (!g.pipe || r.t.asw_evol == 0) {
        return SSAMD_OK;
    }
    const int xt = (r.W + Tx - 1) / Tx, erows = r.r1 - r.r0;
    // rows stay 16-byte aligned for any Se; the phase-shifted kernel's half-width tail tiles (see asw_launch_pipe) may reach
    // up to half a tile + 4 columns further than the last full tile
    const int evolW = round_up(xt * Tx + 2 * r.p + (g.wave_rx ? 0 : Tx / 2 + 8), 4);
    const size_t bytes = (size_t)chunks * (size_t)erows * (size_t)evolW * (size_t)Se;
    // A buffer four times larger than the calls need is given back -- but only after eight such calls in a row
    // and never between the trial launches of the autotuner: a workload alternating a large and a small shape
    // (or the tuner's round-robin over wave and workgroup candidates) must not pay a device synchronisation,
    // a hipFree and a hipMalloc per switch.
    if (c.evol.cap > ((size_t)256 << 20) && (bytes + 4096) * 4 < c.evol.cap) {
        if (r.trial.empty() && ++c.evol_small_calls >= 8) {
            (void)hipStreamSynchronize(s);                    // (earlier launches of this call may still read it)
            c.evol.release();
            c.evol_small_calls = 0;
        }
    } else {
        c.evol_small_calls = 0;
    }
    int erc = SSAMD_ENOMEM;
    if (r.t.evol_fail) {                                      // test hook: a hipMalloc that really fails
        void *none = nullptr;
        size_t free_b = 0, total_b = (size_t)512 << 30;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (hipMalloc(&none, 2 * total_b) == hipSuccess) (void)hipFree(none);     // twice the device's memory
        // (deliberately NOT drained here: the fallback below has to cope with the sticky error itself)
    } else if (asw_volume_fits(r, bytes + 4096)) {
        erc = c.evol.reserve(bytes + 4096);                   // + one DMA piece of slack behind the last tile
    }
    if (erc) {
        (void)hipGetLastError();      // a failed hipMalloc stays the thread's last HIP error on ROCm 7: drop it before the launches' checks
        // the phase-shifted kernel builds its e tiles itself when there is no volume (evol == nullptr);
        // only the wave kernel cannot run without one
        if (g.wave_rx) return fail(erc == SSAMD_ENOMEM ? SSAMD_ENOMEM : erc, "TAD volume of %zu bytes does not fit the device memory left", bytes);
        ++c.evol_fallbacks;
        g_err.clear();
        return SSAMD_OK;
    }
    r.evol = (const unsigned char *)c.evol.ptr;
    r.evolW = evolW;
    const int rd = g.wave_rx ? r.wave.RD : 4;
    Timed t(c, s, SSAMD_K_LAB);
    const dim3 egrid((unsigned)((evolW + TADV_COLS - 1) / TADV_COLS), (unsigned)erows, (unsigned)chunks);
    const size_t elds = (size_t)(2 * TADV_COLS + Dc) * 4;
    const long long tiles = (long long)egrid.x * egrid.y * egrid.z;
    if (r.lab_pending && tiles + r.lab_blocks < (1ll << 31)) {
        AswPrepassArgs pa;
        pa.bgrL = r.dL; pa.bgrR = r.dR; pa.recL = (PixRec *)c.recL.ptr; pa.recR = (PixRec *)c.recR.ptr;
        pa.evol = (unsigned char *)c.evol.ptr; pa.npix_total = (long long)r.H * r.W;
        pa.W = r.W; pa.pad = r.p; pa.minD = r.minD; pa.Dc = Dc; pa.Se = Se; pa.erow0 = r.r0; pa.erows = erows; pa.evolW = evolW;
        pa.rd = rd;
        pa.lab_blocks = r.lab_blocks; pa.ex = (int)egrid.x; pa.ey = (int)egrid.y;
        if (int grc = grant_dyn_lds(c, (const void *)asw_prepass_kernel, (int)elds)) return grc;
        hipLaunchKernelGGL(asw_prepass_kernel, dim3((unsigned)(tiles + r.lab_blocks)), dim3(256), elds, s, pa);
        HIP_TRY(hipGetLastError());
        r.lab_pending = false;
        return SSAMD_OK;
    }
    if (r.lab_pending) {                   // (cannot share a launch: records first, as in rounds 2-4)
        r.lab_pending = false;
        if (int lrc = asw_lab_records(r)) return lrc;
    }
    if (int grc = grant_dyn_lds(c, (const void *)asw_tad_volume_kernel, (int)elds)) return grc;
    hipLaunchKernelGGL(asw_tad_volume_kernel, egrid, dim3(256), elds, s, (const PixRec *)c.recL.ptr, (const PixRec *)c.recR.ptr,
                       (unsigned char *)c.evol.ptr, r.W, r.p, r.minD, Dc, Se, r.r0, erows, evolW, rd);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// Every member AswArgs and AswWaveArgs share (all but the geometry), for a launch of geometry g.
template <class Args> void asw_fill_args(Args &x, const AswRun &r, const AswGeom &g)
{
    const bool direct = asw_is_direct(r, g);
    x.recL = (const PixRec *)r.c.recL.ptr; x.recR = (const PixRec *)r.c.recR.ptr;
    x.prox = r.d_prox;
    x.keyL = direct ? nullptr : (u64 *)r.c.keyL.ptr;
    x.keyR = r.consistent ? (u64 *)r.c.keyR.ptr : nullptr;
    x.disp = direct ? r.d_disp : nullptr;
    x.costs = r.d_costs;
    x.cost_keys = 0;
    x.xq = r.xq_kernel;                                               // (the autotuner's trial launches run without the queue)
    x.evol = r.evol; x.erow0 = r.r0; x.erows = r.r1 - r.r0; x.evolW = r.evolW;
    x.H = r.H; x.W = r.W; x.win = r.win; x.pad = r.p; x.minD = r.minD; x.maxD = r.maxD; x.row0 = r.row0; x.rows = r.rows;
    x.kC = (float)(-1.4426950408889634 / r.gammaC);
    x.ystep = r.alternate ? 2 : 1;
    x.yb0 = 0;
    x.yskip_at = r.skip > 0 ? r.skip_at : 0x7fffffff; x.yskip = r.skip;
}

int asw_launch_pipe(AswRun &r, const AswArgs &a, const dim3 &grid)
{
    Ctx &c = r.c;
    const AswGeom &g = a.g;
    const AswKernel pk = asw_pick_pipe_kernel(g, r.d_costs != nullptr, r.t.asw_static);
    const int pipe_lds = a.evol ? g.lds_bytes_evol : g.lds_bytes;          // (no staged colour bytes when the e tiles come from the volume)
    if (pipe_lds > 160 * 1024) return fail(SSAMD_ELIMIT, "this tile needs the TAD volume (LDS %d bytes without it)", pipe_lds);
    if (int grc = grant_dyn_lds(c, (const void *)pk, pipe_lds)) return grc;
    // The last PARTIAL round of workgroups (round 4).  The kernel keeps one 12-wave workgroup per CU, so a launch
    // of n workgroups takes ceil(n / 256) rounds: a row strip of an 8-GPU run (135 rows x 16 tiles = 8.44 rounds)
    // pays nine.  When the last round is at most half full, the rows that fill whole rounds keep the tile and the
    // remaining rows are launched with tiles of half the columns (twice the workgroups, half the taps each: the
    // round ends after about half its time).  Same taps in the same order per (x, d): maps cannot change
    // (tests/test_gpu_asw.py).  Worth ~4 % at 8.44 rounds, nothing beyond a few dozen; SSAMD_ASW_TAIL=0 / 1 forces.
    int rows_main = r.grows;
    AswGeom tail_g;
    // workgroups in flight at a time: the device's CUs x the tile's residency (168 VGPRs -> three waves per SIMD;
    // the tile's LDS).  One per CU for the 9- to 12-wave tiles of the headline configurations.
    const int per_simd = (g.threads / 64 + 3) / 4;
    const long long resident = std::max(1, std::min(3 / std::max(1, per_simd), (160 * 1024) / std::max(1, pipe_lds)));
    const long long per_row = (long long)grid.x * g.nchunks, slots = (long long)c.cus * resident;
    if (!r.alternate && r.t.asw_tail != 0 && g.XG >= 4) {
        const long long n = per_row * r.grows;
        const long long full = n / slots, rem = n - full * slots;
        if (full >= 1 && rem > 0 && 2 * rem <= slots && (full < 32 || r.t.asw_tail > 0)) {
            const int rm = (int)(full * slots / per_row);
            if (rm >= 1 && rm < r.grows &&
                asw_layout_e(tail_g, r.po, r.win, (g.XG + 1) / 2, g.DG, 160 * 1024, g.JC, 8, true, false, true) && tail_g.pipe &&
                tail_g.Se == g.Se && tail_g.Dc == g.Dc &&
                (a.evol == nullptr || round_up(((r.W + tail_g.Tx - 1) / tail_g.Tx) * tail_g.Tx + 2 * r.p, 4) <= a.evolW)) {
                tail_g.nchunks = g.nchunks;
                rows_main = rm;
            }
        }
    }
    // The persistent form (round 8, asw_pipe_kernel.hip.h): as many workgroups as are resident at a time, each drawing the launch's
    // tiles as items from eight queues.  What it recovers is the XCD whose tiles include the light left-border ones running dry
    // about 12 % of the launch early (the dispatcher deals blocks to XCDs by id % 8 whatever their load: profiles/r08_xcd_dispatch.txt)
    // and the round quantisation; what it costs is fixed (the memset, one exposed ticket).  Measured on the 120 x 196 tile
    // (profiles/r08_pipe_persistent.txt): + 0.6 % at 8 full rounds, + 0.3 % at 16, nothing either way at 33.75, - 0.8 ... - 1.2 % at 67.5
    // (1080p), - 1.5 % at 4096 x 2160.  The host picks it from 64 full rounds on: where it is measured to gain.  Between 34 and 64
    // rounds nothing is measured and the launch stays the plain grid.  SSAMD_ASW_PERSIST=0 / n forces the plain grid /
    // min(n, slots) workgroups.  Same tiles, same instructions.
    const long long items = per_row * rows_main;
    long long workers = r.t.asw_persist > 0 ? std::min<long long>(r.t.asw_persist, slots) : (r.t.asw_persist < 0 && items >= 64 * slots ? slots : 0);
    workers = std::min(workers, items);
    if (workers > 0 && items < (1ll << 30)) {
        const size_t pq_bytes = (size_t)(ASW_PQ_QUEUES + 1) * ASW_PQ_LINE * 4;
        if (!c.pq.ptr) {
            if (int prc = c.pq.reserve(pq_bytes)) return prc;
            HIP_TRY(hipMemsetAsync(c.pq.ptr, 0, pq_bytes, r.s));       // (the counter of finished items behind the queues' is never zeroed again)
        }
        HIP_TRY(hipMemsetAsync(c.pq.ptr, 0, (size_t)ASW_PQ_QUEUES * ASW_PQ_LINE * 4, r.s));
        AswArgs pa = a;
        pa.pq = (unsigned int *)c.pq.ptr;
        pa.pq_nx = (int)grid.x; pa.pq_ny = rows_main; pa.pq_items = (int)items;
        ++c.persist_launches;
        hipLaunchKernelGGL(pk, dim3((unsigned)workers), dim3(g.threads), pipe_lds, r.s, pa);
    } else {
        hipLaunchKernelGGL(pk, dim3(grid.x, rows_main, grid.z), dim3(g.threads), pipe_lds, r.s, a);
    }
    HIP_TRY(hipGetLastError());
    if (rows_main < r.grows) {
        ++c.tail_splits;
        AswArgs t = a;
        t.g = tail_g;
        t.yb0 = rows_main;              // (workgroup rows continue; outputs are addressed by image row, so the buffers stay put)
        const AswKernel tk = asw_pick_pipe_kernel(tail_g, r.d_costs != nullptr, 0);
        const int tail_lds = a.evol ? tail_g.lds_bytes_evol : tail_g.lds_bytes;
        if (int grc = grant_dyn_lds(c, (const void *)tk, tail_lds)) return grc;
        hipLaunchKernelGGL(tk, dim3((r.W + tail_g.Tx - 1) / tail_g.Tx, r.grows - rows_main, tail_g.nchunks), dim3(tail_g.threads),
                           tail_lds, r.s, t);
        HIP_TRY(hipGetLastError());
    }
    return SSAMD_OK;
}

// The aggregation launch of geometry g (after asw_prepare_volume(r, g)); r.geom = g afterwards.
int asw_launch(AswRun &r, const AswGeom &g)
{
    r.geom = g;
    if (g.wave_rx) {                  // (asw_prepare_volume(r, g) filled r.wave and built the volume)
        AswWaveArgs wa;
        asw_fill_args(wa, r, g);
        wa.g = r.wave;
        const AswWaveKernel wk = asw_pick_wave_kernel(wa.g, r.d_costs != nullptr, r.t.wave_unroll != 0);
        const int lds = wa.g.wave_lds * wa.g.waves, xt = (r.W + wa.g.Txw - 1) / wa.g.Txw;
        if (int grc = grant_dyn_lds(r.c, (const void *)wk, lds)) return grc;
        hipLaunchKernelGGL(wk, dim3((xt + wa.g.waves - 1) / wa.g.waves, r.grows, 1), dim3(64 * wa.g.waves), lds, r.s, wa);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    }
    AswArgs a{};
    asw_fill_args(a, r, g);
    a.g = g;
    const dim3 grid((r.W + g.Tx - 1) / g.Tx, r.grows, g.nchunks);
    if (g.pipe) return asw_launch_pipe(r, a, grid);
    const bool chunked = g.JC < r.win;
    AswKernel kern = chunked ? (r.d_costs ? asw_aggregate_kernel<true, true> : asw_aggregate_kernel<false, true>)
                             : (r.d_costs ? asw_aggregate_kernel<true, false> : asw_aggregate_kernel<false, false>);
    if (g.Rx == 4)
        kern = chunked ? (r.d_costs ? asw_aggregate_kernel<true, true, 4> : asw_aggregate_kernel<false, true, 4>)
                       : (r.d_costs ? asw_aggregate_kernel<true, false, 4> : asw_aggregate_kernel<false, false, 4>);
    if (int grc = grant_dyn_lds(r.c, (const void *)kern, g.lds_bytes)) return grc;
    hipLaunchKernelGGL(kern, grid, dim3(g.threads), g.lds_bytes, r.s, a);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// The autotuner's trial launches: times r.trial on the call's own buffers, caches the fastest for the shape, leaves it in r.geom.
int asw_autotune(AswRun &r)
{
    hipStream_t s = r.s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    bool all_prepared = true;     // a candidate whose volume cannot be had right now is never launched, and the verdict of such a round is not cached
    // (a phase-shifted tile whose volume cannot be had is timed with in-kernel e tiles, or fails its launch when it was
    //  planned on the volume's LDS saving: that round says nothing about the tile, so its verdict is not kept either)
    const bool want_evol = r.t.asw_evol != 0;
    for (const AswGeom &g : r.trial) {                                             // code load, clocks, scratch
        if (asw_prepare_volume(r, g) != SSAMD_OK) { all_prepared = false; continue; }
        if (g.pipe && !g.wave_rx && want_evol && !r.evol) all_prepared = false;
        if (asw_launch(r, g) != SSAMD_OK) all_prepared = false;
    }
    const int fastest = autotune_rounds(r.trial.size(), 4, false, e0, e1, s, &all_prepared, [&](size_t ci) {
        const AswGeom &g = r.trial[ci];
        const bool launched = asw_prepare_volume(r, g) == SSAMD_OK && asw_launch(r, g) == SSAMD_OK;
        if (g.pipe && !g.wave_rx && want_evol && !r.evol) all_prepared = false;
        return launched;
    });
    if (fastest >= 0) r.geom = r.trial[fastest];      // (none timed: the geometry launched last)
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (all_prepared) autotune_keep(g_asw_geom, r.shape, r.geom);
    else g_err.clear();
    return SSAMD_OK;
}

// The final geometry's volume, with the two ways out when it cannot be had.  final_geom may change; r.need_keys follows.
int asw_final_volume(AswRun &r, AswGeom &final_geom)
{
    int rc = asw_prepare_volume(r, final_geom);
    if (rc == SSAMD_ENOMEM && final_geom.wave_rx) {
        // the volume's hipMalloc failed although the pre-check said it fits (fragmentation, another allocator on the
        // same GPU): the wave kernel cannot run without it, the workgroup geometry stored next to it can (in-kernel
        // e tiles, or a smaller volume if that one can be had)
        ++r.c.evol_fallbacks;
        g_err.clear();
        final_geom.wave_rx = 0;
        r.geom = final_geom;
        if (!asw_is_direct(r, final_geom) && !r.need_keys) {
            if ((rc = reset_keys(r.c.keyL, r.nout, r.s))) return rc;
            r.need_keys = true;
        }
        rc = asw_prepare_volume(r, final_geom);
    }
    if (rc) return rc;
    if (final_geom.pipe && !final_geom.wave_rx && !r.evol && final_geom.lds_bytes > 160 * 1024) {
        // the tile was planned on the TAD volume (no staged colour bytes in LDS) and the volume cannot be had: plan
        // again for the in-kernel e tiles (PlanOptions::no_volume)
        AswGeom g2;
        if ((rc = asw_search(g2, PlanOptions{r.t, true}, r.W, r.grows, r.win, r.nD))) return rc;
        g2.wave_rx = 0;
        if (!asw_is_direct(r, g2) && !r.need_keys && (rc = reset_keys(r.c.keyL, r.nout, r.s))) return rc;
        final_geom = g2;
        if ((rc = asw_prepare_volume(r, final_geom))) return rc;
    }
    return SSAMD_OK;
}

// odd rows of the alternate-rows mode: candidates bounded by the exact rows above and below (asw_alt_kernels.hip.h).  With an
// empty disparity range the decode already wrote x everywhere and the fill reproduces it.
int asw_alternate_fill(AswRun &r)
{
    Ctx &c = r.c;
    hipStream_t s = r.s;
    int rc;
    AswAltArgs f;
    const size_t nodd = (size_t)(r.rows / 2) * r.W;
    if ((double)nodd * ((r.nD + 7) / 8 + 1) >= 4.0e9)
        return fail(SSAMD_ELIMIT, "alternate-rows mode: image x disparity range too large for the 32-bit job counter");
    f.cap = (unsigned int)std::min<size_t>(std::max<size_t>(nodd, 1 << 16), 1u << 28);   // jobs of 8 candidates
    if (r.t.alt_queue_cap)                                      // test hook: a tiny queue forces the in-place path
        f.cap = (unsigned int)r.t.alt_queue_cap;
    if ((rc = c.altq.reserve((size_t)f.cap * 8 + 16))) return rc;
    f.ctr = (unsigned int *)c.altq.ptr; f.queue = (u64 *)((char *)c.altq.ptr + 16);
    HIP_TRY(hipMemsetAsync(f.ctr, 0, 16, s));
    f.recL = (const PixRec *)c.recL.ptr; f.recR = (const PixRec *)c.recR.ptr; f.prox = r.d_prox;
    f.disp = r.d_disp; f.key = (u64 *)c.keyL.ptr;
    f.H = r.H; f.W = r.W; f.win = r.win; f.pad = r.p; f.minD = r.minD; f.maxD = r.maxD; f.row0 = r.row0; f.rows = r.rows;
    f.kC = (float)(-1.4426950408889634 / r.gammaC);
    const dim3 pix_grid((r.W + 255) / 256, r.rows / 2);
    Timed t(c, s, SSAMD_K_ASW_ALT);
    hipLaunchKernelGGL(asw_alt_scan_kernel, pix_grid, dim3(256), 0, s, f);
    hipLaunchKernelGGL(asw_alt_jobs_kernel, dim3(256 * 8), dim3(256), 0, s, f);
    hipLaunchKernelGGL(asw_alt_decode_kernel, pix_grid, dim3(256), 0, s, f);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int asw_device_impl(Ctx &c, const AswCall &q)
{
    int rc = asw_check_call(q);
    if (rc) return rc > 0 ? SSAMD_OK : rc;
    hipStream_t s = q.s;
    ScratchOrder order(c, s);
    const Tuning &t = tune();
    AswRun r{q, c, t, PlanOptions{t, false}};
    r.exact = q.exact && q.maxD >= q.minD;                            // empty candidate loops: nothing to break ties between
    r.p = q.win / 2; r.nD = q.maxD - q.minD + 1;
    r.nout = (size_t)q.rows * q.W;
    r.grows = q.alternate ? (q.rows + 1) / 2 : q.rows - q.skip;       // workgroup rows: every row (of both ranges), or the even ones
    r.shape = {q.W, r.grows, q.win, r.nD};
    r.r0 = std::max(0, q.row0 - r.p); r.r1 = std::min(q.H, q.row0 + q.rows + r.p);
    r.np2 = (long long)(r.r1 - r.r0) * q.W;
    r.lab_blocks = (int)std::min<long long>((2 * r.np2 + 255) / 256, 256 * 8);
    if ((rc = asw_plan_call(r))) return rc;
    if (r.need_keys && (rc = reset_keys(c.keyL, r.nout, s))) return rc;
    if (q.consistent && (rc = reset_keys(c.keyR, r.nout, s))) return rc;
    if (r.nD >= 1) {
        if ((rc = c.recL.reserve((size_t)q.H * q.W * sizeof(PixRec)))) return rc;
        if ((rc = c.recR.reserve((size_t)q.H * q.W * sizeof(PixRec)))) return rc;
        if ((rc = get_prox(c, q.win, q.gammaP, s, &r.d_prox))) return rc;
        // Round 5: when the call goes straight to its final geometry (no trial launches) and the images are plain byte arrays, the
        // records are NOT launched here: the TAD volume is then built from the images' bytes, independent of the records, and both
        // jobs share one launch (asw_prepass_kernel, see asw_prepare_volume) -- two dependent launches per call instead of three.
        r.lab_pending = r.trial.empty() && !q.rm && t.prepass_fuse != 0;
        if (!r.lab_pending && (rc = asw_lab_records(r))) return rc;
        if (!r.trial.empty() && (rc = asw_autotune(r))) return rc;
        AswGeom final_geom = r.geom;
        if ((rc = asw_final_volume(r, final_geom))) return rc;
        if (r.lab_pending) {                   // no volume for this call (in-kernel e tiles, round-1 kernel): the records on their own
            r.lab_pending = false;
            if ((rc = asw_lab_records(r))) return rc;
        }
        if (r.exact) {
            if (!r.trial.empty()) {
                // the trial launches of the autotuner merged their winners into the keys: start the final launch from clean
                // ones, or its tile-local winners would meet their own copies (asw_exact_merge)
                if (r.need_keys && (rc = reset_keys(c.keyL, r.nout, s))) return rc;
                if (q.consistent && (rc = reset_keys(c.keyR, r.nout, s))) return rc;
            }
            if ((rc = asw_exact_prepare(c, q.W, q.rows, q.win, r.nD, q.gammaC, q.consistent, asw_is_direct(r, final_geom), s, r.xq_final, r.xq_raw, r.xq_kernel))) return rc;
        }
        Timed agg(c, s, SSAMD_K_ASW_AGG);
        if ((rc = asw_launch(r, final_geom))) return rc;
    }
    const bool direct = asw_is_direct(r, r.geom);
    if (r.exact && r.nD >= 1 &&
        (rc = asw_exact_pass(c, r.xq_final, r.xq_raw, q.H, q.W, q.row0, q.rows, q.win, q.maxD, q.minD, q.gammaC, q.gammaP, q.consistent, direct, q.d_disp, s)))
        return rc;
    if (!direct && q.skip > 0) {
        // decode / left-right check of the two bands only; the rows between keep what the interior call wrote
        if ((rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, 0, q.skip_at, q.W, q.d_disp, s)) ||
            (rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, q.skip_at + q.skip, q.rows - q.skip_at - q.skip, q.W, q.d_disp, s)))
            return rc;
    } else if (!direct && (rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, 0, q.rows, q.W, q.d_disp, s, q.d_raw_right))) return rc;
    return q.alternate && q.rows > 1 ? asw_alternate_fill(r) : SSAMD_OK;
}

// The alternate-rows mode on a row range of a (sub-)image.  row_parity = parity of the sub-image's row 0 in the whole
// image: rows whose index in the whole image is even are matched exactly, the odd ones are filled from their two exact
// neighbours -- so a range that starts or ends with an odd row also needs the exact row just outside it (the caller's
// halo is winSize/2 + 1 rows then).  Those rows are computed into a scratch map and the requested rows copied out.
int asw_alternate_rows(Ctx &c, AswCall q, int row_parity)
{
    int rc = check_common(q.H, q.W, q.win, q.minD, q.maxD, q.row0, q.rows);
    if (rc) return rc;
    if (q.rows == 0) return SSAMD_OK;
    const int row0 = q.row0, rows = q.rows;
    const bool top_odd = ((row0 + row_parity) & 1) != 0, bottom_odd = ((row0 + rows - 1 + row_parity) & 1) != 0;
    if (top_odd && row0 == 0)
        return fail(SSAMD_EINVAL, "alternate rows: the first output row is an odd row of the image, the sub-image must start at least one row above it");
    const int e0 = top_odd ? row0 - 1 : row0, e1 = bottom_odd ? std::min(q.H, row0 + rows + 1) : row0 + rows;
    q.alternate = true;
    if (e0 == row0 && e1 == row0 + rows) return asw_device_impl(c, q);
    ScratchOrder order(c, q.s);
    if ((rc = c.altdisp.reserve((size_t)(e1 - e0) * q.W * 2))) return rc;
    int16_t *const d_disp = q.d_disp;
    q.row0 = e0; q.rows = e1 - e0; q.d_disp = (int16_t *)c.altdisp.ptr;
    if ((rc = asw_device_impl(c, q))) return rc;
    HIP_TRY(hipMemcpyAsync(d_disp, (const int16_t *)c.altdisp.ptr + (size_t)(row0 - e0) * q.W, (size_t)rows * q.W * 2, hipMemcpyDeviceToDevice, q.s));
    return SSAMD_OK;
}

// ------------------------------------------------------------ GSW
int gsw_device_impl(Ctx &c, const uint8_t *dL, const uint8_t *dR, int H, int W, int row0, int rows, int win, int maxD,
                    int minD, int gamma, float fMax, int iterations, int16_t *d_disp, hipStream_t s, const RemapSrc *rm = nullptr)
{
    int rc = check_common(H, W, win, minD, maxD, row0, rows);
    if (rc) return rc;
    if (gamma == 0) return fail(SSAMD_EINVAL, "gamma must be non-zero");
    if (rows == 0) return SSAMD_OK;
    ScratchOrder order(c, s);
    const Tuning &opts = tune();
    const int p = win / 2, nD = maxD - minD + 1;
    const size_t npix = (size_t)H * W, nout = (size_t)rows * W;
    if ((rc = c.keyL.reserve(nout * 8)) || (rc = c.keyR.reserve(nout * 8))) return rc;
    HIP_TRY(hipMemsetAsync(c.keyL.ptr, 0xFF, nout * 8, s));
    HIP_TRY(hipMemsetAsync(c.keyR.ptr, 0xFF, nout * 8, s));
    if (nD >= 1) {
        // packed pixels live in the (larger) ASW record buffers: 4 B/pixel
        if ((rc = c.recL.reserve(npix * 4)) || (rc = c.recR.reserve(npix * 4))) return rc;
        const float *d_tab = nullptr;
        if ((rc = get_gsw_table(c, gamma, s, &d_tab))) return rc;
        const int r0 = std::max(0, row0 - p), r1 = std::min(H, row0 + rows + p);
        const long long np = (long long)(r1 - r0) * W;
        const int blocks = (int)std::min<long long>((np + 255) / 256, 256 * 8);
        {
            Timed t(c, s, SSAMD_K_LAB);
            if (rm) {       // raw frames through the rig's maps: rectification + packing of both images, one launch
                hipLaunchKernelGGL(remap_pack_pair_kernel, dim3(blocks), dim3(256), 0, s, *rm, (uint32_t *)c.recL.ptr, (uint32_t *)c.recR.ptr,
                                   (long long)r0 * W, np);
            } else {
                hipLaunchKernelGGL(bgr_pack_kernel, dim3(blocks), dim3(256), 0, s, dL + (size_t)r0 * W * 3,
                                   (uint32_t *)c.recL.ptr + (size_t)r0 * W, np);
                hipLaunchKernelGGL(bgr_pack_kernel, dim3(blocks), dim3(256), 0, s, dR + (size_t)r0 * W * 3,
                                   (uint32_t *)c.recR.ptr + (size_t)r0 * W, np);
            }
            HIP_TRY(hipGetLastError());
        }
        GswArgs a;
        if ((rc = gsw_choose_geometry(a.g, opts, W, rows, win, nD))) return rc;
        a.tab = d_tab;
        a.H = H; a.W = W; a.win = win; a.pad = p; a.minD = minD; a.maxD = maxD; a.row0 = row0; a.rows = rows;
        a.iterations = iterations; a.fMax = fMax;
        // both passes with geometry g (the winner-take-all keys merge by atomicMin: repeated launches are idempotent)
        auto launch = [&](const GswGeom &g) -> int {
            a.g = g;
            const int TyS = g.Ty * g.Hy;
            const dim3 grid((W + g.Tx - 1) / g.Tx, (rows + TyS - 1) / TyS, g.nchunks), block(g.threads * g.Hy);
            auto kernel = g.Ty == 2 ? gsw_aggregate_kernel<2, 4> : gsw_aggregate_kernel<1, 8>;
            if (int grc = grant_dyn_lds(c, (const void *)kernel, g.lds_bytes)) return grc;
            for (int pass = 0; pass < 2; ++pass) {
                a.right = pass;
                a.ref = (const uint32_t *)(pass ? c.recR.ptr : c.recL.ptr);
                a.tgt = (const uint32_t *)(pass ? c.recL.ptr : c.recR.ptr);
                a.key = (u64 *)(pass ? c.keyR.ptr : c.keyL.ptr);
                hipLaunchKernelGGL(kernel, grid, block, g.lds_bytes, s, a);
                HIP_TRY(hipGetLastError());
            }
            return SSAMD_OK;
        };
        // Autotuning (ssamd_autotune, as for ASW): the first call of a shape times the candidates of gsw_candidates on the
        // call's own buffers -- three rounds in round-robin order, fastest launch of each (autotune_rounds) -- and caches the winner.  Default
        // mode: calls of at most 6e10 window taps (both passes; 2 lane-ops each: about 5 ms), where the model is least reliable.
        const ShapeKey shape{W, rows, win, nD};
        if (autotune_due(g_gsw_geom, shape, 2.0 * (double)W * rows * nD * win * win) && opts.gsw_geom.empty()) {
            std::vector<GswGeom> trial;
            gsw_candidates(trial, a.g, W, rows, win, nD);
            if (trial.size() >= 2) {
                hipEvent_t e0 = nullptr, e1 = nullptr;
                HIP_TRY(hipEventCreate(&e0));
                if (hipEventCreate(&e1) != hipSuccess) {
                    (void)hipEventDestroy(e0);
                    return fail(SSAMD_EHIP, "hipEventCreate failed");
                }
                const int fastest = autotune_rounds(trial.size(), 3, true, e0, e1, s, nullptr, [&](size_t ci) { return launch(trial[ci]) == SSAMD_OK; });
                (void)hipGetLastError();
                g_err.clear();            // a failed trial launch is not the call's error
                a.g = trial[std::max(0, fastest)];
                (void)hipEventDestroy(e0);
                (void)hipEventDestroy(e1);
                autotune_keep(g_gsw_geom, shape, a.g);
            }
        }
        {
            const GswGeom final_geom = a.g;
            Timed t(c, s, SSAMD_K_GSW_AGG);
            if ((rc = launch(final_geom))) return rc;
        }
    }
    return launch_finalize(c, SSAMD_K_GSW_FIN, true, 0, rows, W, d_disp, s);   // consistency is unconditional in GSW
}

}  // namespace

// =================================================================== C ABI
namespace {

// ---- host-buffer paths: H2D copy of rows [in0, in1) of both images, kernels on output rows [o0, o1), D2H copy.
// Used for the whole image (ssamd_asw / ssamd_gsw) and, one host thread per device, for the row strips of
// ssamd_*_multi: output row y needs input rows y-pad .. y+pad only and the left-right check and occlusion filling
// are row-local (_passive.cpp:38-40, 60-62, 251-285), so a strip that carries its halo reproduces the rows of the
// whole-image result bit for bit.
struct HostJob {
    const uint8_t *img1, *img2;
    int H, W, win, maxD, minD;
    int o0, o1;                    // output rows of the full image
    int16_t *disparity;            // full-image output [H][W]
    // ASW
    double gammaC, gammaP; int consistent; float *costs; bool alternate;
    bool exact;                    // fp64 tie-break pass (ssamd_asw_exact*)
    int16_t *raw_right;            // verification dump (ssamd_asw_argmins): raw right-referenced matches, full image
    // GSW
    bool gsw; int gamma; float fMax; int iterations;
};

int host_rows(const HostJob &j, int device)
{
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    if ((rc = check_common(j.H, j.W, j.win, j.minD, j.maxD, j.o0, j.o1 - j.o0))) return rc;
    const int p = j.win / 2 + (j.alternate ? 1 : 0);        // alternate rows: + the exact row beyond an odd first / last row
    const int in0 = std::max(0, j.o0 - p), in1 = std::min(j.H, j.o1 + p), rows = j.o1 - j.o0;
    const size_t nb = (size_t)(in1 - in0) * j.W * 3, nout = (size_t)rows * j.W;
    if ((rc = c->imgL.reserve(nb)) || (rc = c->imgR.reserve(nb)) || (rc = c->disp.reserve(nout * 2))) return rc;
    const size_t ncost = j.costs ? nout * (size_t)std::max(1, j.maxD - j.minD + 1) : 0;
    if (j.costs && (rc = c->costs.reserve(ncost * 4))) return rc;
    if (j.raw_right && (rc = c->lab.reserve(nout * 2))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, j.img1 + (size_t)in0 * j.W * 3, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->imgR.ptr, j.img2 + (size_t)in0 * j.W * 3, nb, hipMemcpyHostToDevice, s));
    if (j.costs) HIP_TRY(hipMemsetAsync(c->costs.ptr, 0xFF, ncost * 4, s));      // 0xFFFFFFFF = NaN
    if (j.gsw) {
        rc = gsw_device_impl(*c, (const uint8_t *)c->imgL.ptr, (const uint8_t *)c->imgR.ptr, in1 - in0, j.W, j.o0 - in0, rows,
                             j.win, j.maxD, j.minD, j.gamma, j.fMax, j.iterations, (int16_t *)c->disp.ptr, s);
    } else {
        AswCall q;
        q.dL = (const uint8_t *)c->imgL.ptr; q.dR = (const uint8_t *)c->imgR.ptr;
        q.H = in1 - in0; q.W = j.W; q.row0 = j.o0 - in0; q.rows = rows;
        q.win = j.win; q.maxD = j.maxD; q.minD = j.minD; q.gammaC = j.gammaC; q.gammaP = j.gammaP; q.consistent = j.consistent != 0;
        q.d_disp = (int16_t *)c->disp.ptr; q.s = s;
        if (!j.alternate) {
            q.exact = j.exact;
            q.d_costs = j.costs ? (float *)c->costs.ptr : nullptr;
            q.d_raw_right = j.raw_right ? (int16_t *)c->lab.ptr : nullptr;
        }
        rc = j.alternate ? asw_alternate_rows(*c, q, in0 & 1) : asw_device_impl(*c, q);
    }
    if (rc) return rc;
    if (j.raw_right)
        HIP_TRY(hipMemcpyAsync(j.raw_right + (size_t)j.o0 * j.W, c->lab.ptr, nout * 2, hipMemcpyDeviceToHost, s));
    if (j.disparity)
        HIP_TRY(hipMemcpyAsync(j.disparity + (size_t)j.o0 * j.W, c->disp.ptr, nout * 2, hipMemcpyDeviceToHost, s));
    if (j.costs) HIP_TRY(hipMemcpyAsync(j.costs, c->costs.ptr, ncost * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

// Contiguous row strips whose heights differ by at most one row (empty when there are more devices than rows) --
// the same cut as simplestereo_amd/strips.py::strip_bounds.  One host thread per strip: each takes its own device's lock, so the
// copies and kernels of all devices overlap.  The first failing strip's code and message are returned.
int run_strips(const HostJob &job, const int *devices, int n_devices)
{
    if (!devices || n_devices < 1) return fail(SSAMD_EINVAL, "devices must name at least one GPU");
    if (n_devices > 16) return fail(SSAMD_EINVAL, "at most 16 devices");
    for (int a = 0; a < n_devices; ++a) {
        if (devices[a] < 0) return fail(SSAMD_EINVAL, "devices[%d] = %d: explicit non-negative ordinals only", a, devices[a]);
        // test hook SSAMD_MULTI_ALLOW_REPEAT: a 1-GPU box exercises the strip cut with one device listed several
        // times (the strips then simply queue on that device's mutex)
        for (int b = 0; b < a && !tune().multi_allow_repeat; ++b)
            if (devices[a] == devices[b]) return fail(SSAMD_EINVAL, "device %d listed twice", devices[a]);
    }
    int rc = check_common(job.H, job.W, job.win, job.minD, job.maxD, 0, job.H);
    if (rc) return rc;
    const int base = job.H / n_devices, extra = job.H % n_devices;
    std::vector<int> codes(n_devices, SSAMD_OK);
    std::vector<std::string> msgs(n_devices);
    std::vector<std::thread> th;
    for (int k = 0; k < n_devices; ++k) {
        HostJob j = job;
        j.o0 = k * base + std::min(k, extra);
        j.o1 = j.o0 + base + (k < extra ? 1 : 0);
        if (j.o1 <= j.o0) continue;                      // more devices than rows: nothing for this one
        const int dev = devices[k];
        try {
            th.emplace_back([j, dev, k, &codes, &msgs]() {
                codes[k] = host_rows(j, dev);
                if (codes[k]) msgs[k] = g_err;           // thread-local message of the worker
            });
        } catch (const std::exception &e) {              // no exception may cross the C ABI: finish what runs, report
            codes[k] = SSAMD_ENOMEM;
            msgs[k] = std::string("could not start a host thread: ") + e.what();
            break;
        }
    }
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; ++k)
        if (codes[k]) return fail(codes[k], "strip %d on device %d: %s", k, devices[k], msgs[k].c_str());
    return SSAMD_OK;
}

HostJob asw_job(const uint8_t *img1, const uint8_t *img2, int H, int W, int win, int maxD, int minD, double gammaC,
                double gammaP, int consistent, int16_t *disparity, float *costs, bool alternate, bool exact = false)
{
    HostJob j{};
    j.img1 = img1; j.img2 = img2; j.H = H; j.W = W; j.win = win; j.maxD = maxD; j.minD = minD; j.o0 = 0; j.o1 = H;
    j.disparity = disparity; j.gammaC = gammaC; j.gammaP = gammaP; j.consistent = consistent; j.costs = costs;
    j.alternate = alternate; j.exact = exact;
    return j;
}

HostJob gsw_job(const uint8_t *img1, const uint8_t *img2, int H, int W, int win, int maxD, int minD, int gamma, float fMax,
                int iterations, int16_t *disparity)
{
    HostJob j{};
    j.img1 = img1; j.img2 = img2; j.H = H; j.W = W; j.win = win; j.maxD = maxD; j.minD = minD; j.o0 = 0; j.o1 = H;
    j.disparity = disparity; j.gsw = true; j.gamma = gamma; j.fMax = fMax; j.iterations = iterations;
    return j;
}

// The rig's raw frames and maps of the *_rectified_device entry points, with their argument checks (d_out: checked with them)
int make_remap_src(RemapSrc &rm, const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                   const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int interpolation, const void *d_out)
{
    if (!d_raw1 || !d_raw2 || !d_mapx1 || !d_mapy1 || !d_mapx2 || !d_mapy2 || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    if (src_height <= 0 || src_width <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (interpolation != 0 && interpolation != 1) return fail(SSAMD_EINVAL, "only INTER_NEAREST (0) and INTER_LINEAR (1) are supported");
    rm.src1 = d_raw1; rm.src2 = d_raw2; rm.mapx1 = d_mapx1; rm.mapy1 = d_mapy1; rm.mapx2 = d_mapx2; rm.mapy2 = d_mapy2;
    rm.Hs = src_height; rm.Ws = src_width; rm.nearest = interpolation == 0 ? 1 : 0;
    return SSAMD_OK;
}

// ssamd_asw_device, ssamd_asw_device_rows2 (skip_rows > 0), ssamd_asw_alternate_device and, with rm (checked by make_remap_src),
// ssamd_asw_rectified_device; `exact`: their _exact twins
int asw_device_entry(const RemapSrc *rm, const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                     int skip_row0, int skip_rows, int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP,
                     int consistent, int16_t *d_disparity, void *stream, bool exact, bool alternate = false)
{
    if (!rm && (!d_img1 || !d_img2 || !d_disparity)) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    if (skip_rows < 0 || (skip_rows > 0 && (skip_row0 < out_row0 || skip_row0 + skip_rows > out_row0 + out_rows)))
        return fail(SSAMD_EINVAL, "the skipped rows [%d,%d) must lie inside the output rows [%d,%d)", skip_row0, skip_row0 + skip_rows,
                    out_row0, out_row0 + out_rows);
    AswCall q;
    q.rm = rm; q.dL = d_img1; q.dR = d_img2; q.H = height; q.W = width; q.row0 = out_row0; q.rows = out_rows;
    q.skip_at = skip_rows > 0 ? skip_row0 - out_row0 : 0; q.skip = skip_rows;
    q.win = winSize; q.maxD = maxDisparity; q.minD = minDisparity; q.gammaC = gammaC; q.gammaP = gammaP; q.consistent = consistent != 0;
    q.exact = exact; q.alternate = alternate; q.d_disp = d_disparity; q.s = (hipStream_t)stream;
    return asw_device_impl(*c, q);
}

int asw_rectified_entry(const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                        const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int height, int width, int interpolation,
                        int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                        int16_t *d_disparity, void *stream, bool exact)
{
    RemapSrc rm;
    const int rc = make_remap_src(rm, d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, interpolation, d_disparity);
    return rc ? rc : asw_device_entry(&rm, nullptr, nullptr, height, width, 0, height, 0, 0, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                      consistent, d_disparity, stream, exact);
}

int check_geometry_query(int width, int winSize, int maxDisparity, int minDisparity, const int *out, int *nD)
{
    if (!out) return fail(SSAMD_EINVAL, "out is NULL");
    int rc = check_common(1 << 14, width, winSize, minDisparity, maxDisparity, 0, 0);
    if (rc) return rc;
    *nD = maxDisparity - minDisparity + 1;
    return *nD < 1 ? fail(SSAMD_EINVAL, "empty disparity range") : SSAMD_OK;
}
}  // namespace

extern "C" {

int ssamd_abi_version(void) { return SSAMD_ABI_VERSION; }
const char *ssamd_last_error(void) { return g_err.c_str(); }

int ssamd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ssamd_kernel_name(int slot)
{
    static const char *names[SSAMD_K_COUNT] = {"asw pre-pass (asw_prepass_kernel: Lab records + TAD volume; or bgr2lab_records_pair_kernel, asw_tad_volume_kernel)", "asw aggregation kernel (asw_aggregate_pipe / _wave / asw_aggregate_kernel)",
                                               "asw finalize (wta_decode / lr_check_fill)",
                                               "gsw_aggregate_kernel", "gsw finalize (lr_check_fill)", "remap_bgr_kernel", "reproject_kernel / ftp_cloud_kernel",
                                               "asw_alt_fill_kernel", "asw fp64 tie-break pass (bgr2lab_f64_pair + asw_exact_winners / _eval / _resolve / _patch kernels)",
                                               "iir_unwrap_kernel", "ftp_phase_kernel", "np_unwrap_row_kernel / np_unwrap_col_kernel"};
    return (slot >= 0 && slot < SSAMD_K_COUNT) ? names[slot] : "";
}

int ssamd_set_option(const char *name, const char *value)
{
    if (!name) return fail(SSAMD_EINVAL, "option name is NULL");
    std::lock_guard<std::mutex> lk(g_tune_mutex);
    if (value) {
        if (!tuning_assign(g_tuning, name, value)) return fail(SSAMD_EINVAL, "unknown option %s", name);
    } else {
        // NULL = back to the value the library loaded from the environment (not "unset": a process started with
        // SSAMD_ASW_WAVE=0 keeps that setting after a `with options(...)` block of a test)
        const auto it = g_tuning_env.find(name);
        if (!tuning_assign(g_tuning, name, it == g_tuning_env.end() ? nullptr : it->second.c_str()))
            return fail(SSAMD_EINVAL, "unknown option %s", name);
    }
    if (std::string(name) == "SSAMD_AUTOTUNE")
        g_autotune.store(g_tuning.autotune_env != -2 ? g_tuning.autotune_env : -1);
    g_tune_version.fetch_add(1, std::memory_order_release);
    return SSAMD_OK;
}

int ssamd_counter(int device, const char *name, long long *value)
{
    if (!name || !value) return fail(SSAMD_EINVAL, "name / value is NULL");
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    const std::string n(name);
    if (n == "evol_fallbacks") *value = c->evol_fallbacks;
    else if (n == "evol_bytes") *value = (long long)c->evol.cap;
    else if (n == "tail_splits") *value = c->tail_splits;
    else if (n == "exact_calls") *value = c->exact_calls;
    else if (n == "pipe_persist_launches") *value = c->persist_launches;
    else if (n == "pipe_persist_items") {
        // tiles finished by persistent phase-shifted launches on this device so far (counted on the device, once per finished item)
        unsigned long long done = 0;
        if (c->pq.ptr) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(&done, (const unsigned int *)c->pq.ptr + ASW_PQ_QUEUES * ASW_PQ_LINE, sizeof(done), hipMemcpyDeviceToHost));
        }
        *value = (long long)done;
    }
    else if (n == "exact_entries" || n == "exact_flagged_left" || n == "exact_flagged_right" || n == "exact_overflow" || n == "exact_raw_entries") {
        // of the LAST exact call on this device: candidates re-evaluated in fp64, pixels with near-ties, whether the queue overflowed
        unsigned int ctr[5] = {0, 0, 0, 0, 0};
        if (c->xflags.ptr && c->exact_calls > 0) {       // (the counters are the first 64 bytes of the flag buffer: one memset per call)
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(ctr, c->xflags.ptr, sizeof(ctr), hipMemcpyDeviceToHost));
        }
        *value = n == "exact_entries" ? ctr[0] : n == "exact_flagged_left" ? ctr[1] : n == "exact_flagged_right" ? ctr[2] :
                 n == "exact_raw_entries" ? ctr[4] : ((ctr[0] > c->xcap || (c->xrawcap && ctr[4] > c->xrawcap)) ? 1 : 0);
    }
    else return fail(SSAMD_EINVAL, "unknown counter %s", name);
    return SSAMD_OK;
}

int ssamd_autotune(int on)
{
    return g_autotune.exchange(on > 0 ? 1 : (on < 0 ? -1 : 0));
}

int ssamd_asw_geometry(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    const Tuning &t = tune();
    const PlanOptions po{t, false};
    AswGeom g;
    if ((rc = asw_choose_geometry(g, po, width, rows, winSize, nD))) return rc;
    out[0] = g.Tx; out[1] = g.Dc; out[2] = g.nchunks; out[3] = g.threads; out[4] = g.lds_bytes;
    out[5] = (width + g.Tx - 1) / g.Tx; out[6] = rows; out[7] = g.nchunks;
    AswWaveGeom wg;
    if (g.wave_rx && asw_wave_layout(wg, po, winSize, nD, g.wave_rx, t.wave_unroll != 0)) {      // a "tile" = the four strips of a workgroup's waves (LDS of the plain call: no cost dump)
        out[0] = wg.Txw * wg.waves; out[1] = wg.Dc; out[2] = 1; out[3] = 64 * wg.waves; out[4] = wg.wave_lds * wg.waves;
        out[5] = (width + out[0] - 1) / out[0]; out[7] = 1;
    }
    return SSAMD_OK;
}

int ssamd_asw_kernel_form(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    const Tuning &t = tune();
    AswGeom g;
    if ((rc = asw_choose_geometry(g, PlanOptions{t, false}, width, rows, winSize, nD))) return rc;
    out[0] = g.pipe; out[1] = g.Rx; out[2] = g.JC >= winSize ? 0 : g.JC; out[3] = g.pipe ? g.dephase : 0;
    out[4] = g.wave_rx & 15;
    if (g.wave_rx) { out[0] = 0; out[1] = g.wave_rx & 15; out[2] = 0; out[3] = 0; }
    return SSAMD_OK;
}

int ssamd_gsw_geometry(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    GswGeom g;
    if ((rc = gsw_choose_geometry(g, tune(), width, rows, winSize, nD))) return rc;
    out[0] = g.Tx; out[1] = g.Dc; out[2] = g.nchunks; out[3] = g.threads * g.Hy; out[4] = g.lds_bytes;
    out[5] = (width + g.Tx - 1) / g.Tx; out[6] = (rows + g.Ty * g.Hy - 1) / (g.Ty * g.Hy); out[7] = g.nchunks; out[8] = g.Ty * g.Hy;
    return SSAMD_OK;
}

// An ASW entry point and its _exact twin (the fp64 tie-break pass on top): one parameter list, one body, `exact` the only difference.
#define SSAMD_ASW_TWINS(SUFFIX, PARAMS, BODY)                                   \
    int ssamd_asw##SUFFIX PARAMS { const bool exact = false; return BODY; }     \
    int ssamd_asw_exact##SUFFIX PARAMS { const bool exact = true; return BODY; }

SSAMD_ASW_TWINS(_device, (const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows, int winSize,
                          int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent, int16_t *d_disparity, void *stream),
                asw_device_entry(nullptr, d_img1, d_img2, height, width, out_row0, out_rows, 0, 0, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                 consistent, d_disparity, stream, exact))

SSAMD_ASW_TWINS(_device_rows2, (const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows, int skip_row0,
                                int skip_rows, int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                                int16_t *d_disparity, void *stream),
                asw_device_entry(nullptr, d_img1, d_img2, height, width, out_row0, out_rows, skip_row0, skip_rows, winSize, maxDisparity, minDisparity,
                                 gammaC, gammaP, consistent, d_disparity, stream, exact))

SSAMD_ASW_TWINS(_rectified_device, (const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                                    const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int height, int width, int interpolation,
                                    int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                                    int16_t *d_disparity, void *stream),
                asw_rectified_entry(d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, height, width, interpolation,
                                    winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent, d_disparity, stream, exact))
#undef SSAMD_ASW_TWINS

int ssamd_asw_alternate_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int winSize,
                               int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                               int16_t *d_disparity, void *stream)
{
    return asw_device_entry(nullptr, d_img1, d_img2, height, width, 0, height, 0, 0, winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent,
                            d_disparity, stream, false, true);
}

int ssamd_asw_alternate_rows_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                                    int row_parity, int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP,
                                    int consistent, int16_t *d_disparity, void *stream)
{
    if (!d_img1 || !d_img2 || !d_disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    if (row_parity != 0 && row_parity != 1) return fail(SSAMD_EINVAL, "row_parity must be 0 or 1");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    AswCall q;
    q.dL = d_img1; q.dR = d_img2; q.H = height; q.W = width; q.row0 = out_row0; q.rows = out_rows;
    q.win = winSize; q.maxD = maxDisparity; q.minD = minDisparity; q.gammaC = gammaC; q.gammaP = gammaP; q.consistent = consistent != 0;
    q.d_disp = d_disparity; q.s = (hipStream_t)stream;
    return asw_alternate_rows(*c, q, row_parity);
}

// The matcher on host arrays, on one device or as row strips on several (rows are independent jobs and the tie-break pass is
// row-local: each strip runs its own): plain, exact, alternate rows
#define SSAMD_ASW_HOST(NAME, ALTERNATE, EXACT)                                                                                              \
    int NAME(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity, int minDisparity,             \
             double gammaC, double gammaP, int consistent, int16_t *disparity, int device)                                                 \
    {                                                                                                                                      \
        if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");                                                        \
        return host_rows(asw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent, disparity,    \
                                 nullptr, ALTERNATE, EXACT), device);                                                                      \
    }                                                                                                                                      \
    int NAME##_multi(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity, int minDisparity,     \
                     double gammaC, double gammaP, int consistent, int16_t *disparity, const int *devices, int n_devices)                  \
    {                                                                                                                                      \
        if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");                                                        \
        return run_strips(asw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent, disparity,   \
                                  nullptr, ALTERNATE, EXACT), devices, n_devices);                                                         \
    }
SSAMD_ASW_HOST(ssamd_asw, false, false)
SSAMD_ASW_HOST(ssamd_asw_exact, false, true)
SSAMD_ASW_HOST(ssamd_asw_alternate, true, false)
#undef SSAMD_ASW_HOST

int ssamd_asw_costs(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                    int minDisparity, double gammaC, double gammaP, float *costs, int device)
{
    if (!img1 || !img2 || !costs) return fail(SSAMD_EINVAL, "NULL buffer");
    if (maxDisparity < minDisparity) return fail(SSAMD_EINVAL, "empty disparity range");
    return host_rows(asw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gammaC, gammaP, 0, nullptr,
                                 costs, false), device);
}

int ssamd_asw_argmins(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                      int minDisparity, double gammaC, double gammaP, int16_t *left_disparity, int16_t *right_match,
                      int device)
{
    if (!img1 || !img2 || !left_disparity || !right_match) return fail(SSAMD_EINVAL, "NULL buffer");
    if (maxDisparity < minDisparity) return fail(SSAMD_EINVAL, "empty disparity range");
    HostJob j = asw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gammaC, gammaP, 1, left_disparity,
                        nullptr, false);
    j.raw_right = right_match;
    return host_rows(j, device);
}

int ssamd_bgr2lab(const uint8_t *img, int height, int width, float *lab, int device)
{
    if (!img || !lab || height <= 0 || width <= 0) return fail(SSAMD_EINVAL, "bad argument");
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    const size_t npix = (size_t)height * width;
    if ((rc = c->imgL.reserve(npix * 3)) || (rc = c->lab.reserve(npix * 12))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, img, npix * 3, hipMemcpyHostToDevice, s));
    const int blocks = (int)std::min<size_t>((npix + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(bgr2lab_f32_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t *)c->imgL.ptr,
                       (float *)c->lab.ptr, (long long)npix);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lab, c->lab.ptr, npix * 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

// Verification: the fp64 costs the tie-break pass computes for n given candidates (y, x, d triples), and optionally the fp64 Lab
// images it reads -- to compare with the oracle's fp64 costs bit for bit.
int ssamd_debug_exact_costs(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, double gammaC, double gammaP,
                            int n, const int *yxd, double *costs, double *lab1, double *lab2)
{
    if (!img1 || !img2 || !yxd || !costs || n < 0) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = check_common(height, width, winSize, 0, 0, 0, height);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    const size_t npix = (size_t)height * width;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    if ((rc = c->imgL.reserve(npix * 3)) || (rc = c->imgR.reserve(npix * 3)) || (rc = c->recL.reserve(npix * sizeof(PixRec))) ||
        (rc = c->recR.reserve(npix * sizeof(PixRec))) || (rc = c->xlabL.reserve(npix * 24)) || (rc = c->xlabR.reserve(npix * 24)) ||
        (rc = c->xqueue.reserve((size_t)std::max(n, 1) * 8)) || (rc = c->xcost.reserve((size_t)std::max(n, 1) * 8)) || (rc = c->xctr.reserve(64)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, img1, npix * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->imgR.ptr, img2, npix * 3, hipMemcpyHostToDevice, s));
    const int blocks = (int)std::min<long long>((2 * (long long)npix + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(bgr2lab_records_pair_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t *)c->imgL.ptr, (const uint8_t *)c->imgR.ptr,
                       (PixRec *)c->recL.ptr, (PixRec *)c->recR.ptr, (long long)npix);
    hipLaunchKernelGGL(bgr2lab_f64_pair_kernel, dim3(blocks), dim3(256), 0, s, (const PixRec *)c->recL.ptr, (const PixRec *)c->recR.ptr,
                       (double *)c->xlabL.ptr, (double *)c->xlabR.ptr, (long long)npix);
    std::vector<u64> ent((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int y = yxd[3 * k], x = yxd[3 * k + 1], d = yxd[3 * k + 2];
        if (y < 0 || y >= height || x < 0 || x >= width || d < 0 || x - d < 0) return fail(SSAMD_EINVAL, "candidate %d outside the image", k);
        ent[k] = (u64)((uint32_t)y * (uint32_t)width + (uint32_t)x) | ((u64)(uint32_t)d << 32);       // sides = 0: cost only
    }
    const unsigned int ctr[16] = {(unsigned int)n};            // (counter[7] = the eval kernel's work counter)
    HIP_TRY(hipMemcpyAsync(c->xqueue.ptr, ent.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->xctr.ptr, ctr, sizeof(ctr), hipMemcpyHostToDevice, s));
    const double *d_prox = nullptr;
    if ((rc = get_prox64(*c, winSize, gammaP, s, &d_prox))) return rc;
    AswExactArgs x{};
    x.recL = (const PixRec *)c->recL.ptr; x.recR = (const PixRec *)c->recR.ptr;
    x.labL = (const double *)c->xlabL.ptr; x.labR = (const double *)c->xlabR.ptr;
    x.prox = d_prox; x.q.entries = (u64 *)c->xqueue.ptr; x.q.counter = (unsigned int *)c->xctr.ptr; x.q.cap = (unsigned int)std::max(n, 1);
    x.ecost = (double *)c->xcost.ptr;
    x.H = height; x.W = width; x.win = winSize; x.pad = winSize / 2; x.row0 = 0; x.rows = height; x.gammaC = gammaC;
    hipLaunchKernelGGL(asw_exact_eval_kernel, dim3(256), dim3(64 * EXACT_WAVES), 0, s, x);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(costs, c->xcost.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (lab1) HIP_TRY(hipMemcpyAsync(lab1, c->xlabL.ptr, npix * 24, hipMemcpyDeviceToHost, s));
    if (lab2) HIP_TRY(hipMemcpyAsync(lab2, c->xlabR.ptr, npix * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

int ssamd_gsw_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                     int winSize, int maxDisparity, int minDisparity, int gamma, float fMax, int iterations, int bins,
                     int16_t *d_disparity, void *stream)
{
    return ssamd_gsw_device_rows2(d_img1, d_img2, height, width, out_row0, out_rows, 0, 0, winSize, maxDisparity, minDisparity, gamma, fMax,
                                  iterations, bins, d_disparity, stream);
}

// ssamd_gsw_device on TWO row ranges (round 6: the border bands of a row strip whose interior rows ran while the halo was in flight,
// strips.py).  GSW workgroups are small (two 8-wave groups per CU, strips of 2-8 rows) and a band is winSize/2 = 5 rows at the class
// default: each band is an ordinary call on its rows -- pack, both passes, left-right check -- written at its place in d_disparity.
int ssamd_gsw_device_rows2(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                           int skip_row0, int skip_rows, int winSize, int maxDisparity, int minDisparity, int gamma, float fMax,
                           int iterations, int bins, int16_t *d_disparity, void *stream)
{
    (void)bins;                       // never read by the reference either (_passive.cpp:410)
    if (!d_img1 || !d_img2 || !d_disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    if (skip_rows < 0 || (skip_rows > 0 && (skip_row0 < out_row0 || skip_row0 + skip_rows > out_row0 + out_rows)))
        return fail(SSAMD_EINVAL, "the skipped rows [%d,%d) must lie inside the output rows [%d,%d)", skip_row0, skip_row0 + skip_rows,
                    out_row0, out_row0 + out_rows);
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    if (skip_rows == 0)
        return gsw_device_impl(*c, d_img1, d_img2, height, width, out_row0, out_rows, winSize, maxDisparity, minDisparity,
                               gamma, fMax, iterations, d_disparity, (hipStream_t)stream);
    if ((rc = check_common(height, width, winSize, minDisparity, maxDisparity, out_row0, out_rows))) return rc;
    const int bot0 = skip_row0 + skip_rows, band0[2] = {out_row0, bot0}, band_rows[2] = {skip_row0 - out_row0, out_row0 + out_rows - bot0};
    for (int k = 0; k < 2; ++k)
        if (band_rows[k] > 0 && (rc = gsw_device_impl(*c, d_img1, d_img2, height, width, band0[k], band_rows[k], winSize, maxDisparity, minDisparity, gamma, fMax,
                                                      iterations, d_disparity + (size_t)(band0[k] - out_row0) * width, (hipStream_t)stream)))
            return rc;
    return SSAMD_OK;
}

int ssamd_gsw_rectified_device(const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width,
                               const float *d_mapx1, const float *d_mapy1, const float *d_mapx2, const float *d_mapy2,
                               int height, int width, int interpolation, int winSize, int maxDisparity, int minDisparity,
                               int gamma, float fMax, int iterations, int bins, int16_t *d_disparity, void *stream)
{
    (void)bins;
    RemapSrc rm;
    int rc = make_remap_src(rm, d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, interpolation, d_disparity);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return gsw_device_impl(*c, nullptr, nullptr, height, width, 0, height, winSize, maxDisparity, minDisparity, gamma, fMax, iterations,
                           d_disparity, (hipStream_t)stream, &rm);
}

int ssamd_gsw(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
              int minDisparity, int gamma, float fMax, int iterations, int bins, int16_t *disparity, int device)
{
    (void)bins;
    if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    return host_rows(gsw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations,
                                 disparity), device);
}

int ssamd_gsw_multi(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                    int minDisparity, int gamma, float fMax, int iterations, int bins, int16_t *disparity,
                    const int *devices, int n_devices)
{
    (void)bins;
    if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    return run_strips(gsw_job(img1, img2, height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations,
                              disparity), devices, n_devices);
}

int ssamd_remap_bgr_device(const uint8_t *d_src, int src_h, int src_w, const float *d_mapx, const float *d_mapy,
                           int dst_h, int dst_w, int interpolation, uint8_t *d_dst, void *stream)
{
    if (!d_src || !d_mapx || !d_mapy || !d_dst) return fail(SSAMD_EINVAL, "NULL buffer");
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (interpolation != 0 && interpolation != 1) return fail(SSAMD_EINVAL, "only INTER_NEAREST (0) and INTER_LINEAR (1) are supported");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)dst_h * dst_w;
    // (a thread owns four output pixels; the map and output pointers are 16- / 4-byte aligned: device allocations)
    if (((uintptr_t)d_mapx | (uintptr_t)d_mapy) & 15 || ((uintptr_t)d_dst & 3)) return fail(SSAMD_EINVAL, "maps must be 16-byte and the output 4-byte aligned");
    const int blocks = (int)std::min<long long>((npix / 4 + 255) / 256 + 1, 256 * 16);
    Timed t(*c, s, SSAMD_K_REMAP);
    hipLaunchKernelGGL(remap_bgr_kernel, dim3(blocks), dim3(256), 0, s, d_src, src_h, src_w, d_mapx, d_mapy, d_dst, npix,
                       interpolation == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int ssamd_reproject_device(const int16_t *d_disparity, int h, int w, const double *Q, float *d_points, void *stream)
{
    if (!d_disparity || !Q || !d_points) return fail(SSAMD_EINVAL, "NULL buffer");
    if (h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    Mat4 q;
    for (int k = 0; k < 16; ++k) q.m[k] = Q[k];
    if (h > 65535) return fail(SSAMD_ELIMIT, "more than 65535 rows");
    if ((w & 3) == 0 && (((uintptr_t)d_disparity & 7) || ((uintptr_t)d_points & 15)))
        return fail(SSAMD_EINVAL, "disparity / point buffers must be 8- / 16-byte aligned");
    const int per_row = (w & 3) == 0 ? w / 4 : w;                 // threads a row needs
    Timed t(*c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(reproject_kernel, dim3((per_row + 255) / 256, h), dim3(256), 0, s, d_disparity, d_points, h, w, q);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

}  // extern "C"

namespace {
// _unwrapping.infiniteImpulseResponse's checks (_unwrapping.cpp:63-74) on n [h][w] maps, plus the kernel's own limits
int unwrap_check(int n, int h, int w, double tau)
{
    if (n < 0 || h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    if (tau < 0 || tau > 1) return fail(SSAMD_EINVAL, "Wrong tau value!");                   // NaN passes, as in the reference
    if (w > UNWRAP_MAX_W) return fail(SSAMD_ELIMIT, "phase maps wider than %d columns are not supported (width %d)", UNWRAP_MAX_W, w);
    if ((long long)h * w > (1ll << 40)) return fail(SSAMD_ELIMIT, "phase map of %d x %d pixels too large", h, w);
    return SSAMD_OK;
}

// One workgroup per map.  Bands as few as the row cap allows, their heights as even as whole waves make them: the step count,
// bands * w + 2 (h - bands), depends on the number of bands only, and fewer waves per workgroup share the CU's SIMDs.
int unwrap_launch(Ctx &c, const double *d_phase, int n, int h, int w, double tau, double *d_out, hipStream_t s)
{
    if (n == 0) return SSAMD_OK;
    const int cap = tune().unwrap_rows > 0 ? round_up(tune().unwrap_rows, 64) : UNWRAP_MAX_ROWS;
    const int bands = (h + cap - 1) / cap;
    const int R = round_up((h + bands - 1) / bands, 64);
    const int lds = (w + 2 * R) * (int)sizeof(double);
    int rc = grant_dyn_lds(c, reinterpret_cast<const void *>(&iir_unwrap_kernel), lds);
    if (rc) return rc;
    Timed t(c, s, SSAMD_K_UNWRAP);
    hipLaunchKernelGGL(iir_unwrap_kernel, dim3(n), dim3(R), lds, s, d_phase, d_out, h, w, tau);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {

int ssamd_iir_unwrap(const double *phase, int n, int h, int w, double tau, double *out, int device)
{
    if (!phase || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = unwrap_check(n, h, w, tau);
    if (rc) return rc;
    if (n == 0) return SSAMD_OK;
    CtxLock c;
    if ((rc = get_ctx(device, c))) return rc;
    const size_t bytes = (size_t)n * h * w * sizeof(double);
    if ((rc = c->uwIn.reserve(bytes)) || (rc = c->uwOut.reserve(bytes))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    HIP_TRY(hipMemcpyAsync(c->uwIn.ptr, phase, bytes, hipMemcpyHostToDevice, s));
    if ((rc = unwrap_launch(*c, (const double *)c->uwIn.ptr, n, h, w, tau, (double *)c->uwOut.ptr, s))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->uwOut.ptr, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

int ssamd_iir_unwrap_device(const double *d_phase, int n, int h, int w, double tau, double *d_out, void *stream)
{
    if (!d_phase || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = unwrap_check(n, h, w, tau);
    if (rc) return rc;
    if (n == 0) return SSAMD_OK;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return unwrap_launch(*c, d_phase, n, h, w, tau, d_out, (hipStream_t)stream);
}

namespace {
// np.unwrap on the geometry [outer][len][inner] (np_unwrap_plan.h): the checks shared by the host and the device entry points
int npu_check(long long outer, long long len, long long inner, double period, NpuPlan &plan)
{
    if (!(period > 0) || !std::isfinite(period)) return fail(SSAMD_EINVAL, "period must be a finite positive number");
    switch (npu_plan(outer, len, inner, plan)) {
    case NPU_OK: return SSAMD_OK;
    case NPU_NEGATIVE: return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    case NPU_TOO_MANY_ELEMS: return fail(SSAMD_ELIMIT, "more than 2^40 phase samples (%lld x %lld x %lld)", outer, len, inner);
    default:
        return fail(SSAMD_ELIMIT, "more than %lld %s to scan (%lld x %lld): one launch holds fewer than 2^32 threads",
                    NPU_MAX_LAUNCH_THREADS / plan.threads, plan.form == 0 ? "lines" : "groups of 16 columns", outer, inner);
    }
}

// one scan; d_out may be d_p (the kernels work in place)
int npu_launch(Ctx &c, const NpuPlan &plan, const double *d_p, long long len, long long inner, double discont, double period,
               double *d_out, hipStream_t s)
{
    if (plan.blocks == 0) return SSAMD_OK;
    const double hi = period / 2, lo = -hi;
    Timed t(c, s, SSAMD_K_NPUNWRAP);
    if (plan.form == 0)
        hipLaunchKernelGGL(np_unwrap_row_kernel, dim3((unsigned)plan.blocks), dim3(plan.threads), 0, s, d_p, d_out, len, discont, period,
                           hi, lo);
    else
        hipLaunchKernelGGL(np_unwrap_col_kernel, dim3((unsigned)plan.blocks), dim3(plan.threads), 0, s, d_p, d_out, len, inner,
                           plan.groups, discont, period, hi, lo);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// the reference's default composition (active.py:739-745) on n maps [h][w]: along x (axis 1), then along y (axis 0), discont = pi
struct NpuXY { NpuPlan x, y; };
int npu_xy_check(int n, int h, int w, NpuXY &q)
{
    if (n < 0 || h < 0 || w < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    int rc = npu_check((long long)n * h, w, 1, 2 * M_PI, q.x);
    return rc ? rc : npu_check(n, h, w, 2 * M_PI, q.y);
}
int npu_xy_launch(Ctx &c, const NpuXY &q, const double *d_p, int h, int w, double *d_out, hipStream_t s)
{
    int rc = npu_launch(c, q.x, d_p, w, 1, M_PI, 2 * M_PI, d_out, s);
    return rc ? rc : npu_launch(c, q.y, d_out, h, w, M_PI, 2 * M_PI, d_out, s);
}

// host buffers through the unwrapper's staging pair
extern "C++" {
template <class Launch>      // int launch(Ctx &, const double *d_p, double *d_out, hipStream_t)
int npu_host(const double *p, double *out, size_t count, int device, Launch launch)
{
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    const size_t bytes = count * sizeof(double);
    if ((rc = c->uwIn.reserve(bytes)) || (rc = c->uwOut.reserve(bytes))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    HIP_TRY(hipMemcpyAsync(c->uwIn.ptr, p, bytes, hipMemcpyHostToDevice, s));
    if ((rc = launch(*c, (const double *)c->uwIn.ptr, (double *)c->uwOut.ptr, s))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->uwOut.ptr, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}
}  // extern "C++"
}  // namespace

int ssamd_np_unwrap_plan(long long outer, long long len, long long inner, int32_t *plan)
{
    if (!plan) return fail(SSAMD_EINVAL, "NULL buffer");
    NpuPlan q;
    int rc = npu_check(outer, len, inner, 1.0, q);
    if (rc) return rc;
    const int32_t v[8] = {q.form, q.chunk, q.lanes, q.threads, (int32_t)q.blocks, q.lds_bytes, q.per_thread, (int32_t)q.groups};
    std::copy(v, v + 8, plan);
    return SSAMD_OK;
}

int ssamd_np_unwrap(const double *p, long long outer, long long len, long long inner, double discont, double period, double *out,
                    int device)
{
    NpuPlan q;
    int rc = npu_check(outer, len, inner, period, q);
    if (rc || q.blocks == 0) return rc;
    if (!p || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    return npu_host(p, out, (size_t)outer * len * inner, device, [&](Ctx &c, const double *d_p, double *d_out, hipStream_t s) {
        return npu_launch(c, q, d_p, len, inner, discont, period, d_out, s);
    });
}

int ssamd_np_unwrap_device(const double *d_p, long long outer, long long len, long long inner, double discont, double period,
                           double *d_out, void *stream)
{
    NpuPlan q;
    int rc = npu_check(outer, len, inner, period, q);
    if (rc || q.blocks == 0) return rc;
    if (!d_p || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return npu_launch(*c, q, d_p, len, inner, discont, period, d_out, (hipStream_t)stream);
}

int ssamd_np_unwrap_xy(const double *p, int n, int h, int w, double *out, int device)
{
    NpuXY q;
    int rc = npu_xy_check(n, h, w, q);
    if (rc || q.y.blocks == 0) return rc;
    if (!p || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    return npu_host(p, out, (size_t)n * h * w, device, [&](Ctx &c, const double *d_p, double *d_out, hipStream_t s) {
        return npu_xy_launch(c, q, d_p, h, w, d_out, s);
    });
}

int ssamd_np_unwrap_xy_device(const double *d_p, int n, int h, int w, double *d_out, void *stream)
{
    NpuXY q;
    int rc = npu_xy_check(n, h, w, q);
    if (rc || q.y.blocks == 0) return rc;
    if (!d_p || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return npu_xy_launch(*c, q, d_p, h, w, d_out, (hipStream_t)stream);
}

namespace {
// band planning, table and launches of ssamd_ftp_phase*; the caller holds the context and has ordered the scratch (ScratchOrder)
static_assert(FTP_MAX_W == SSAMD_FTP_MAX_W, "ssamd.h states the width limit of ftp_plan.h");
int ftp_check(int ch_obj, int ch_ref, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau)
{
    if (h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if ((ch_obj != 1 && ch_obj != 3) || (ch_ref != 1 && ch_ref != 3)) return fail(SSAMD_EINVAL, "images must have 1 or 3 channels");
    if (!fmin || !fmax) return fail(SSAMD_EINVAL, "NULL band bounds");
    if (unwrap < 0 || unwrap > 2) return fail(SSAMD_EINVAL, "unwrap must be 0, 1 or 2");
    if (w > FTP_MAX_W) return fail(SSAMD_ELIMIT, "rows wider than %d columns are not supported (width %d)", FTP_MAX_W, w);
    if (unwrap == 2) {                                   // tau is not read
        NpuXY q;
        return npu_xy_check(1, h, w, q);
    }
    return unwrap == 1 ? unwrap_check(1, h, w, tau) : SSAMD_OK;
}

int ftp_twiddles(Ctx &c, int w, hipStream_t s, const double2 **tw)
{
    auto it = c.ftpTabs.find(w);
    if (it == c.ftpTabs.end()) {
        if (c.ftpTabs.size() >= 16) {                    // hipFree waits for the kernels that may still read a table
            for (auto &e : c.ftpTabs) e.second.release();
            c.ftpTabs.clear();
        }
        DevBuf buf;
        int rc = buf.reserve((size_t)w * sizeof(double2));
        if (rc) return rc;
        hipLaunchKernelGGL(ftp_twiddle_kernel, dim3((w + 255) / 256), dim3(256), 0, s, (double2 *)buf.ptr, w);
        HIP_TRY(hipGetLastError());
        it = c.ftpTabs.emplace(w, buf).first;
    }
    *tw = (const double2 *)it->second.ptr;
    return SSAMD_OK;
}

int ftp_launch(Ctx &c, const uint8_t *d_obj, int ch_obj, const uint8_t *d_ref, int ch_ref, int h, int w, const double *fmin,
               const double *fmax, int unwrap, double tau, double *d_out, hipStream_t s)
{
    int rc;
    // the bands go through pinned staging that the previous call's upload may still be reading
    if (!c.ftp_band_copied) HIP_TRY(hipEventCreateWithFlags(&c.ftp_band_copied, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(c.ftp_band_copied));
    if ((size_t)h > c.ftpBandHostCap) {
        if (c.ftpBandHost) { (void)hipHostFree(c.ftpBandHost); c.ftpBandHost = nullptr; c.ftpBandHostCap = 0; }
        const size_t want = (size_t)h + (size_t)h / 8 + 64;
        HIP_TRY(hipHostMalloc((void **)&c.ftpBandHost, want * 2 * sizeof(int32_t), hipHostMallocDefault));
        c.ftpBandHostCap = want;
    }
    int max_bins = 0;
    for (int y = 0; y < h; ++y) {
        int32_t lo, hi;
        ftp_band_row(w, fmin[y], fmax[y], lo, hi);
        c.ftpBandHost[2 * (size_t)y] = lo;
        c.ftpBandHost[2 * (size_t)y + 1] = hi;
        max_bins = std::max(max_bins, hi - lo + 1);
    }
    if ((rc = c.ftpBand.reserve((size_t)h * 2 * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(c.ftpBand.ptr, c.ftpBandHost, (size_t)h * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.ftp_band_copied, s));
    const double2 *tw = nullptr;
    if ((rc = ftp_twiddles(c, w, s, &tw))) return rc;
    double *d_phase = d_out;
    if (unwrap == 1) {                                   // the wavefront kernel does not work in place
        if ((rc = c.ftpPhase.reserve((size_t)h * w * sizeof(double)))) return rc;
        d_phase = (double *)c.ftpPhase.ptr;
    }
    const FtpGeom g = ftp_geometry(w);
    const int q = ftp_lanes_per_bin(g.threads, std::max(max_bins, 1));
    auto launch = [&](auto kernel) -> int {
        int r = grant_dyn_lds(c, reinterpret_cast<const void *>(kernel), g.lds_bytes);
        if (r) return r;
        Timed t(c, s, SSAMD_K_FTP);
        hipLaunchKernelGGL(kernel, dim3(h), dim3(g.threads), g.lds_bytes, s, d_obj, ch_obj, d_ref, ch_ref, w,
                           (const int2 *)c.ftpBand.ptr, tw, q, FTP_BIN_CHUNK, d_phase);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    };
    switch (g.cpt) {
    case 1: rc = launch(&ftp_phase_kernel<1>); break;
    case 2: rc = launch(&ftp_phase_kernel<2>); break;
    case 4: rc = launch(&ftp_phase_kernel<4>); break;
    default: rc = launch(&ftp_phase_kernel<8>); break;
    }
    if (rc) return rc;
    if (unwrap == 2) {
        NpuXY q;
        if ((rc = npu_xy_check(1, h, w, q))) return rc;  // cannot fail: ftp_check has asked before anything was enqueued
        return npu_xy_launch(c, q, d_out, h, w, d_out, s);
    }
    return unwrap ? unwrap_launch(c, d_phase, 1, h, w, tau, d_out, s) : SSAMD_OK;
}
}  // namespace

int ssamd_ftp_band(int w, int h, const double *fmin, const double *fmax, int32_t *slo, int32_t *shi)
{
    if (w <= 0 || h < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (h > 0 && (!fmin || !fmax || !slo || !shi)) return fail(SSAMD_EINVAL, "NULL buffer");
    for (int y = 0; y < h; ++y) ftp_band_row(w, fmin[y], fmax[y], slo[y], shi[y]);
    return SSAMD_OK;
}

int ssamd_ftp_phase(const uint8_t *img_obj, int ch_obj, const uint8_t *img_ref, int ch_ref, int h, int w, const double *fmin,
                    const double *fmax, int unwrap, double tau, double *out, int device)
{
    if (!img_obj || !img_ref || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch_obj, ch_ref, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(device, c))) return rc;
    const size_t px = (size_t)h * w, bytes = px * sizeof(double);
    if ((rc = c->imgL.reserve(px * ch_obj)) || (rc = c->imgR.reserve(px * ch_ref)) || (rc = c->uwOut.reserve(bytes))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, img_obj, px * ch_obj, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->imgR.ptr, img_ref, px * ch_ref, hipMemcpyHostToDevice, s));
    if ((rc = ftp_launch(*c, (const uint8_t *)c->imgL.ptr, ch_obj, (const uint8_t *)c->imgR.ptr, ch_ref, h, w, fmin, fmax, unwrap, tau,
                         (double *)c->uwOut.ptr, s)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, c->uwOut.ptr, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

int ssamd_ftp_phase_device(const uint8_t *d_img_obj, int ch_obj, const uint8_t *d_img_ref, int ch_ref, int h, int w,
                           const double *fmin, const double *fmax, int unwrap, double tau, double *d_out, void *stream)
{
    if (!d_img_obj || !d_img_ref || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch_obj, ch_ref, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    ScratchOrder order(*c, (hipStream_t)stream);        // the band, the table and the wrapped map are the context's
    return ftp_launch(*c, d_img_obj, ch_obj, d_img_ref, ch_ref, h, w, fmin, fmax, unwrap, tau, d_out, (hipStream_t)stream);
}

namespace {
// FTP phase -> cloud (ftp_cloud_kernels.hip.h): the checks shared by the host and the device entry point; fills the by-value
// geometry, the phase shift of the fringe order and the distortion model the coefficients ask for
static_assert(SSAMD_FTP_CLOUD_NGEOM * sizeof(double) == sizeof(FtpCloudGeom), "geom layout of ssamd.h");
int ftp_cloud_check(int h, int w, int x0, int y0, const double *geom, double k, FtpCloudGeom &G, double &kshift, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions or origin!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "phase map of %d x %d pixels: 2^31 or more", h, w);
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    if (!std::isfinite(k)) return fail(SSAMD_EINVAL, "the fringe order k must be finite");
    for (int i = 0; i < SSAMD_FTP_CLOUD_NGEOM; ++i)
        if (!std::isfinite(geom[i])) return fail(SSAMD_EINVAL, "geom[%d] is not finite", i);
    std::memcpy(&G, geom, sizeof(G));
    kshift = (k * 2.0) * M_PI;                       // active.py:791: k * 2 * np.pi
    auto any = [&](int a, int b) { for (int i = a; i < b; ++i) if (G.d[i] != 0) return true; return false; };
    model = any(8, 12) ? 3 : any(5, 8) ? 2 : any(0, 5) ? 1 : 0;
    return SSAMD_OK;
}

int ftp_cloud_launch(Ctx &c, const double *d_phase, int h, int w, int x0, int y0, const FtpCloudGeom &G, double kshift, int model,
                     double *d_out, hipStream_t s)
{
    if (((uintptr_t)d_phase | (uintptr_t)d_out) & 15) return fail(SSAMD_EINVAL, "phase and point buffers must be 16-byte aligned");
    const long long npix = (long long)h * w, pairs = (npix + 1) / 2;
    const int blocks = (int)std::min<long long>((pairs + FTP_CLOUD_THREADS - 1) / FTP_CLOUD_THREADS, (long long)c.cus * 8);
    Timed t(c, s, SSAMD_K_REPROJECT);
    switch (model) {
    case 0: hipLaunchKernelGGL(ftp_cloud_kernel<0>, dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, kshift, G); break;
    case 1: hipLaunchKernelGGL(ftp_cloud_kernel<1>, dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, kshift, G); break;
    case 2: hipLaunchKernelGGL(ftp_cloud_kernel<2>, dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, kshift, G); break;
    default: hipLaunchKernelGGL(ftp_cloud_kernel<3>, dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, kshift, G); break;
    }
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

int ssamd_ftp_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, double k, double *out, int device)
{
    FtpCloudGeom G;
    double kshift;
    int model;
    int rc = ftp_cloud_check(h, w, x0, y0, geom, k, G, kshift, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!phase || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(device, c))) return rc;
    const size_t bytes = (size_t)h * w * sizeof(double);
    if ((rc = c->uwIn.reserve(bytes)) || (rc = c->uwOut.reserve(3 * bytes))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    HIP_TRY(hipMemcpyAsync(c->uwIn.ptr, phase, bytes, hipMemcpyHostToDevice, s));
    if ((rc = ftp_cloud_launch(*c, (const double *)c->uwIn.ptr, h, w, x0, y0, G, kshift, model, (double *)c->uwOut.ptr, s))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->uwOut.ptr, 3 * bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

int ssamd_ftp_cloud_device(const double *d_phase, int h, int w, int x0, int y0, const double *geom, double k, double *d_out, void *stream)
{
    FtpCloudGeom G;
    double kshift;
    int model;
    int rc = ftp_cloud_check(h, w, x0, y0, geom, k, G, kshift, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!d_phase || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return ftp_cloud_launch(*c, d_phase, h, w, x0, y0, G, kshift, model, d_out, (hipStream_t)stream);      // no scratch: nothing to order
}

namespace {
__global__ void debug_libm_kernel(int which, int n, const void *in, void *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (which == 0) reinterpret_cast<double *>(out)[i] = glibc_exp(reinterpret_cast<const double *>(in)[i]);
    else if (which == 1) reinterpret_cast<float *>(out)[i] = glibc_powf_pos(reinterpret_cast<const float *>(in)[i], (float)(1 / 3.0));
    else if (which == 2) reinterpret_cast<double *>(out)[i] = ssamd::exact_sqrt(reinterpret_cast<const double *>(in)[i]);
    else reinterpret_cast<double *>(out)[i] = reinterpret_cast<const double *>(in)[i] / 0.7 + reinterpret_cast<const double *>(in)[i] / 5.0;
}
}  // namespace

// Verification / diagnosis: the queues of the LAST exact call on the current device.  which = 0: the final queue (entries
// re-evaluated in fp64), 1: the raw queue of a merging call with its cost images.  Copies up to max_n entries; *n = entries appended.
int ssamd_debug_exact_queue(int which, long long max_n, unsigned long long *entries, unsigned int *keys, long long *n)
{
    if (!n || max_n < 0 || (max_n > 0 && !entries)) return fail(SSAMD_EINVAL, "bad argument");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    *n = 0;
    if (!c->xflags.ptr || c->exact_calls == 0) return SSAMD_OK;
    HIP_TRY(hipDeviceSynchronize());
    unsigned int ctr[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(ctr, c->xflags.ptr, sizeof(ctr), hipMemcpyDeviceToHost));
    const unsigned int cnt = which ? ctr[4] : ctr[0], cap = which ? c->xrawcap : c->xcap;
    *n = cnt;
    const size_t m = (size_t)std::min<long long>(std::min<unsigned int>(cnt, cap), max_n);
    if (m == 0) return SSAMD_OK;
    const void *src = which ? c->xraw.ptr : c->xqueue.ptr;
    if (!src) return SSAMD_OK;
    HIP_TRY(hipMemcpy(entries, src, m * 8, hipMemcpyDeviceToHost));
    if (which && keys) HIP_TRY(hipMemcpy(keys, (const char *)src + (size_t)c->xrawcap * 8, m * 4, hipMemcpyDeviceToHost));
    return SSAMD_OK;
}

int ssamd_debug_libm(int which, int n, const void *in, void *out)
{
    if (!in || !out || n < 0 || which < 0 || which > 3)
        return fail(SSAMD_EINVAL, "ssamd_debug_libm: which = 0 (exp, doubles), 1 (powf(x, 1/3), floats), 2 (sqrt, doubles), 3 (x / 0.7 + x / 5.0, doubles)");
    if (n == 0) return SSAMD_OK;
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    const size_t bytes = (size_t)n * (which == 1 ? 4 : 8);
    if ((rc = c->lab.reserve(2 * bytes))) return rc;
    char *const d_in = (char *)c->lab.ptr, *const d_out = d_in + bytes;
    HIP_TRY(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(debug_libm_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, which, n, (const void *)d_in, (void *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SSAMD_OK;
}

int ssamd_debug_gsw_sqrt(int n, float *out)
{
    int what = 0;
    if (n < 0) { what = 1; n = -n; }       // n < 0: the bare v_sqrt_f32 over 0 .. -n - 1 (measurement of why it is not used)
    if (!out || n <= 0 || n > GSW_TAB_SIZE) return fail(SSAMD_EINVAL, "bad argument");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    if ((rc = c->lab.reserve((size_t)n * 4))) return rc;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    hipLaunchKernelGGL(gsw_sqrt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (float *)c->lab.ptr, n, what);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->lab.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

int ssamd_profile_enable(int on)
{
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        c.prof.on = on != 0;
    }
    return SSAMD_OK;
}

int ssamd_profile_reset(void)
{
    DeviceGuard guard;
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.dev < 0) continue;
        (void)hipSetDevice(c.dev);
        c.prof.drain();
        std::fill(c.prof.ms, c.prof.ms + SSAMD_K_COUNT, 0.0);
        std::fill(c.prof.n, c.prof.n + SSAMD_K_COUNT, 0LL);
    }
    return SSAMD_OK;
}

int ssamd_profile_read(double *ms, long long *launches)
{
    DeviceGuard guard;
    for (int k = 0; k < SSAMD_K_COUNT; ++k) { if (ms) ms[k] = 0; if (launches) launches[k] = 0; }
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.dev < 0) continue;
        (void)hipSetDevice(c.dev);
        c.prof.drain();
        for (int k = 0; k < SSAMD_K_COUNT; ++k) { if (ms) ms[k] += c.prof.ms[k]; if (launches) launches[k] += c.prof.n[k]; }
    }
    return SSAMD_OK;
}

}  // extern "C"
