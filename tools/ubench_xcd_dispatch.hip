// tools/ubench_xcd_dispatch.hip -- how the dispatcher deals the workgroups of ONE launch over the eight XCDs when one workgroup
// fits a CU, and what lies between two workgroups on the same CU (round 8: the premise of a persistent asw_aggregate_pipe_kernel).
// 2048 workgroups of 768 threads that each ask for 136 KB of dynamic LDS (one resident per CU, like the 120 x 196 tile) and run a
// fixed count of dependent FMAs; the workgroups with linear id % 8 == 0 run 0.75 x the count (the left-border tile of a 1080p row).
// Every workgroup records its XCD (HW_REG_XCC_ID), its CU (HW_REG_HW_ID: shader engine, array, CU), wall_clock64() (100 MHz) at its
// start and end, and its linear id.  The host answers:
//   1. is the block -> XCD deal static (block b on the XCD of block b % 8 whatever the load), so that the XCD with the light blocks
//      finishes early and idles, or do its CUs get other blocks?
//   2. how long is a CU without a workgroup between the end of one and the start of the next?
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_xcd_dispatch.hip -o tools/ubench_xcd_dispatch
// Run:   tools/ubench_xcd_dispatch [fmas per thread = 60000] [workgroups = 2048]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Rec { unsigned long long t0, t1; unsigned int xcc, hwid, id, pad; };

__global__ __launch_bounds__(768, 3) void dispatch_kernel(Rec *rec, float *sink, int iters, int light_mod)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned long long t0 = wall_clock64();
    const unsigned int id = blockIdx.x;
    const int n = light_mod > 0 && id % (unsigned)light_mod == 0 ? iters - iters / 4 : iters;
    float a = 1.0f + 1e-7f * threadIdx.x, x = 0.5f;
    for (int k = 0; k < n; ++k) x = fmaf(x, a, 1e-3f);           // one dependent chain per thread: nothing to overlap
    reinterpret_cast<float *>(smem)[threadIdx.x] = x;           // (the LDS request must not be optimised away)
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        Rec r;
        r.t0 = t0; r.t1 = wall_clock64(); r.xcc = xcc & 15u; r.hwid = hwid; r.id = id; r.pad = 0;
        rec[id] = r;
        sink[id] = reinterpret_cast<float *>(smem)[(id * 7u) % 768u];
    }
}

static double med(std::vector<double> v) { if (v.empty()) return 0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? std::max(1000, std::min(4000000, atoi(argv[1]))) : 60000;
    const int nwg = argc > 2 ? std::max(8, std::min(65536, atoi(argv[2]))) : 2048;
    const int lds = 136 * 1024;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    printf("device %s, %d CUs; %d workgroups x 768 threads, %d bytes of dynamic LDS, %d dependent FMAs (ids %% 8 == 0: %d)\n",
           prop.name, prop.multiProcessorCount, nwg, lds, iters, iters - iters / 4);
    HIP_OK(hipFuncSetAttribute((const void *)dispatch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    Rec *d_rec = nullptr;
    float *d_sink = nullptr;
    HIP_OK(hipMalloc(&d_rec, sizeof(Rec) * nwg));
    HIP_OK(hipMalloc(&d_sink, sizeof(float) * nwg));
    std::vector<Rec> rec(nwg);
    for (int pass = 0; pass < 3; ++pass) {          // pass 0 warms up; 1: light ids % 8 == 0; 2: all workgroups alike (control)
        const int light_mod = pass == 2 ? 0 : 8;
        HIP_OK(hipMemset(d_rec, 0, sizeof(Rec) * nwg));
        hipLaunchKernelGGL(dispatch_kernel, dim3(nwg), dim3(768), lds, 0, d_rec, d_sink, iters, light_mod);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        if (pass == 0) continue;
        HIP_OK(hipMemcpy(rec.data(), d_rec, sizeof(Rec) * nwg, hipMemcpyDeviceToHost));
        unsigned long long tmin = ~0ull, tmax = 0;
        for (const Rec &r : rec) { tmin = std::min(tmin, r.t0); tmax = std::max(tmax, r.t1); }
        const double us = 0.01;                       // wall_clock64 ticks at 100 MHz
        printf("\n== pass %d: %s; launch %.1f us from first start to last end\n", pass,
               light_mod ? "ids % 8 == 0 run 0.75 x the FMAs" : "all workgroups alike", (tmax - tmin) * us);
        // 1. per XCD: workgroups, how many of each id % 8, when its last workgroup ended
        printf("xcd  workgroups  light  ids%%8 histogram                          CUs  first start  last end (us)  idle before launch end\n");
        for (unsigned x = 0; x < 8; ++x) {
            int cnt = 0, light = 0, h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            unsigned long long e = 0, s = ~0ull;
            std::map<unsigned, int> cus;
            for (const Rec &r : rec)
                if (r.xcc == x) { ++cnt; ++h[r.id & 7]; light += (r.id & 7) == 0; e = std::max(e, r.t1); s = std::min(s, r.t0); ++cus[r.hwid & 0xff00u]; }
            if (!cnt) { printf("%3u  none\n", x); continue; }
            printf("%3u  %10d  %5d  %4d %4d %4d %4d %4d %4d %4d %4d  %3zu  %11.1f  %13.1f  %6.1f us = %4.1f %%\n", x, cnt, light, h[0], h[1], h[2], h[3], h[4], h[5],
                   h[6], h[7], cus.size(), (s - tmin) * us, (e - tmin) * us, (tmax - e) * us, 100.0 * (tmax - e) / (double)(tmax - tmin));
        }
        // 2. per CU (XCD, shader engine, array, CU of HW_ID bits 8..15): the workgroups in start order, the time between one's end
        //    and the next one's start, and how many ids of each kind the CU ran
        std::map<unsigned, std::vector<const Rec *>> by_cu;
        for (const Rec &r : rec) by_cu[(r.xcc << 16) | (r.hwid & 0xff00u)].push_back(&r);
        std::vector<double> gaps, durs_light, durs_full;
        int overlaps = 0;
        size_t most = 0, least = ~(size_t)0;
        for (auto &kv : by_cu) {
            auto &v = kv.second;
            std::sort(v.begin(), v.end(), [](const Rec *a, const Rec *b) { return a->t0 < b->t0; });
            most = std::max(most, v.size()); least = std::min(least, v.size());
            for (size_t k = 0; k < v.size(); ++k) {
                ((v[k]->id & 7) == 0 && light_mod ? durs_light : durs_full).push_back((v[k]->t1 - v[k]->t0) * us);
                if (k + 1 < v.size()) {
                    if (v[k + 1]->t0 < v[k]->t1) ++overlaps;
                    else gaps.push_back((v[k + 1]->t0 - v[k]->t1) * us);
                }
            }
        }
        std::vector<double> g = gaps;
        std::sort(g.begin(), g.end());
        printf("CUs seen: %zu; workgroups per CU: %zu .. %zu; two workgroups overlapping on one CU: %d\n", by_cu.size(), least, most, overlaps);
        printf("workgroup time: full median %.1f us, light median %.1f us\n", med(durs_full), med(durs_light));
        if (!g.empty())
            printf("gap between a workgroup's end and the next one's start on the same CU: min %.2f, median %.2f, p90 %.2f, max %.2f us (%zu gaps)\n",
                   g.front(), g[g.size() / 2], g[g.size() * 9 / 10], g.back(), g.size());
    }
    HIP_OK(hipFree(d_rec));
    HIP_OK(hipFree(d_sink));
    return 0;
}
