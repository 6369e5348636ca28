// Phase-shift structured light: the three closures of the reference's calibration.phaseShift (getPhase, unwrap, getProjCoord,
// calibration.py:656-687 and :726-738) run on every camera pixel, and the triangulation of StructuredLightRig.triangulate
// (_rigs.py:654-700) for correspondences of the caller's own.  Two kernels:
//   phaseshift_decode_kernel  planes (+ the undistortion maps) -> the projector coordinates (px, py) per pixel, NaN where masked
//   sl_triangulate_kernel     camera points (or the pixel grid) + projector points -> points, by ftp_triangulate
// The decode uses the partition and the front of graycode_decode_kernel (PlaneStack and plane_stack_frame of
// graycode_kernels.hip.h): the region's pixels are one flattened index p = ry * w + rx (npix = h w < 2^31), GRAYCODE_BLOCK
// consecutive pixels per workgroup, thread t owns the pixels 4 t .. 4 t + 3 of its block, the plane loop innermost, the taps of a
// pixel computed once for all planes; phaseshift_coords is the body the frame calls.
#pragma once
#include "common.hip.h"
#include "ftp_cloud_kernels.hip.h"
#include "graycode_kernels.hip.h"

namespace ssamd {

constexpr int SL_MAX_PERIODS = 8;              // SSAMD_SL_MAX_PERIODS of include/ssamd_structured_light.h

struct PhaseShiftArgs {
    PlaneStack stack;               // 4 (nx + ny) planes: I0 .. I3 of each x-period, then of each y-period
    double *out;                    // [h][w][2]
    int n[2];                       // periods per axis, 1 .. SL_MAX_PERIODS
    int thr2;                       // mask where a^2 + b^2 < thr2
    double T[2][SL_MAX_PERIODS];    // the periods, T[axis][0] the first
    double extent[2];               // proj_w, proj_h
};

// A plane pointer as the scalar it is (the same in every lane).  Without it the compiler keeps one 64-bit address per tap and
// plane alive across the plane loop as an induction variable: 256 VGPRs and one wave per SIMD for the kernel with maps, against
// 192 and two this way (66 against 90 without maps).
__device__ __forceinline__ const uint8_t *phaseshift_uniform(const uint8_t *p)
{
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const uint8_t *)(((uint64_t)hi << 32) | lo);
}

// The projector coordinates of a thread's four pixels: per axis the wrapped phase of the first period, then one heterodyne step
// per later period, then getProjCoord.  masked[j]: some set's a^2 + b^2 (integers, at most 2 * 255^2) is below thr2.
template <int MODE>
__device__ __forceinline__ void phaseshift_coords(const PhaseShiftArgs &A, const bool (&live)[GRAYCODE_PER_THREAD], const uint32_t (&at)[GRAYCODE_PER_THREAD],
                                                  const GrayTaps *taps, const GrayWindow *win, double (&coord)[2][GRAYCODE_PER_THREAD],
                                                  bool (&masked)[GRAYCODE_PER_THREAD])
{
#pragma clang fp contract(off)
    const double two_pi = 6.283185307179586476925286766559;      // 2 * np.pi, exact doubling of the double pi
    const PlaneStack &S = A.stack;
    const uint8_t *pl = S.planes;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) masked[j] = false;
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        double phi[GRAYCODE_PER_THREAD];
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) phi[j] = 0.0;
        const double T0 = A.T[axis][0];
        for (int k = 0; k < A.n[axis]; ++k) {
            int I[4][GRAYCODE_PER_THREAD];
#pragma unroll
            for (int i = 0; i < 4; ++i) graycode_fetch<MODE>(phaseshift_uniform(pl + i * S.plane_stride), S.wc, live, at, taps, win, I[i]);
            pl += 4 * S.plane_stride;
            const double T = A.T[axis][k];
#pragma unroll
            for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
                const int a = I[3][j] - I[1][j], b = I[0][j] - I[2][j];
                masked[j] = masked[j] || a * a + b * b < A.thr2;
                double theta = atan2((double)a, (double)b);
                if (!(theta >= 0.0)) theta = theta + two_pi;
                if (k == 0) {
                    phi[j] = theta;
                } else {
                    const double kk = rint(((phi[j] * T0) / T - theta) / two_pi);
                    phi[j] = ((theta + two_pi * kk) * T) / T0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) coord[axis][j] = (A.extent[axis] * phi[j]) / two_pi;
    }
}

// HBM floor per pixel: 4 (nx + ny) plane bytes (+ 8 map bytes) in, 16 out.  out must be 16-byte aligned.
template <bool MAPS>
__global__ __launch_bounds__(GRAYCODE_THREADS) void phaseshift_decode_kernel(const PhaseShiftArgs A)
{
    const long long p0 = (long long)blockIdx.x * GRAYCODE_BLOCK + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    if (p0 >= A.stack.npix) return;              // (no barrier in this kernel)
    bool live[GRAYCODE_PER_THREAD], masked[GRAYCODE_PER_THREAD];
    double coord[2][GRAYCODE_PER_THREAD];
    plane_stack_frame<MAPS>(A.stack, p0, live, [&](auto mode, const uint32_t (&at)[GRAYCODE_PER_THREAD], const GrayTaps *taps, const GrayWindow *win) {
        phaseshift_coords<decltype(mode)::value>(A, live, at, taps, win, coord, masked);
    });
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double2 *const o = reinterpret_cast<double2 *>(A.out) + p0;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j)
        if (live[j]) o[j] = masked[j] ? make_double2(nan, nan) : make_double2(coord[0][j], coord[1][j]);
}

// StructuredLightRig.triangulate.  Point p from the camera point cam[p] -- or, with cam == NULL, the camera pixel
// (x0 + p % w, y0 + p / w), integer coordinates: the convention of the calibration routine the decode's formulae come from --
// and the projector point proj[p], by ftp_triangulate and nothing else; three NaN where proj[p] holds a NaN.  One point per
// thread; the workgroup's points are gathered in LDS (6 KiB) and leave as contiguous 8-byte stores, as graycode_cloud_kernel's
// do.  n is any count whose workgroups fit one grid dimension; cam, proj and out need 8-byte alignment only.
constexpr int SL_TRI_THREADS = 256;

template <int MODEL>
__global__ __launch_bounds__(SL_TRI_THREADS) void sl_triangulate_kernel(const double *__restrict__ cam, const double *__restrict__ proj,
                                                                        double *__restrict__ out, long long n, int w, int x0, int y0,
                                                                        const FtpCloudGeom G)
{
#pragma clang fp contract(off)
    __shared__ double stage[SL_TRI_THREADS * 3];
    const long long block0 = (long long)blockIdx.x * SL_TRI_THREADS;
    const long long p = block0 + (int)threadIdx.x;
    if (p < n) {
        const double px = proj[2 * p], py = proj[2 * p + 1];
        double u, v;
        if (cam) {                                            // (uniform: a kernel argument)
            u = cam[2 * p]; v = cam[2 * p + 1];
        } else {
            const long long ry = p / w, rx = p - ry * w;
            u = (double)(rx + x0); v = (double)(ry + y0);     // exact: integers below 2^53
        }
        double o[3];
        if (px != px || py != py) {
            o[0] = o[1] = o[2] = __longlong_as_double(0x7ff8000000000000ll);
        } else {
            ftp_triangulate<MODEL>(G, u, v, px, py, o);
        }
        stage[3 * threadIdx.x] = o[0]; stage[3 * threadIdx.x + 1] = o[1]; stage[3 * threadIdx.x + 2] = o[2];
    }
    __syncthreads();
    const long long left = n - block0;
    const int total = (int)(left < SL_TRI_THREADS ? left : SL_TRI_THREADS);
    double *const dst = out + 3 * block0;
    for (int i = threadIdx.x; i < 3 * total; i += SL_TRI_THREADS) dst[i] = stage[i];
}

}  // namespace ssamd
