// Classic FTP without a reference plane: the per-pixel _triangulate that ends the reference's StereoFTP_Mapping.getCloud
// (active.py:1436-1447 with _triangulate, :561-605): the unwrapped phase of the object image alone is mapped to a projector
// column, the projector row comes from the epipolar line of the fundamental matrix, and the pair is triangulated by the device
// function ftp_cloud_kernel and graycode_cloud_kernel end with (ftp_triangulate, ftp_cloud_kernels.hip.h).  One pointwise fp64
// kernel: 8 B of phase in, 24 B of point out; the geometry, F and the three scalars arrive by value.
//
// Arithmetic contract: the operations of tests/_ftp_mapping_ref.py (mapping_cloud) in that order, each rounded once -- no
// contraction into fused multiply-adds, IEEE divisions -- so the output equals that numpy restatement bit for bit, non-finite
// values included.  Of the geometry only f2, d, P, R1, R2, Ri and baseline are read: neither a reference plane nor the epipole
// enters, so a rig with T[2] == 0 works.
#pragma once
#include "ftp_cloud_kernels.hip.h"

namespace ssamd {

struct FtpMapArgs {
    double F[9];        // the fundamental matrix, camera point -> line on the projector image (active.py:573)
    double theta;       // the phase at the central stripe (:1431-1436)
    double peak;        // stripeCentralPeak (:1441)
    double two_pi_fp;   // (2 pi) * fp (:1441)
};

// One pixel centre (cx, cy) of the camera image and its unwrapped phase -> point o[0..2].
template <int MODEL>
__device__ __forceinline__ void ftp_mapping_pixel(const FtpCloudGeom &G, const FtpMapArgs &A, double cx, double cy, double ph, double *o)
{
#pragma clang fp contract(off)
    const double px = (((ph - A.theta) / A.two_pi_fp) + A.peak) + 0.5;
    const double l0 = (A.F[0] * cx + A.F[1] * cy) + A.F[2];
    const double l1 = (A.F[3] * cx + A.F[4] * cy) + A.F[5];
    const double l2 = (A.F[6] * cx + A.F[7] * cy) + A.F[8];
    const double py = -((l0 * px + l2) / l1);
    ftp_triangulate<MODEL>(G, cx, cy, px, py, o);
}

// phase [h][w] (ROI origin x0, y0 in the camera image) -> out [h][w][3].  The frame of ftp_cloud_kernel: pixels are one
// flattened index (npix = h w < 2^31; rows are not a grid dimension), a thread owns the two pixels 2q, 2q + 1 (one 16-byte
// phase read), and a wave's up to 128 x 24 bytes go out as three contiguous 1 KiB stores through an LDS transpose.  phase and
// out must be 16-byte aligned.
template <int MODEL>
__global__ __launch_bounds__(FTP_CLOUD_THREADS) void ftp_mapping_cloud_kernel(const double *__restrict__ phase, double *__restrict__ out,
                                                                              long long npix, int w, int x0, int y0, const FtpMapArgs A,
                                                                              const FtpCloudGeom G)
{
#pragma clang fp contract(off)
    __shared__ double2 xchg[FTP_CLOUD_WAVES][192];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * FTP_CLOUD_THREADS;
    // q0: the wave's first pair of this round
    for (long long q0 = (long long)blockIdx.x * FTP_CLOUD_THREADS + (threadIdx.x - lane); 2 * q0 < npix; q0 += stride) {
        const long long p = 2 * (q0 + lane);
        if (p < npix) {
            const bool two = p + 1 < npix;
            double ph0, ph1 = 0.0;
            if (two) {
                const double2 pv = reinterpret_cast<const double2 *>(phase)[q0 + lane];
                ph0 = pv.x; ph1 = pv.y;
            } else {
                ph0 = phase[p];
            }
            const unsigned int yy = (unsigned int)p / (unsigned int)w, xx = (unsigned int)p - yy * (unsigned int)w;
            const bool wrap = xx + 1 == (unsigned int)w;          // the second pixel starts the next row
            double o[6];
            ftp_mapping_pixel<MODEL>(G, A, ((double)xx + 0.5) + (double)x0, ((double)yy + 0.5) + (double)y0, ph0, o);
            ftp_mapping_pixel<MODEL>(G, A, ((double)(wrap ? 0u : xx + 1) + 0.5) + (double)x0, ((double)(wrap ? yy + 1 : yy) + 0.5) + (double)y0,
                                     ph1, o + 3);
            double2 *const mine = xchg[wave] + 3 * lane;
            mine[0] = make_double2(o[0], o[1]);
            mine[1] = make_double2(o[2], o[3]);
            mine[2] = make_double2(o[4], o[5]);
        }
        // (a wave's LDS accesses execute in order: no workgroup barrier)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const long long left = npix - 2 * q0;
        const int n = (int)(left < 128 ? left : 128);              // pixels of this wave in this round
        const int nchunk = 3 * n / 2;                              // whole 16-byte chunks of their 24 n bytes
        double2 *const op = reinterpret_cast<double2 *>(out + 6 * q0);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (lane + 64 * k < nchunk) op[lane + 64 * k] = xchg[wave][lane + 64 * k];
        if ((n & 1) && lane == 0) out[6 * q0 + 3 * n - 1] = xchg[wave][nchunk].x;       // z of an odd last pixel
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace ssamd
