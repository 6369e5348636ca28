// FTP phase -> point cloud: the triangulation of the reference's StereoFTP.getCloud (active.py:776-841, with the projector
// coordinates of _getProjectorMapping, :463-485), which is 2 W H cv2.projectPoints, W H cv2.undistortPoints and three
// cv2.perspectiveTransform there.  One pointwise fp64 kernel: 8 B of phase in, 24 B of point out, nothing else read from
// memory -- the geometry arrives by value (FtpCloudGeom, as Mat4 in rig_kernels.hip.h).  The kernel is ftp_cloud_pixel in
// ftp_cloud_frame; ftp_mapping_cloud_kernel (ftp_mapping_kernels.hip.h) is another pixel function in the same frame.
//
// Arithmetic contract: every pixel is evaluated by the operations of tests/_ftp_cloud_ref.py (cloud_from_geometry) in that
// order, each rounded once: no contraction into fused multiply-adds, IEEE divisions.  With the same geometry
// the output equals that numpy restatement bit for bit wherever the intermediate values are finite, so a pixel whose disparity
// is exactly 0 there is exactly 0 here.  A distortion model leaves out only terms that are exact no-ops for its zero
// coefficients on finite values (x * 1, + 0, / 1), which is why the model is a template parameter and not a data-dependent branch:
//   0 no distortion   1 k1 k2 p1 p2 k3   2 + k4 k5 k6 (rational)   3 + s1 .. s4 (thin prism)
// No bit-parity with cv2 is claimed (its operation order is not the restatement's).
#pragma once
#include "common.hip.h"

namespace ssamd {

// include/ssamd.h documents the same layout for the flat `geom` array of the C ABI (SSAMD_FTP_CLOUD_NGEOM doubles)
struct FtpCloudGeom {
    double M[9];        // z_plane * R * inv(K1), used verbatim as projectPoints' rotation matrix (active.py:479)
    double T[3];        // tvec (:480)
    double f2[4];       // fx2, fy2, cx2, cy2 of K2 (:480; the skew is ignored, as in OpenCV)
    double d[12];       // distCoeffs2 k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (:481)
    double P[9];        // undistortPoints' P = K2, all nine entries (:813)
    double ep[2];       // epipole on the projector image (:394-395)
    double two_pi_fp;   // (2 pi) * fp, fp = 1 / period (:799)
    double R1[9];       // Rectify1 (:390, :823)
    double R2[9];       // Rectify2 (:390, :830)
    double Ri[9];       // inv(commonR) (:398)
    double baseline;    // rig.getBaseline() (:834)
};
static_assert(sizeof(FtpCloudGeom) == 68 * sizeof(double), "SSAMD_FTP_CLOUD_NGEOM");

constexpr int FTP_CLOUD_THREADS = 256;
constexpr int FTP_CLOUD_WAVES = FTP_CLOUD_THREADS / 64;

// cv2.projectPoints((u, v, 1), M, T, K2, distCoeffs2) with the 3x3 M copied into the rotation matrix (active.py:478-481):
// the operations of tests/_ftp_cloud_ref.py (project_points) in that order.  Geom is any struct that begins like FtpCloudGeom
// (M, T, f2, d): ftp_cloud_kernel and ftp_reference_kernel (ftp_reference_kernels.hip.h) share this text.
template <int MODEL, class Geom>
__device__ __forceinline__ void ftp_project(const Geom &G, double u, double v, double &Xa, double &Ya)
{
#pragma clang fp contract(off)
    const double k1 = G.d[0], k2 = G.d[1], p1 = G.d[2], p2 = G.d[3], k3 = G.d[4], k4 = G.d[5], k5 = G.d[6], k6 = G.d[7];
    const double s1 = G.d[8], s2 = G.d[9], s3 = G.d[10], s4 = G.d[11];
    const double X = ((G.M[0] * u + G.M[1] * v) + G.M[2]) + G.T[0];
    const double Y = ((G.M[3] * u + G.M[4] * v) + G.M[5]) + G.T[1];
    const double Z = ((G.M[6] * u + G.M[7] * v) + G.M[8]) + G.T[2];
    const double iz = 1.0 / Z;
    const double x = X * iz, y = Y * iz;
    double xd = x, yd = y;
    if (MODEL > 0) {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        double kr = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6;
        if (MODEL > 1) kr = kr / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6);
        xd = (x * kr + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x);
        yd = (y * kr + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y;
        if (MODEL > 2) {
            xd = (xd + s1 * r2) + s2 * r4;
            yd = (yd + s3 * r2) + s4 * r4;
        }
    }
    Xa = G.f2[0] * xd + G.f2[2];
    Ya = G.f2[1] * yd + G.f2[3];
}

// A point (u, v) of image 1 and an undistorted point (hx, hy) of image 2 -> point o[0..2]: the two rectifying homographies (of
// the second point only x is used), disparity -> depth, the common rotation undone.  Reads R1, R2, Ri and baseline of G.  What
// ftp_triangulate ends with, and all of the two-camera triangulation (graycode_stereo_kernels.hip.h, active.py:1594-1606), where
// both images were undistorted beforehand.  A disparity of exactly 0 divides by zero as the reference's arithmetic does: inf / NaN.
__device__ __forceinline__ void rectified_triangulate(const FtpCloudGeom &G, double u, double v, double hx, double hy, double *o)
{
#pragma clang fp contract(off)
    const double ppx = ((G.R2[0] * hx + G.R2[1] * hy) + G.R2[2]) / ((G.R2[6] * hx + G.R2[7] * hy) + G.R2[8]);
    const double Wc = (G.R1[6] * u + G.R1[7] * v) + G.R1[8];
    const double pcx = ((G.R1[0] * u + G.R1[1] * v) + G.R1[2]) / Wc, pcy = ((G.R1[3] * u + G.R1[4] * v) + G.R1[5]) / Wc;
    const double disparity = fabs(ppx - pcx);
    const double px = G.baseline * (pcx / disparity), py = G.baseline * (pcy / disparity), pz = G.baseline * (1.0 / disparity);
    o[0] = (G.Ri[0] * px + G.Ri[1] * py) + G.Ri[2] * pz;
    o[1] = (G.Ri[3] * px + G.Ri[4] * py) + G.Ri[5] * pz;
    o[2] = (G.Ri[6] * px + G.Ri[7] * py) + G.Ri[8] * pz;
}

// The camera pixel centre (u, v) and the projector point (Xh, Yh) it corresponds to -> point o[0..2]: the triangulation both
// structured-light methods end with (active.py:813-841 for StereoFTP, :1246-1261 for GrayCode), the operations of
// tests/_ftp_cloud_ref.py (cloud_from_geometry) from its undistort_points line to the end.  Reads f2, d, P, R1, R2, Ri and
// baseline of G; ftp_cloud_kernel and graycode_cloud_kernel (graycode_kernels.hip.h) share this text.
template <int MODEL>
__device__ __forceinline__ void ftp_triangulate(const FtpCloudGeom &G, double u, double v, double Xh, double Yh, double *o)
{
#pragma clang fp contract(off)
    const double k1 = G.d[0], k2 = G.d[1], p1 = G.d[2], p2 = G.d[3], k3 = G.d[4], k4 = G.d[5], k5 = G.d[6], k6 = G.d[7];
    const double s1 = G.d[8], s2 = G.d[9], s3 = G.d[10], s4 = G.d[11];
    // undistortPoints(H, K2, dist2, P = K2): five fixed-point iterations
    const double xn = (Xh - G.f2[2]) / G.f2[0], yn = (Yh - G.f2[3]) / G.f2[1];
    double a = xn, b = yn;
    if (MODEL > 0) {
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const double r2 = a * a + b * b;
            const double den = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double icdist = (MODEL > 1 ? 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2 : 1.0) / den;
            double dx = ((2.0 * p1) * a) * b + p2 * (r2 + (2.0 * a) * a);
            double dy = p1 * (r2 + (2.0 * b) * b) + ((2.0 * p2) * a) * b;
            if (MODEL > 2) {
                dx = (dx + s1 * r2) + (s2 * r2) * r2;
                dy = (dy + s3 * r2) + (s4 * r2) * r2;
            }
            a = (xn - dx) * icdist;
            b = (yn - dy) * icdist;
        }
    }
    const double Wp = (G.P[6] * a + G.P[7] * b) + G.P[8];
    const double hx = ((G.P[0] * a + G.P[1] * b) + G.P[2]) / Wp, hy = ((G.P[3] * a + G.P[4] * b) + G.P[5]) / Wp;
    rectified_triangulate(G, u, v, hx, hy, o);
}

// One pixel centre (u, v) and its unwrapped phase (already shifted by the fringe order) -> point o[0..2].
template <int MODEL>
__device__ __forceinline__ void ftp_cloud_pixel(const FtpCloudGeom &G, double u, double v, double ph, double *o)
{
#pragma clang fp contract(off)
    // projector coordinates of the camera pixel on the reference plane: projectPoints
    double Xa, Ya;
    ftp_project<MODEL>(G, u, v, Xa, Ya);
    // phase -> projector column, row on the epipolar line
    const double Xh = Xa + ph / G.two_pi_fp;
    const double Yh = ((Xh - G.ep[0]) / (Xa - G.ep[0])) * (Ya - G.ep[1]) + G.ep[1];
    ftp_triangulate<MODEL>(G, u, v, Xh, Yh, o);
}

// The frame of the pointwise cloud kernels (ftp_cloud_kernel here, ftp_mapping_cloud_kernel of ftp_mapping_kernels.hip.h):
// phase [h][w] (ROI origin x0, y0 in the camera image) -> out [h][w][3], with pixel(u, v, phase, o) the per-pixel step from a pixel
// centre and its phase to the point o[0..2].  Pixels are one flattened index (npix = h w < 2^31): rows are not a grid dimension,
// so h is not limited by one.  A thread owns the two pixels 2q, 2q + 1 (one 16-byte phase read); whole waves iterate, so that a
// wave's up to 128 x 24 bytes go out as three contiguous 1 KiB stores: the 16-byte chunks are transposed through LDS and lane l
// writes chunks l, l + 64, l + 128 (reproject_kernel's pattern).  phase and out must be 16-byte aligned; blockDim.x is
// FTP_CLOUD_THREADS.  (The kernels' own parameters are __restrict__; the frame's need not be.)
template <class Pixel>
__device__ __forceinline__ void ftp_cloud_frame(const double *phase, double *out, long long npix, int w, int x0, int y0, Pixel pixel)
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
            // the pixel centre, (x + x0) + 0.5: the restatement of the mapping spells it (x + 0.5) + x0, and both sums are exact in
            // fp64 (integers below 2^32, then one half), so the one spelling gives either restatement's value
            pixel(((double)xx + (double)x0) + 0.5, ((double)yy + (double)y0) + 0.5, ph0, o);
            pixel(((double)(wrap ? 0u : xx + 1) + (double)x0) + 0.5, ((double)(wrap ? yy + 1 : yy) + (double)y0) + 0.5, ph1, o + 3);
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

// The frame with ftp_cloud_pixel on the phase shifted by the fringe order (kshift = 2 pi k).
template <int MODEL>
__global__ __launch_bounds__(FTP_CLOUD_THREADS) void ftp_cloud_kernel(const double *__restrict__ phase, double *__restrict__ out,
                                                                      long long npix, int w, int x0, int y0, double kshift,
                                                                      const FtpCloudGeom G)
{
    ftp_cloud_frame(phase, out, npix, w, x0, y0, [&](double u, double v, double ph, double *o) {
#pragma clang fp contract(off)
        ftp_cloud_pixel<MODEL>(G, u, v, ph + kshift, o);
    });
}

}  // namespace ssamd
