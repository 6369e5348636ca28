// Classic FTP without a reference plane: the per-pixel _triangulate that ends the reference's StereoFTP_Mapping.getCloud
// (active.py:1436-1447 with _triangulate, :561-605): the unwrapped phase of the object image alone is mapped to a projector
// column, the projector row comes from the epipolar line of the fundamental matrix, and the pair is triangulated by the device
// function ftp_cloud_kernel and graycode_cloud_kernel end with (ftp_triangulate, ftp_cloud_kernels.hip.h).  One pointwise fp64
// kernel in ftp_cloud_kernel's frame (ftp_cloud_frame): 8 B of phase in, 24 B of point out; the geometry, F and the three scalars
// arrive by value.
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

// phase [h][w] (ROI origin x0, y0 in the camera image) -> out [h][w][3]: ftp_cloud_frame (ftp_cloud_kernels.hip.h) with
// ftp_mapping_pixel.  phase and out must be 16-byte aligned.
template <int MODEL>
__global__ __launch_bounds__(FTP_CLOUD_THREADS) void ftp_mapping_cloud_kernel(const double *__restrict__ phase, double *__restrict__ out,
                                                                              long long npix, int w, int x0, int y0, const FtpMapArgs A,
                                                                              const FtpCloudGeom G)
{
    ftp_cloud_frame(phase, out, npix, w, x0, y0, [&](double cx, double cy, double ph, double *o) {
        ftp_mapping_pixel<MODEL>(G, A, cx, cy, ph, o);
    });
}

}  // namespace ssamd
