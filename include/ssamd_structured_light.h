/*
 * ssamd_structured_light.h -- fifth public header of libssamd.so: phase-shift decoding with heterodyne unwrapping and the
 * triangulation of arbitrary camera-projector correspondences, beside ssamd.h, ssamd_active.h, ssamd_graycode.h and
 * ssamd_ftp_mapping.h.
 *
 *   ssamd_phaseshift_decode  <->  getPhase, unwrap and getProjCoord of calibration.phaseShift for every pixel   calibration.py:656-687, :726-738
 *                                 (with cv2.undistort of every image fused in)
 *   ssamd_sl_triangulate     <->  StructuredLightRig.triangulate                                                _rigs.py:654-700
 *
 * Same library, same conventions as ssamd.h: int return codes (SSAMD_OK, SSAMD_E*), the message of ssamd_last_error, `device` = -1 for the
 * calling thread's current device, NAME takes host buffers and is synchronous, NAME_device takes device buffers and is
 * asynchronous on `stream`.  No CPU fallback.  This header has a version of its own; SSAMD_ABI_VERSION does not move with it.
 */
#ifndef SSAMD_STRUCTURED_LIGHT_H
#define SSAMD_STRUCTURED_LIGHT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAMD_SL_VERSION 1
#define SSAMD_SL_MAX_PERIODS 8

/* Four-step phase shifting with heterodyne unwrapping for every pixel of the region [y0, y0 + h) x [x0, x0 + w):
 * out[p] = (px, py), the projector coordinates of the camera pixel.  The planes come in the reference's image-set order: the four
 * shifts I0 .. I3 of each x-period, then those of each y-period, I_i = cos(theta + i pi / 2) expected.  Per pixel, in fp64, no
 * contraction, each operation rounded once, in this order:
 *   a = I3 - I1, b = I0 - I2 (exact);  theta = atan2(a, b);  numpy's mod(theta, 2 pi): theta if theta >= 0, else theta + 2 pi
 *   first period of an axis: phi = theta
 *   every later period T against the first T0: k = rint(((phi * T0) / T - theta) / (2 pi)) (ties to even),
 *                                              phi = ((theta + (2 pi) * k) * T) / T0
 *   px = (proj_w * phi_x) / (2 pi), py = (proj_h * phi_y) / (2 pi)
 * A pixel for which any of the nx + ny sets has a * a + b * b < mod_thr2 (integers) gets (NaN, NaN); mod_thr2 = 0 masks nothing.
 * With mapx and mapy (both or neither) each plane is first sampled as ssamd_graycode_decode samples it
 * (cv2.remap INTER_LINEAR, BORDER_CONSTANT 0 on an 8-bit image); a pixel's taps are computed once for all planes.
 * One HIP kernel (csrc/phaseshift_kernels.hip.h); atan2 is the device library's, so the result is close to, not bit-equal to,
 * the numpy restatement tests/_phaseshift_ref.py.
 *   planes : uint8 [n][hc][wc]
 *   mapx, mapy : float32 [hc][wc], indexed by the camera pixel, or both NULL
 *   n, nx, ny : n == 4 * (nx + ny), 1 <= nx, ny <= SSAMD_SL_MAX_PERIODS
 *   periods_x [nx], periods_y [ny] : HOST arrays, consumed before the call returns, each finite and > 0
 *   proj_w, proj_h : 1 .. 65536
 *   mod_thr2 : >= 0
 *   out : float64 [h][w][2]
 * SSAMD_EINVAL: a NULL pointer (but the maps), a negative size or origin, a region that leaves the planes, hc * wc or h * w of
 * 2^31 or more, n, nx, ny, a period, proj_w, proj_h or mod_thr2 outside the above, one map without the other, an output buffer not
 * 16-byte aligned (device form).  An empty region does nothing. */
int ssamd_phaseshift_decode(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                            int nx, int ny, const double *periods_x, const double *periods_y, int proj_w, int proj_h, int mod_thr2,
                            double *out, int device);
int ssamd_phaseshift_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                   int h, int w, int nx, int ny, const double *periods_x, const double *periods_y, int proj_w, int proj_h,
                                   int mod_thr2, double *d_out, void *stream);

/* StructuredLightRig.triangulate: point p from the (undistorted) camera point cam[p] and the projector point proj[p]:
 * Rectify1 on the camera point, cv2.undistortPoints(proj, K2, distCoeffs2, P = K2) (five iterations), Rectify2,
 * baseline / |disparity| and the common rotation undone -- the operations ssamd_graycode_cloud ends with, in the same order, fp64,
 * each rounded once.  A point whose proj holds a NaN is written as three NaN.
 *   cam  : float64 [n][2], or NULL: point p is the camera pixel (x0 + p % w, y0 + p / w), integer coordinates, nothing added
 *   proj : float64 [n][2]
 *   n    : 0 .. 2^38
 *   w, x0, y0 : read only when cam is NULL; then w >= 1, x0, y0 >= 0
 *   geom : HOST array of SSAMD_FTP_CLOUD_NGEOM doubles (layout in ssamd.h), consumed before the call returns; only [12..36] and
 *          [40..67] are read and must be finite, as for ssamd_graycode_cloud
 *   out  : float64 [n][3]
 * SSAMD_EINVAL: a NULL proj, geom or out, n outside the above, with cam NULL w < 1 or a negative origin, a non-finite entry of
 * geom[12..36] or geom[40..67], a buffer not 8-byte aligned (device form).  n == 0 does nothing. */
int ssamd_sl_triangulate(const double *cam, const double *proj, long long n, int w, int x0, int y0, const double *geom, double *out,
                         int device);
int ssamd_sl_triangulate_device(const double *d_cam, const double *d_proj, long long n, int w, int x0, int y0, const double *geom,
                                double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAMD_STRUCTURED_LIGHT_H */
