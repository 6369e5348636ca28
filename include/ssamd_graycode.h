/*
 * ssamd_graycode.h -- third public header of libssamd.so: Gray-code structured light (simplestereo/active.py, class GrayCode),
 * beside ssamd.h and ssamd_active.h.
 *
 *   ssamd_graycode_decode   <->  cv2.structured_light_GrayCodePattern.getProjPixel for every pixel    active.py:1221-1226
 *                                (with cv2.undistort of every pattern image fused in, :1207)
 *   ssamd_graycode_offsets  <->  the order of the reference's pc / pp lists (raster order of the valid pixels)
 *   ssamd_graycode_cloud    <->  the triangulation that ends GrayCode.getCloud                        active.py:1232-1261
 *
 * Same library, same conventions as ssamd.h: int return codes (SSAMD_OK, SSAMD_E*), the message of ssamd_last_error, `device` = -1 for the
 * calling thread's current device, NAME takes host buffers and is synchronous, NAME_device takes device buffers and is
 * asynchronous on `stream`.  No CPU fallback.  This header has a version of its own; SSAMD_ABI_VERSION does not move with it.
 *
 * The pixels of the region [y0, y0 + h) x [x0, x0 + w) of the camera image are numbered in raster order, p = (y - y0) * w + (x - x0),
 * and cut into blocks of SSAMD_GRAYCODE_BLOCK consecutive pixels; nblocks = ceil(h * w / SSAMD_GRAYCODE_BLOCK).  h * w < 2^31.
 */
#ifndef SSAMD_GRAYCODE_H
#define SSAMD_GRAYCODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAMD_GRAYCODE_VERSION 1
#define SSAMD_GRAYCODE_BLOCK 1024

/* getProjPixel of OpenCV's GrayCodePattern for every pixel of the region: out[p] = (xDec, yDec), or (-1, -1) where it reports an
 * error.  Plane 2 k is the pattern image of bit k and plane 2 k + 1 its inverse; the ncol column bits come first, then the nrow row
 * bits, each most significant bit first (GrayCodePattern.generate()).  Per bit, with v1 the pattern and v2 the inverse value:
 * error if |v1 - v2| < white_thr; the Gray bit is 1 if v1 > v2, else 0; Gray -> binary is the MSB-first prefix XOR; after both
 * codes, error if xDec >= proj_w or yDec >= proj_h.  With n = 0 every pixel decodes to (0, 0).
 * With mapx and mapy (both or neither) each plane is first sampled as cv2.remap(plane, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT 0)
 * samples an 8-bit image: q = rint(map * 32) to even, cell q >> 5, fraction q & 31, (S + 512) >> 10 of the four taps with the
 * weights a * b, a, b in 0 .. 32, taps outside the plane 0; NaN, +-inf and coordinates whose product with 32 leaves int32 give 0.
 * One HIP kernel (csrc/graycode_kernels.hip.h); equal value for value to the numpy restatement tests/_graycode_ref.py.
 *   planes : uint8 [n][hc][wc]; may be NULL when n == 0
 *   mapx, mapy : float32 [hc][wc], indexed by the camera pixel, or both NULL
 *   n, ncol, nrow : n == 2 * (ncol + nrow), 0 <= ncol, nrow <= 16
 *   proj_w, proj_h : 1 .. 65536
 *   white_thr : 0 .. 256
 *   out    : int32 [h][w][2]
 *   counts : int32 [nblocks], the valid pixels of every block, or NULL
 * SSAMD_EINVAL: a NULL pointer (but those named above), a negative size or origin, a region that leaves the planes, hc * wc or
 * h * w of 2^31 or more, n, ncol, nrow, proj_w, proj_h or white_thr outside the above, one map without the other, an output buffer
 * not 16-byte aligned (device form).  An empty region does nothing. */
int ssamd_graycode_decode(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                          int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *out, int32_t *counts, int device);
int ssamd_graycode_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                 int h, int w, int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *d_out, int32_t *d_counts,
                                 void *stream);

/* Exclusive prefix sum of the block counts: offsets[i] = counts[0] + ... + counts[i - 1] for i = 0 .. nblocks, so that
 * offsets[nblocks] is the number of valid pixels.  One HIP kernel, one workgroup.
 *   counts  : int32 [nblocks], each 0 .. SSAMD_GRAYCODE_BLOCK
 *   offsets : int32 [nblocks + 1]
 * SSAMD_EINVAL: a NULL pointer, nblocks < 0 or nblocks > 2^21 (h * w < 2^31). */
int ssamd_graycode_offsets(const int32_t *counts, int nblocks, int32_t *offsets, int device);
int ssamd_graycode_offsets_device(const int32_t *d_counts, int nblocks, int32_t *d_offsets, void *stream);

/* The points of the valid pixels.  Pixel (x, y) of the region with the decoded projector pixel (xDec, yDec) is triangulated from
 * pc = (x + 0.5, y + 0.5) and pp = (xDec + 0.5, yDec + 0.5): cv2.undistortPoints(pp, K2, distCoeffs2, P = K2) (five iterations), the
 * two rectifying homographies, baseline / |disparity| and the common rotation undone -- the operations of ssamd_ftp_cloud from
 * its undistortPoints on, in the same order, fp64, each rounded once.
 *   geom : HOST array of SSAMD_FTP_CLOUD_NGEOM doubles (layout in ssamd.h), consumed before the call returns; only [12..36]
 *          (fx2 fy2 cx2 cy2, the twelve distortion coefficients, P) and [40..67] (Rectify1, Rectify2, inv(commonR), the baseline) are
 *          read and must be finite; M, T, the epipole and 2 pi fp are not read (a rig with T[2] == 0 is fine)
 *
 * Device form: the decoded pixels of ssamd_graycode_decode_device and the offsets of ssamd_graycode_offsets_device.
 *   d_decoded : int32 [h][w][2], 16-byte aligned
 *   d_offsets : int32 [nblocks + 1]: d_out is float64 [offsets[nblocks]][3], the points in raster order (the caller reads the
 *               total to size it) -- or NULL: d_out is float64 [h][w][3] with NaN at the invalid pixels, and nothing is read back
 *
 * Host form: the whole chain on host buffers -- decode (arguments as in ssamd_graycode_decode), offsets, cloud.
 *   dense   : 0: out receives the *npoints points in raster order; otherwise out is [h][w][3] with NaN at the invalid pixels
 *   out     : float64, room for h * w * 3 values in either case
 *   npoints : the number of valid pixels
 * SSAMD_EINVAL: as ssamd_graycode_decode, a NULL geom, out or npoints, a non-finite entry of geom[12..36] or geom[40..67], a
 * misaligned d_decoded.  An empty region does nothing (*npoints = 0). */
int ssamd_graycode_cloud(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                         int ncol, int nrow, int proj_w, int proj_h, int white_thr, const double *geom, int dense, double *out, int *npoints,
                         int device);
int ssamd_graycode_cloud_device(const int32_t *d_decoded, int h, int w, int x0, int y0, const double *geom, const int32_t *d_offsets,
                                double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAMD_GRAYCODE_H */
