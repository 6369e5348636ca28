/*
 * ssamd_graycode_stereo.h -- sixth public header of libssamd.so: Gray-code active stereo with two calibrated cameras and one
 * uncalibrated projector, beside ssamd.h, ssamd_active.h, ssamd_graycode.h, ssamd_ftp_mapping.h and ssamd_structured_light.h.
 * It is what GrayCodeDouble.getCloud of simplestereo/active.py (:1463-1608) sets out to do; that code cannot run as published
 * (camera coordinates index the projector-shaped table, 0.5 is added to an integer array in place, self.R_inv is never assigned,
 * `.any` stands where "both cameras" is meant), so the semantics are written down here.
 *
 *   ssamd_graycode_stereo_match   <->  the two loops that fill `corresp`, and its filter         active.py:1558-1583
 *   ssamd_graycode_stereo_cloud   <->  the triangulation of the matched projector pixels          active.py:1594-1606
 *   ssamd_stereo_triangulate      <->  the same triangulation of point pairs of the caller's own
 *   ssamd_graycode_stereo_points  <->  GrayCodeDouble.getCloud from the two image stacks on
 *
 * Same library, same conventions as ssamd.h: int return codes (SSAMD_OK, SSAMD_E*), the message of ssamd_last_error, `device` = -1 for the
 * calling thread's current device, NAME takes host buffers and is synchronous, NAME_device takes device buffers and is
 * asynchronous on `stream`.  No CPU fallback.  This header has a version of its own; SSAMD_ABI_VERSION does not move with it.
 *
 * The projector's pixels ("cells") are numbered in raster order, c = yDec * proj_w + xDec, cells = proj_w * proj_h < 2^31, and cut
 * into blocks of SSAMD_GRAYCODE_BLOCK (ssamd_graycode.h) consecutive cells; nblocks = ceil(cells / SSAMD_GRAYCODE_BLOCK).
 */
#ifndef SSAMD_GRAYCODE_STEREO_H
#define SSAMD_GRAYCODE_STEREO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAMD_GRAYCODE_STEREO_VERSION 1
#define SSAMD_STEREO_LAST 0
#define SSAMD_STEREO_MEAN 1
/* bytes of the scratch of the device form of the match for `cells` projector pixels: both cameras' tables */
#define SSAMD_GRAYCODE_STEREO_SCRATCH(cells, reduce) (2 * ((((reduce) == SSAMD_STEREO_MEAN ? 20ll : 4ll) * (cells) + 7) & ~7ll))

/* Two decoded maps of ssamd_graycode_decode -> the camera-camera correspondences, one per projector pixel.
 * Camera i (i = 1, 2) contributes the pixels of its region [yi, yi + hi) x [xi, xi + wi) whose decoded value lies inside the
 * projector (an error value, or a value outside proj_w x proj_h, contributes nothing).  Of the pixels of one camera that decode
 * to one cell:
 *   SSAMD_STEREO_LAST  the one that comes last in raster order stands for the cell, as in the reference's loops, where a later
 *                      pixel overwrites an earlier one (an integer atomic max on y * (xi + wi) + x: no order of arrival in it)
 *   SSAMD_STEREO_MEAN  their centroid does: exact integer sums of x and of y (64 bits) and a count, then (double) sum / (double) count
 * Coordinates are absolute image coordinates: the origin (xi, yi) is added.  A cell both cameras reached gives
 * matches[c] = (x1 + 0.5, y1 + 0.5, x2 + 0.5, y2 + 0.5), pixel centres; any other cell gives four NaN.  Integer atomics only: the
 * same bytes on every run.  A memset and three kernel launches (two scatters, one match; csrc/graycode_stereo_kernels.hip.h); equal value for value to the
 * numpy restatement tests/_graycode_stereo_ref.py.
 *   decoded1, decoded2 : int32 [hi][wi][2]; may be NULL when the region is empty
 *   hi, wi, xi, yi : >= 0, hi * wi < 2^31 and (yi + hi) * (xi + wi) < 2^31
 *   proj_w, proj_h : 1 .. 65536, proj_w * proj_h < 2^31
 *   reduce  : SSAMD_STEREO_LAST or SSAMD_STEREO_MEAN
 *   matches : float64 [proj_h][proj_w][4]
 *   counts  : int32 [nblocks], the matched cells of every block (ssamd_graycode_offsets turns them into offsets), or NULL
 *   d_scratch : device form only: SSAMD_GRAYCODE_STEREO_SCRATCH(cells, reduce) bytes, 8-byte aligned; its content before and
 *               after the call means nothing
 * SSAMD_EINVAL: a NULL pointer (but those named above), a negative size or origin, a size or product outside the above, an
 * unknown reduce, d_decoded1, d_decoded2 or d_matches not 16-byte aligned, d_scratch not 8-byte aligned (device form). */
int ssamd_graycode_stereo_match(const int32_t *decoded1, int h1, int w1, int x1, int y1, const int32_t *decoded2, int h2, int w2, int x2, int y2,
                                int proj_w, int proj_h, int reduce, double *matches, int32_t *counts, int device);
int ssamd_graycode_stereo_match_device(const int32_t *d_decoded1, int h1, int w1, int x1, int y1, const int32_t *d_decoded2, int h2, int w2,
                                       int x2, int y2, int proj_w, int proj_h, int reduce, double *d_matches, int32_t *d_counts,
                                       void *d_scratch, void *stream);

/* The points of the matched cells.  From (p1x, p1y, p2x, p2y) = matches[c], in fp64, each operation rounded once, no contraction:
 * Rectify1 on (p1x, p1y), Rectify2 on (p2x, p2y) of which only x is used, disparity = |p1x' - p2x'|,
 * baseline * (p1' / disparity) and the common rotation undone -- the operations ssamd_graycode_cloud ends with after its
 * undistortPoints, which has no place here (both cameras' images were undistorted).  A disparity of exactly 0 gives inf / NaN
 * coordinates, as the reference's arithmetic does.
 *   matches : float64 [proj_h][proj_w][4], 16-byte aligned (device form)
 *   geom    : HOST array of SSAMD_FTP_CLOUD_NGEOM doubles (layout in ssamd.h), consumed before the call returns; only [40..67]
 *             (Rectify1, Rectify2, inv(commonR), the baseline) are read and must be finite
 *   offsets : int32 [nblocks + 1] of ssamd_graycode_offsets on the match's counts: out is float64 [offsets[nblocks]][3], the
 *             points in projector raster order -- or NULL: out is float64 [proj_h][proj_w][3], three NaN where the match holds a NaN
 * SSAMD_EINVAL: a NULL matches, geom or out, a projector size outside the above, a non-finite entry of geom[40..67], a
 * misaligned buffer (device form). */
int ssamd_graycode_stereo_cloud(const double *matches, int proj_w, int proj_h, const double *geom, const int32_t *offsets, double *out,
                                int device);
int ssamd_graycode_stereo_cloud_device(const double *d_matches, int proj_w, int proj_h, const double *geom, const int32_t *d_offsets,
                                       double *d_out, void *stream);

/* The same triangulation of n point pairs of the caller's own: out[p] from points1[p] (image 1) and points2[p] (image 2), both
 * already undistorted.  Three NaN where a pair holds a NaN.
 *   points1, points2 : float64 [n][2]
 *   n    : 0 .. 2^38
 *   geom : as above
 *   out  : float64 [n][3]
 * SSAMD_EINVAL: a NULL pointer, n outside the above, a non-finite entry of geom[40..67], a buffer not 8-byte aligned (device form).
 * n == 0 does nothing. */
int ssamd_stereo_triangulate(const double *points1, const double *points2, long long n, const double *geom, double *out, int device);
int ssamd_stereo_triangulate_device(const double *d_points1, const double *d_points2, long long n, const double *geom, double *d_out,
                                    void *stream);

/* The whole chain on host buffers: the decode of both stacks (arguments as in ssamd_graycode_decode, camera 1 then camera 2; n,
 * ncol, nrow, the projector and white_thr are common), match, offsets, cloud.
 *   dense   : 0: out receives the *npoints points in projector raster order; otherwise out is [proj_h][proj_w][3] with NaN
 *   out     : float64, room for proj_w * proj_h * 3 values in either case
 *   npoints : the number of matched cells
 * SSAMD_EINVAL: as ssamd_graycode_decode for either camera, as the two functions above, a NULL out or npoints. */
int ssamd_graycode_stereo_points(const uint8_t *planes1, int hc1, int wc1, const float *mapx1, const float *mapy1, int x1, int y1, int h1, int w1,
                                 const uint8_t *planes2, int hc2, int wc2, const float *mapx2, const float *mapy2, int x2, int y2, int h2, int w2,
                                 int n, int ncol, int nrow, int proj_w, int proj_h, int white_thr, int reduce, const double *geom, int dense,
                                 double *out, int *npoints, int device);

#ifdef __cplusplus
}
#endif
#endif /* SSAMD_GRAYCODE_STEREO_H */
