/*
 * ssamd_active.h -- second public header of libssamd.so: the front end of Fourier-transform profilometry
 * (simplestereo/active.py, class StereoFTP), beside the operators of ssamd.h (ssamd_ftp_phase, ssamd_ftp_cloud).
 *
 *   ssamd_ftp_reference     <->  the virtual reference image of StereoFTP._getProjectorMapping   active.py:459-490
 *                                (cv2.projectPoints of the integer pixel grid + cv2.remap(INTER_CUBIC) in the reference)
 *   ssamd_stripe_centroids  <->  the per-row centroid of findCentralStripe                       active.py:305-333
 *
 * Same library, same conventions as ssamd.h: int return codes (SSAMD_OK, SSAMD_E*), the message of ssamd_last_error, `device` = -1 for the
 * calling thread's current device, NAME takes host buffers and is synchronous, NAME_device takes device buffers and is
 * asynchronous on `stream`.  No CPU fallback.  This header has a version of its own; SSAMD_ABI_VERSION does not move with it.
 */
#ifndef SSAMD_ACTIVE_H
#define SSAMD_ACTIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAMD_ACTIVE_VERSION 1

/* Virtual reference image: what the camera would see of `fringe` on the reference plane (active.py:459-490).  For the output
 * pixel (x, y): u = x + x0, v = y + y0 (integer coordinates, no + 0.5), projectPoints of (u, v, 1) in fp64 exactly as
 * ssamd_ftp_cloud does it, both coordinates rounded to float32, then cv2.remap(..., INTER_CUBIC, BORDER_CONSTANT 0) for 8-bit
 * images: q = rint(map * 32) to even, cell q >> 5, fraction q & 31, the 4 x 4 taps at cell - 1 .. cell + 2 with the 15-bit
 * integer weights of OpenCV's initInterTab2D(INTER_CUBIC), taps outside the fringe 0, clip((sum + (1 << 14)) >> 15, 0, 255).
 * NaN, +-inf and coordinates whose product with 32 leaves int32 give 0.  One HIP kernel (csrc/ftp_reference_kernels.hip.h);
 * equal byte for byte to the numpy restatement tests/_stereo_ftp_ref.py; parity with cv2 itself is not pinned.
 *   fringe : uint8 [hp][wp], gray; hp, wp >= 1, hp * wp < 2^31
 *   out    : uint8 [h][w], the region of interest whose upper left camera pixel is (x0, y0); h * w < 2^31
 *   geom   : HOST array of SSAMD_FTP_CLOUD_NGEOM doubles (layout in ssamd.h), consumed before the call returns; only
 *            [0..27] are read: M, T, fx2 fy2 cx2 cy2, the twelve distortion coefficients -- and must be finite
 * SSAMD_EINVAL: a NULL pointer, a negative size or origin, an empty fringe, a size of 2^31 pixels or more, a non-finite entry of
 * geom[0..27], an output buffer not 4-byte aligned (device form).  An empty map does nothing. */
int ssamd_ftp_reference(const uint8_t *fringe, int hp, int wp, int h, int w, int x0, int y0, const double *geom, uint8_t *out,
                        int device);
int ssamd_ftp_reference_device(const uint8_t *d_fringe, int hp, int wp, int h, int w, int x0, int y0, const double *geom,
                               uint8_t *d_out, void *stream);

/* Per-row centroid of one colour channel (active.py:319-333): in row y of the BGR image, values below `threshold` count as 0,
 * out[y] = sum(v * x) / sum(v) with exact 64-bit integer sums and one fp64 division -- numpy's result bit for bit; NaN for a
 * row in which every value is below the threshold.  The reference compares uint8 against the fp64 product maxValue *
 * sensitivity; the caller passes the integer equivalent, ceil(255 * sensitivity).
 *   img       : uint8 [h][w][3], BGR
 *   channel   : 0, 1 or 2
 *   threshold : 0 .. 256
 *   out       : fp64 [h]
 * SSAMD_EINVAL: a NULL pointer, a negative size, h * w * 3 >= 2^40, a channel or a threshold outside its range.  An image
 * without rows or without columns does nothing. */
int ssamd_stripe_centroids(const uint8_t *img, int h, int w, int channel, int threshold, double *out, int device);
int ssamd_stripe_centroids_device(const uint8_t *d_img, int h, int w, int channel, int threshold, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAMD_ACTIVE_H */
