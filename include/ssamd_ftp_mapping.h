/*
 * ssamd_ftp_mapping.h -- fourth public header of libssamd.so: Fourier-transform profilometry without a reference plane
 * (simplestereo/active.py, classes StereoFTP_Mapping and StereoFTP_PhaseOnly), beside ssamd.h, ssamd_active.h and ssamd_graycode.h.
 *
 *   ssamd_ftp_carrier_phase  <->  np.angle(np.fft.ifft(bandpass(np.fft.fft(gray))))                active.py:1354-1401, :2067-2074
 *   ssamd_ftp_mapping_cloud  <->  phase -> projector column, _triangulate of every pixel           active.py:1436-1447, :561-605
 *
 * Same library, same conventions as ssamd.h: int return codes (SSAMD_OK, SSAMD_E*), the message of ssamd_last_error, `device` = -1 for the
 * calling thread's current device, NAME takes host buffers and is synchronous, NAME_device takes device buffers and is
 * asynchronous on `stream`.  No CPU fallback.  This header has a version of its own; SSAMD_ABI_VERSION does not move with it.
 */
#ifndef SSAMD_FTP_MAPPING_H
#define SSAMD_FTP_MAPPING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAMD_FTP_MAPPING_VERSION 1

/* Wrapped phase of one fringe image: gray by the channel maximum, and per row the angle of the inverse transform of the
 * spectrum cut to the band [fmin[y], fmax[y]] (bins of np.fft.fftfreq(w), bounds included; ssamd_ftp_band tells which).  The
 * band-limited direct DFT of ssamd_ftp_phase on one image (csrc/ftp_kernels.hip.h, ftp_carrier_kernel): fp64, not bit-identical
 * to numpy's pocketfft, within a few ulp of pi of the exact angle wherever |ghat| is not tiny against its row.  A row whose
 * band holds no bin is exactly 0.0.
 *   img        : uint8 [h][w][ch], ch = 1 (gray) or 3 (BGR)
 *   fmin, fmax : HOST arrays of h doubles (in the device form too), consumed before the call returns
 *   unwrap     : 0 the wrapped phase; 1 ssamd_iir_unwrap of it with tau; 2 ssamd_np_unwrap_xy of it (np.unwrap along x, then
 *                along y); both on the same stream and equal bit for bit to the unwrapper called on the wrapped map
 *   tau        : 0 .. 1, read only with unwrap == 1
 *   out        : float64 [h][w]
 * SSAMD_EINVAL: a NULL pointer, h <= 0 or w <= 0, ch not 1 or 3, unwrap not 0, 1 or 2, what the unwrapper refuses.
 * SSAMD_ELIMIT: w > SSAMD_FTP_MAX_W (8192). */
int ssamd_ftp_carrier_phase(const uint8_t *img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau,
                            double *out, int device);
int ssamd_ftp_carrier_phase_device(const uint8_t *d_img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap,
                                   double tau, double *d_out, void *stream);

/* The point of every pixel of an unwrapped phase map whose upper left pixel is camera pixel (x0, y0).  Per pixel (x, y) of the map,
 * fp64, each operation rounded once (no fused multiply-adds, IEEE divisions):
 *   cx = ((double)x + 0.5) + x0;   cy = ((double)y + 0.5) + y0
 *   px = (((phase - theta) / two_pi_fp) + peak) + 0.5              with two_pi_fp = geom[39]
 *   l_i = (F[3 i] * cx + F[3 i + 1] * cy) + F[3 i + 2],  i = 0, 1, 2
 *   py = -((l_0 * px + l_2) / l_1)
 * and the point of the camera pixel centre (cx, cy) and the projector point (px, py): the operations of ssamd_ftp_cloud from
 * its undistortPoints on (cv2.undistortPoints(K2, distCoeffs2, P = K2), the two rectifying homographies, baseline / |disparity|,
 * the common rotation undone).  One HIP kernel (csrc/ftp_mapping_kernels.hip.h); equal bit for bit to the numpy restatement
 * tests/_ftp_mapping_ref.py, the non-finite values of a non-finite phase included.
 *   phase : float64 [h][w]; 16-byte aligned in the device form
 *   geom  : HOST array of SSAMD_FTP_CLOUD_NGEOM doubles (layout in ssamd.h), consumed before the call returns; only [12..36]
 *           (fx2 fy2 cx2 cy2, the twelve distortion coefficients, P), [39] (2 pi fp) and [40..67] (Rectify1, Rectify2, inv(commonR),
 *           the baseline) are read and must be finite; M, T and the epipole are not read (a rig with T[2] == 0 is fine)
 *   F     : HOST array of 9 doubles, the fundamental matrix row by row, finite
 *   theta, peak : finite
 *   out   : float64 [h][w][3]; 16-byte aligned in the device form
 * SSAMD_EINVAL: a NULL pointer, a negative size or origin, h * w of 2^31 or more, a non-finite value among those read, a
 * misaligned device buffer.  An empty map does nothing. */
int ssamd_ftp_mapping_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, const double *F, double theta,
                            double peak, double *out, int device);
int ssamd_ftp_mapping_cloud_device(const double *d_phase, int h, int w, int x0, int y0, const double *geom, const double *F,
                                   double theta, double peak, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAMD_FTP_MAPPING_H */
