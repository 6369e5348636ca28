// K10: wrapped phase of Fourier-transform profilometry -- the demodulation of the reference's StereoFTP.getCloud
// (simplestereo/active.py:675-737; pure numpy there): gray = max over B, G, R; a row-wise FFT of the object image and of the
// reference image; a per-row band-pass around the carrier; an inverse FFT; angle(ghat * conj(g0hat)).
//
// A band-limited direct DFT, one workgroup per image row.  The band-pass keeps K = shi - slo + 1 bins of a row (about
// 2 * radius_factor * fc * w: some 100 of 1920), so only those are ever computed:
//   forward   G[s]    = sum_x g[x] e^{-2 pi i s x / w}      for the K kept bins       2 FMAs per term and image
//   backward  ghat[x] = sum_s G[s] e^{+2 pi i s x / w}      for the w columns         4 FMAs per term and image
// (numpy's 1/w of the inverse is positive and does not move the angle).  2 K w terms per row and image instead of the
// ~5 w log2 w of two FFTs with their three trips through HBM; any width, no smooth-length restriction.  Both images go through
// the same workgroup and the conjugate product and atan2 are the epilogue: nothing but the phase is written.
//
// Twiddles: ONE fp64 table e^{2 pi i j / w}, j = 0 .. w-1, built on the device (ftp_twiddle_kernel: exact integer octant
// reduction, then sincospi on [0, 1/4] -- no host libm, no multiplicative recurrence), cached per (device, w) by the host and
// staged in LDS.  It is indexed by (s x) mod w, which both passes carry along in integers: one add and one conditional
// subtract per term.
//
// LDS (dynamic):  double2 tw[w] | double4 bins[FTP_BIN_CHUNK] (G re, im, G0 re, im) | uchar2 gray[w] (object, reference).
// Bands longer than FTP_BIN_CHUNK go through the bins buffer a chunk at a time; the column accumulators live in registers
// (CPT columns per thread, 4 doubles each), so the all-bins case (K = w) is correct, merely O(w^2) per row.
// Everything is fp64 on the VALU.
//
// ftp_carrier_kernel is the same transform of ONE image with angle(ghat) as the epilogue.  Both kernels are thin wrappers of one
// row body, ftp_dft_row<CPT, NIMG>, in which the number of images decides the LDS layout, the accumulators and the epilogue.
#pragma once
#include <type_traits>
#include "common.hip.h"

namespace ssamd {

// tw[j] = (cos, sin)(2 pi j / w).  8 j = o w + r splits the turn into octants exactly; the odd octants are reflected, so the
// argument handed to sincospi is r' / (4 w) in [0, 1/4] with one rounding, and the axes and diagonals come out exact.
__global__ void ftp_twiddle_kernel(double2 *__restrict__ tw, int w)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= w) return;
    const int q = 8 * j;                                 // w <= 8192: no overflow
    const int o = q / w;
    int r = q - o * w;
    if (o & 1) r = w - r;
    double s0, c0;
    sincospi((double)r / (4.0 * (double)w), &s0, &c0);
    double c, s;
    switch (o) {
    case 0: c = c0; s = s0; break;
    case 1: c = s0; s = c0; break;
    case 2: c = -s0; s = c0; break;
    case 3: c = -c0; s = s0; break;
    case 4: c = -c0; s = -s0; break;
    case 5: c = -s0; s = -c0; break;
    case 6: c = s0; s = -c0; break;
    default: c = c0; s = -s0; break;
    }
    tw[j] = make_double2(c, s);
}

__device__ __forceinline__ unsigned char ftp_gray(const uint8_t *__restrict__ row, int ch, int x)
{
    if (ch == 1) return row[x];
    const uint8_t *p = row + 3 * (size_t)x;
    return max(max(p[0], p[1]), p[2]);                   // the reference's convertGrayscale: the channel maximum
}

// The row body of both DFT kernels, over NIMG images (2: object and reference, ftp_phase_kernel; 1: ftp_carrier_kernel): the
// empty-band row, the staging of the table and of the gray row(s), the running indexes, the chunked forward pass with its lane-group
// reduction, the backward pass and the angle.  The second image's variables (g0, hr, hi, G0, br, bi) are declared either way, since
// the discarded branches name them, but only the `if constexpr (PAIR)` statements read or update them: with one image they are dead
// and take no register (the one-image instances keep the VGPR and SGPR counts they had as a kernel of their own).  Per image the
// floating-point operations and their order do not depend on NIMG.
// One workgroup per row; blockDim.x = a multiple of 64 with CPT * blockDim.x >= w.  band[row] = (slo, shi), the kept signed
// bins (slo > shi: none).  lanes_per_bin: a power of two in 4 .. 64 (ftp_plan.h).  ref and ch_ref are not read with one image.
// LDS (dynamic, ftp_geometry of ftp_plan.h):  double2 tw[w] | double2 bins[bin_chunk][NIMG] (G re, im; then G0 re, im) |
// uchar2 gray[w] (object, reference) with two images, uint8 gray[w] with one.
template <int CPT, int NIMG>
__device__ __forceinline__ void ftp_dft_row(const uint8_t *obj, int ch_obj, const uint8_t *ref, int ch_ref, int w, const int2 *band,
                                            const double2 *tw_g, int lanes_per_bin, int bin_chunk, double *out)
{
    static_assert(NIMG == 1 || NIMG == 2, "one image or a pair");
    constexpr bool PAIR = NIMG == 2;
    using Gray = std::conditional_t<PAIR, uchar2, uint8_t>;
    extern __shared__ double2 ftp_lds[];
    double2 *tw = ftp_lds;
    double2 *bins = ftp_lds + w;
    Gray *gray = reinterpret_cast<Gray *>(bins + NIMG * bin_chunk);
    const int T = blockDim.x, tid = threadIdx.x;
    const size_t row = blockIdx.x;
    double *orow = out + row * (size_t)w;
    const int2 bd = band[row];
    const int K = bd.y - bd.x + 1;
    if (K <= 0) {                                        // np.angle(0j): exactly 0.0
        for (int x = tid; x < w; x += T) orow[x] = 0.0;
        return;
    }

    const uint8_t *po = obj + row * (size_t)w * ch_obj;
    const uint8_t *pr = PAIR ? ref + row * (size_t)w * ch_ref : nullptr;
    for (int x = tid; x < w; x += T) {
        tw[x] = tw_g[x];
        if constexpr (PAIR) gray[x] = make_uchar2(ftp_gray(po, ch_obj, x), ftp_gray(pr, ch_ref, x));
        else gray[x] = ftp_gray(po, ch_obj, x);
    }

    // columns of this thread and their running index (s x) mod w, started at s = slo
    const int sm0 = bd.x < 0 ? bd.x + w : bd.x;          // slo mod w
    int xs[CPT], js[CPT];
    double ar[CPT], ai[CPT], br[CPT], bi[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        const int x = tid + c * T;
        xs[c] = x < w ? x : 0;                           // columns past the row idle on tw[0]
        js[c] = (int)(((long long)sm0 * xs[c]) % w);
        ar[c] = ai[c] = br[c] = bi[c] = 0.0;
    }
    const int Q = lanes_per_bin;
    const int grp = tid / Q, seg = tid % Q, ngrp = T / Q;
    __syncthreads();

    for (int k0 = 0; k0 < K; k0 += bin_chunk) {
        const int kc = min(bin_chunk, K - k0);
        // ---- forward: the bins k0 .. k0 + kc - 1, Q lanes per bin, each over the columns seg, seg + Q, ...
        for (int b0 = 0; b0 < kc; b0 += ngrp) {
            const int b = b0 + grp;
            const bool live = b < kc;                    // uniform over a lane group; the shuffles below run for every lane
            int sm = bd.x + k0 + (live ? b : 0);
            sm = sm < 0 ? sm + w : sm;
            int j = (int)(((long long)sm * seg) % w);
            const int step = (int)(((long long)sm * Q) % w);
            double gr = 0.0, gi = 0.0, hr = 0.0, hi = 0.0;
            if (live) {
                for (int x = seg; x < w; x += Q) {
                    const double2 t = tw[j];
                    const Gray p = gray[x];
                    double g, g0 = 0.0;
                    if constexpr (PAIR) { g = (double)p.x; g0 = (double)p.y; }
                    else g = (double)p;
                    gr = fma(g, t.x, gr);
                    gi = fma(g, t.y, gi);
                    if constexpr (PAIR) {
                        hr = fma(g0, t.x, hr);
                        hi = fma(g0, t.y, hi);
                    }
                    j += step;
                    j -= j >= w ? w : 0;
                }
            }
            for (int o = Q >> 1; o > 0; o >>= 1) {
                gr += __shfl_xor(gr, o);
                gi += __shfl_xor(gi, o);
                if constexpr (PAIR) {
                    hr += __shfl_xor(hr, o);
                    hi += __shfl_xor(hi, o);
                }
            }
            if (live && seg == 0) {                      // e^{-i theta}: the imaginary part changes sign
                bins[NIMG * b] = make_double2(gr, -gi);
                if constexpr (PAIR) bins[2 * b + 1] = make_double2(hr, -hi);
            }
        }
        __syncthreads();
        // ---- backward: every column adds the kc bins; from one bin to the next (s x) mod w moves by x
#pragma unroll 2
        for (int b = 0; b < kc; ++b) {
            const double2 G = bins[NIMG * b];
            double2 G0;
            if constexpr (PAIR) G0 = bins[2 * b + 1];
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                const double2 t = tw[js[c]];
                ar[c] = fma(G.x, t.x, ar[c]);
                ar[c] = fma(-G.y, t.y, ar[c]);
                ai[c] = fma(G.x, t.y, ai[c]);
                ai[c] = fma(G.y, t.x, ai[c]);
                if constexpr (PAIR) {
                    br[c] = fma(G0.x, t.x, br[c]);
                    br[c] = fma(-G0.y, t.y, br[c]);
                    bi[c] = fma(G0.x, t.y, bi[c]);
                    bi[c] = fma(G0.y, t.x, bi[c]);
                }
                js[c] += xs[c];
                js[c] -= js[c] >= w ? w : 0;
            }
        }
        __syncthreads();
    }

    // ---- angle(ghat * conj(g0hat)) of a pair, angle(ghat) of one image
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        const int x = tid + c * T;
        if (x < w) {
            if constexpr (PAIR) {
                const double zr = fma(ar[c], br[c], ai[c] * bi[c]);
                const double zi = fma(ai[c], br[c], -(ar[c] * bi[c]));
                orow[x] = atan2(zi, zr);
            } else {
                orow[x] = atan2(ai[c], ar[c]);
            }
        }
    }
}

// Wrapped phase of an object image against a reference image, angle(ghat * conj(g0hat)): the header of this file.
template <int CPT>
__global__ __launch_bounds__(1024) void ftp_phase_kernel(const uint8_t *__restrict__ obj, int ch_obj, const uint8_t *__restrict__ ref,
                                                         int ch_ref, int w, const int2 *__restrict__ band,
                                                         const double2 *__restrict__ tw_g, int lanes_per_bin, int bin_chunk,
                                                         double *__restrict__ out)
{
    ftp_dft_row<CPT, 2>(obj, ch_obj, ref, ch_ref, w, band, tw_g, lanes_per_bin, bin_chunk, out);
}

// Wrapped phase of ONE fringe image, np.angle(ifft(bandpass(fft(gray)))): the demodulation of the reference's
// StereoFTP_Mapping.getCloud (active.py:1354-1401) and the second and third result of StereoFTP_PhaseOnly.getPhase (:2067-2074).
// The same band, table, lane groups and running indexes as the pair, half the accumulators, and the angle of ghat itself.
template <int CPT>
__global__ __launch_bounds__(1024) void ftp_carrier_kernel(const uint8_t *__restrict__ img, int ch, int w, const int2 *__restrict__ band,
                                                           const double2 *__restrict__ tw_g, int lanes_per_bin, int bin_chunk,
                                                           double *__restrict__ out)
{
    ftp_dft_row<CPT, 1>(img, ch, nullptr, 0, w, band, tw_g, lanes_per_bin, bin_chunk, out);
}

}  // namespace ssamd
