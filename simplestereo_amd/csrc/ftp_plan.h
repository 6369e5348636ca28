// Host planner of the Fourier-profilometry phase kernel (ftp_kernels.hip.h): which DFT bins a row keeps, and the launch shape.
// Pure arithmetic, like asw_plan.h and gsw_plan.h (host_context.h, a host section of ssamd_api.hip, is the only file that includes it); needs no device.
//
// The reference masks the spectrum with numpy (active.py:681-722):
//     freqs = np.fft.fftfreq(w);  G[(freqs - fmin) < 0] = 0;  G[(freqs - fmax) > 0] = 0
// np.fft.fftfreq(w) is the INTEGER bin index times the double 1.0 / w -- two roundings, not s / w -- for the signed indices
// s = 0 .. (w-1)/2, -(w/2) .. -1 (the Nyquist bin of an even w is s = -w/2).  Bin s is kept iff
//     !(f(s) - fmin < 0) && !(f(s) - fmax > 0),      f(s) = (double)s * (1.0 / (double)w)
// so a NaN bound masks nothing on its side.  f is non-decreasing in s and so is a rounded difference with a constant: the
// kept bins are one contiguous signed range [slo, shi] (empty: slo > shi), found by two bisections.
#pragma once

// the two halves of the predicate; a fused multiply-add would skip the rounding of s * inv and move a band edge by one bin
inline bool ftp_not_below(int s, double inv, double fmin)
{
#pragma clang fp contract(off)
    const double f = (double)s * inv;
    const double d = f - fmin;
    return !(d < 0);
}
inline bool ftp_not_above(int s, double inv, double fmax)
{
#pragma clang fp contract(off)
    const double f = (double)s * inv;
    const double d = f - fmax;
    return !(d > 0);
}

// kept signed bins of one row of width w >= 1: [slo, shi], slo > shi when the band is empty
inline void ftp_band_row(int w, double fmin, double fmax, int32_t &slo, int32_t &shi)
{
    const double inv = 1.0 / (double)w;
    const int smin = -(w / 2), smax = (w - 1) / 2;
    int a = smin, b = smax + 1;                 // first s in [smin, smax + 1] that is not below fmin
    while (a < b) {
        const int m = a + (b - a) / 2;
        if (ftp_not_below(m, inv, fmin)) b = m; else a = m + 1;
    }
    slo = a;
    a = smin - 1; b = smax;                     // last s in [smin - 1, smax] that is not above fmax
    while (a < b) {
        const int m = b - (b - a) / 2;
        if (ftp_not_above(m, inv, fmax)) a = m; else b = m - 1;
    }
    shi = a;
    if (slo > shi) { slo = 0; shi = -1; }       // one spelling of "empty"
}

// Launch shape for rows of w columns of `images` images (2: ftp_phase_kernel, 1: ftp_carrier_kernel): CPT output columns per
// thread (the kernel's template argument), threads per workgroup (whole waves, at most FTP_THREADS_MAX), dynamic LDS bytes.
struct FtpGeom { int cpt, threads, lds_bytes; };

constexpr int FTP_MAX_W = 8192;                 // twiddles 16 w + gray pairs 2 w + a chunk of bins: 148 KiB of the 160 KiB
constexpr int FTP_THREADS_MAX = 1024;
constexpr int FTP_BIN_CHUNK = 128;              // bins held in LDS at a time (16 bytes each and image)

// LDS of ftp_dft_row: twiddles 16 w, a chunk of bins of 16 bytes per image, gray bytes w per image (148 KiB with two images at
// FTP_MAX_W, 138 KiB with one)
inline FtpGeom ftp_geometry(int w, int images)
{
    FtpGeom g;
    g.cpt = w <= 1024 ? 1 : w <= 2048 ? 2 : w <= 4096 ? 4 : 8;
    g.threads = (((w + g.cpt - 1) / g.cpt) + 63) / 64 * 64;
    g.lds_bytes = 16 * w + 16 * images * FTP_BIN_CHUNK + ((images * w + 15) & ~15);
    return g;
}

// lanes of a wave that share one bin in the forward pass (a power of two, 4 .. 64): as few as still give every bin of a
// chunk a lane group in one round, so short bands keep all lanes busy and long ones need few reduction steps
inline int ftp_lanes_per_bin(int threads, int max_bins)
{
    const int bins = max_bins < FTP_BIN_CHUNK ? max_bins : FTP_BIN_CHUNK;
    int q = 64;
    while (q > 4 && (threads / q) < bins) q >>= 1;
    return q;
}
