// The front end of StereoFTP.getCloud on the device: the virtual reference image of _getProjectorMapping (active.py:459-490,
// the integer-grid half: cv2.projectPoints of every camera pixel, float32 maps, cv2.remap(INTER_CUBIC) of the fringe) and the
// per-row centroid of findCentralStripe (:305-333).
//
// ftp_reference_kernel, per output pixel (x, y): u = x + x0, v = y + y0 (integer coordinates: no + 0.5 here), ftp_project of
// (u, v, 1) in fp64 with the operations of tests/_ftp_cloud_ref.py (shared with ftp_cloud_kernel), both coordinates rounded to
// float32, then OpenCV's published 8-bit bicubic arithmetic (modules/imgproc/src/imgwarp.cpp, remap / remapBicubic /
// initInterTab2D): q = rint(map * 32) (half to even), cell = q >> 5, fraction = q & 31, the 4 x 4 taps at cell - 1 .. cell + 2
// weighted by the 16 shorts of table entry [fy][fx] (15-bit fixed point, each entry sums to 32768; built on the host,
// host_ftp_reference.h), taps outside the fringe contribute the border value 0, result clip((sum + (1 << 14)) >> 15, 0, 255).
// NaN, +-inf and coordinates of 2^26 and beyond give 0 (remap_pixel's rule).  All of it after the float32 cast is integer
// arithmetic: the output equals tests/_stereo_ftp_ref.py byte for byte.
//
// The 32 KiB table is staged in LDS once per workgroup (a lane reads its 32 bytes as two ds_read_b128); the fringe is read
// through the caches as four unaligned 4-byte rows per pixel (projector-sized: it sits in L2).  A thread owns four consecutive
// output pixels of the flattened map (npix = h w < 2^31: rows are not a grid dimension) and writes them as one 4-byte store.
#pragma once
#include "common.hip.h"
#include "ftp_cloud_kernels.hip.h"

namespace ssamd {

constexpr int FTP_REF_THREADS = 512;
constexpr int FTP_REF_TAB = 32 * 32 * 16;       // shorts: [fy][fx][tap row][tap column]

// what ftp_project reads: the first 28 doubles of the SSAMD_FTP_CLOUD_NGEOM block
struct FtpProjGeom {
    double M[9];
    double T[3];
    double f2[4];
    double d[12];
};
static_assert(sizeof(FtpProjGeom) == 28 * sizeof(double) && offsetof(FtpCloudGeom, P) == sizeof(FtpProjGeom), "the head of FtpCloudGeom");

// One pixel of cv2.remap(fringe, mapx, mapy, INTER_CUBIC) for a gray uint8 fringe [Hp][Wp], BORDER_CONSTANT 0.
__device__ __forceinline__ uint32_t remap_cubic_pixel(const uint8_t *__restrict__ fr, int Hp, int Wp, const short *tab, float mx, float my)
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    if (!(fabsf(mx) < 0x1p26f && fabsf(my) < 0x1p26f)) return 0u;          // NaN, +-inf, map * 32 outside int32
    const int qx = (int)rint((double)mx * 32.0), qy = (int)rint((double)my * 32.0);
    const int x0 = (qx >> 5) - 1, y0 = (qy >> 5) - 1;                       // the first tap
    if (x0 >= Wp || x0 + 4 <= 0 || y0 >= Hp || y0 + 4 <= 0) return 0u;     // no tap inside the fringe
    const short *const wt = tab + ((((qy & 31) << 5) | (qx & 31)) << 4);
    short w[16];
    *reinterpret_cast<int4 *>(w) = *reinterpret_cast<const int4 *>(wt);
    *reinterpret_cast<int4 *>(w + 8) = *reinterpret_cast<const int4 *>(wt + 8);
    int sum = 0;
    if (x0 >= 0 && x0 + 3 < Wp && y0 >= 0 && y0 + 3 < Hp) {
        const uint8_t *s = fr + ((size_t)y0 * Wp + x0);
#pragma unroll
        for (int r = 0; r < 4; ++r, s += Wp) {
            const uint32_t v = *reinterpret_cast<const u32_unaligned *>(s);
            sum += (int)(v & 0xff) * w[4 * r] + (int)((v >> 8) & 0xff) * w[4 * r + 1] + (int)((v >> 16) & 0xff) * w[4 * r + 2] +
                   (int)(v >> 24) * w[4 * r + 3];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int xx = x0 + c, yy = y0 + r;
                if (xx >= 0 && xx < Wp && yy >= 0 && yy < Hp) sum += (int)fr[(size_t)yy * Wp + xx] * w[4 * r + c];
            }
    }
    const int v = (sum + (1 << 14)) >> 15;
    return (uint32_t)min(max(v, 0), 255);
}

template <int MODEL>
__device__ __forceinline__ uint32_t ftp_reference_pixel(const FtpProjGeom &G, const uint8_t *__restrict__ fr, int Hp, int Wp,
                                                        const short *tab, unsigned int xx, unsigned int yy, int x0, int y0)
{
    double Xa, Ya;
    ftp_project<MODEL>(G, (double)xx + (double)x0, (double)yy + (double)y0, Xa, Ya);
    return remap_cubic_pixel(fr, Hp, Wp, tab, (float)Xa, (float)Ya);
}

// fringe [Hp][Wp] -> out [h][w] (ROI origin x0, y0 in the camera image); d_tab: the FTP_REF_TAB shorts, 16-byte aligned;
// out 4-byte aligned.
template <int MODEL>
__global__ __launch_bounds__(FTP_REF_THREADS) void ftp_reference_kernel(const uint8_t *__restrict__ fr, int Hp, int Wp,
                                                                        const short *__restrict__ d_tab, uint8_t *__restrict__ out,
                                                                        long long npix, int w, int x0, int y0, const FtpProjGeom G)
{
    __shared__ __attribute__((aligned(16))) short tab[FTP_REF_TAB];
    for (int i = threadIdx.x; i < FTP_REF_TAB / 8; i += FTP_REF_THREADS)
        reinterpret_cast<int4 *>(tab)[i] = reinterpret_cast<const int4 *>(d_tab)[i];
    __syncthreads();
    const long long nquad = npix >> 2;
    const long long tid = (long long)blockIdx.x * FTP_REF_THREADS + threadIdx.x, stride = (long long)gridDim.x * FTP_REF_THREADS;
    for (long long q = tid; q < nquad; q += stride) {
        const unsigned int p = (unsigned int)(4 * q);
        unsigned int yy = p / (unsigned int)w, xx = p - yy * (unsigned int)w;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v |= ftp_reference_pixel<MODEL>(G, fr, Hp, Wp, tab, xx, yy, x0, y0) << (8 * k);
            if (++xx == (unsigned int)w) { xx = 0; ++yy; }
        }
        reinterpret_cast<uint32_t *>(out)[q] = v;
    }
    for (long long p = 4 * nquad + tid; p < npix; p += stride) {
        const unsigned int yy = (unsigned int)p / (unsigned int)w, xx = (unsigned int)p - yy * (unsigned int)w;
        out[p] = (uint8_t)ftp_reference_pixel<MODEL>(G, fr, Hp, Wp, tab, xx, yy, x0, y0);
    }
}

// findCentralStripe's per-row centroid (active.py:319-333): of row y of a BGR uint8 image [h][w][3], channel `ch`, the values
// below `threshold` count as 0 (the reference's `fringe < maxValue * sensitivity`, an fp64 comparison: the caller passes the
// integer threshold equivalent to it, ceil of the product); out[y] = sum(v * x) / sum(v), the sums exact 64-bit integers
// (255 W^2 / 2 passes 2^32 beyond W = 5800), one fp64 division: numpy's result bit for bit, NaN (0 / 0) for a row without stripe.
// One wave per row, four rows per workgroup.
constexpr int STRIPE_THREADS = 256;
__global__ __launch_bounds__(STRIPE_THREADS) void stripe_centroid_kernel(const uint8_t *__restrict__ img, int h, int w, int ch,
                                                                         int threshold, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int nwave = gridDim.x * (STRIPE_THREADS / 64);
    for (int y = blockIdx.x * (STRIPE_THREADS / 64) + (threadIdx.x >> 6); y < h; y += nwave) {
        const uint8_t *const row = img + (size_t)y * w * 3 + ch;
        unsigned long long sv = 0, svx = 0;
        for (int x = lane; x < w; x += 64) {
            const unsigned int v = row[3 * (size_t)x];
            if ((int)v >= threshold) { sv += v; svx += (unsigned long long)v * (unsigned int)x; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sv += __shfl_xor(sv, m, 64);
            svx += __shfl_xor(svx, m, 64);
        }
        if (lane == 0) out[y] = (double)svx / (double)sv;
    }
}

}  // namespace ssamd
