// K0: BGR u8 -> pixel records {L,a,b,bgrx}.  Pointwise, HBM-bound (3 B in, 16 B out
// per pixel).  Replaces ColorConversion::ImageFromBGR2Lab
// (reference headers/colorconversion.hpp:18-86, called at _passive.cpp:337-341).
#pragma once
#include "common.hip.h"
#include "glibc_math.hip.h"

namespace ssamd {

// sRGB byte -> linear*100 (colorconversion.hpp:19-37).  The transfer curve only
// depends on the byte, so it is a 256-entry table filled once by the host.
__constant__ float c_lin100[256];

// CIE f(t) with the reference's precision mix: float powf above the knee, double linear segment below
// (colorconversion.hpp:55-65).  Round 5: powf is glibc's own algorithm restated (glibc_math.hip.h: table-driven log2 / exp2 in
// double, one rounding to float) and returns the SAME float as the libm the reference links for every argument the conversion can
// produce -- checked exhaustively on the host (oracle/libm_check.c) -- so the records hold exactly the reference's Lab values
// rounded to float, and the fp64 tie-break pass the reference's doubles.  (Rounds 2-4 computed a correctly rounded cube root by
// Newton steps: 99.90 % of the floats were glibc's, whose powf is within 0.82 ulp but not correctly rounded.)

// The conversion's three lookup tables (sRGB byte -> linear * 100; glibc powf's log2 and exp2 tables) staged in LDS by the
// record-producing kernels: 1.5 KB, indexed per lane.
struct LabTables {
    const float *lin100;
    const double *log2tab;
    const uint64_t *exp2tab;
};
#define SSAMD_LAB_TABLES_IN_LDS(name)                                                                          \
    __shared__ float name##_lin[256];                                                                          \
    __shared__ double name##_log2[32];                                                                         \
    __shared__ uint64_t name##_exp2[32];                                                                       \
    for (int k_ = threadIdx.x; k_ < 256; k_ += blockDim.x) name##_lin[k_] = c_lin100[k_];                      \
    for (int k_ = threadIdx.x; k_ < 32; k_ += blockDim.x) { name##_log2[k_] = gm_powf_log2_tab[k_]; name##_exp2[k_] = gm_exp2f_tab[k_]; } \
    __syncthreads();                                                                                           \
    const LabTables name{name##_lin, name##_log2, name##_exp2};

__device__ __forceinline__ double lab_f(double t, const LabTables &T)
{
#pragma clang fp contract(off)
    if (t > 0.008856) return (double)glibc_powf_pos_t((float)t, (float)(1 / 3.0), T.log2tab, T.exp2tab);
    return (7.787 * t) + (16.0 / 116.0);
}

// The reference's Lab values are DOUBLES (colorconversion.hpp:67-69: 116 * y - 16 ... on doubles that hold float powf results);
// the aggregation kernels use them rounded to float, the fp64 tie-break pass (asw_exact_kernels.hip.h) as they are.
__device__ __forceinline__ void bgr_to_lab_f64(uint32_t B, uint32_t G, uint32_t R, double &L, double &a, double &b, const LabTables &T)
{
#pragma clang fp contract(off)           // (the reference is a plain x86-64 build: no fused multiply-adds in its matrix and affine steps)
    const float r = T.lin100[R], g = T.lin100[G], bl = T.lin100[B];
    // observer 2 deg / D65 matrix in fp64 (colorconversion.hpp:40-42)
    const double X = r * 0.4124 + g * 0.3576 + bl * 0.1805;
    const double Y = r * 0.2126 + g * 0.7152 + bl * 0.0722;
    const double Z = r * 0.0193 + g * 0.1192 + bl * 0.9505;
    const float refX = 95.047f, refY = 100.0f, refZ = 108.883f;   // float constants, :48
    const double fx = lab_f(X / refX, T), fy = lab_f(Y / refY, T), fz = lab_f(Z / refZ, T);
    L = 116 * fy - 16;
    a = 500 * (fx - fy);
    b = 200 * (fy - fz);
}

__device__ __forceinline__ void bgr_to_lab(uint32_t B, uint32_t G, uint32_t R, float &L, float &a, float &b, const LabTables &T)
{
    double L64, a64, b64;
    bgr_to_lab_f64(B, G, R, L64, a64, b64, T);
    L = (float)L64;
    a = (float)a64;
    b = (float)b64;
}

// The pixel front of the matchers, each step written once.
// Pixel p of a uint8 [npix][3] image as B | G << 8 | R << 16.  4 consecutive pixels share 12 contiguous bytes but a 3-byte-per-lane
// read is still fully coalesced at the wave level (192 B/wave): one unaligned 4-byte read instead of three byte reads (the 4th byte
// is the next pixel's); byte reads for the last pixel, whose 4-byte read would run one byte past the buffer.
__device__ __forceinline__ uint32_t load_bgr(const uint8_t *__restrict__ img, long long p, long long npix)
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    const uint8_t *const b = img + 3 * p;
    return p + 1 < npix ? (*reinterpret_cast<const u32_unaligned *>(b) & 0xffffffu)
                        : ((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16));
}

// packed pixel -> record: its Lab values and the bytes themselves
__device__ __forceinline__ PixRec lab_record(uint32_t bgr, const LabTables &T)
{
    PixRec o;
    bgr_to_lab(bgr & 0xff, (bgr >> 8) & 0xff, (bgr >> 16) & 0xff, o.L, o.a, o.b, T);
    o.bgrx = bgr;
    return o;
}

// The records of an image pair by the `blocks` workgroups of one launch: item q of 2 * npix -> (right image?, pixel p), whose
// packed pixel is pixel(right, p).
// Both images of a pair in ONE launch (round 3: a 1080p image is a 20 us kernel, two of them plus the gap between two
// dependent launches were a third of the pre-pass; at Tsukuba size the launch is most of it).
// (The two remap kernels of rig_kernels.hip.h walk their pair with a loop of their own: through this function their device
// code changed, profiles/fp32_steps_fold.txt.)
template <class F>
__device__ __forceinline__ void lab_records_pair(PixRec *__restrict__ recL, PixRec *__restrict__ recR, long long npix, unsigned blocks,
                                                 const LabTables &T, F pixel)
{
    long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)blocks * blockDim.x;
    for (; q < 2 * npix; q += stride) {
        const bool right = q >= npix;
        const long long p = right ? q - npix : q;
        (right ? recR : recL)[p] = lab_record(pixel(right, p), T);
    }
}

__global__ __launch_bounds__(256) void bgr2lab_records_pair_kernel(const uint8_t *__restrict__ bgrL, const uint8_t *__restrict__ bgrR,
                                                                   PixRec *__restrict__ recL, PixRec *__restrict__ recR, long long npix)
{
    SSAMD_LAB_TABLES_IN_LDS(T)
    lab_records_pair(recL, recR, npix, gridDim.x, T, [&](bool right, long long p) { return load_bgr(right ? bgrR : bgrL, p, npix); });
}

// debug/verification: plain float32 Lab image
__global__ __launch_bounds__(256) void bgr2lab_f32_kernel(const uint8_t *__restrict__ bgr,
                                                          float *__restrict__ lab, long long npix)
{
    SSAMD_LAB_TABLES_IN_LDS(T)
    long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; p < npix; p += stride) {
        const PixRec o = lab_record(load_bgr(bgr, p, npix), T);
        lab[3 * p] = o.L;
        lab[3 * p + 1] = o.a;
        lab[3 * p + 2] = o.b;
    }
}

}  // namespace ssamd
