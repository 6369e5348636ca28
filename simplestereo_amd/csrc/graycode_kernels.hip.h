// Gray-code structured light: the reference's GrayCode.getCloud (active.py:1174-1263), which calls
// cv2.structured_light_GrayCodePattern.getProjPixel once per camera pixel from a Python double loop and returns the valid
// points only, in raster order.  Three kernels:
//   graycode_decode_kernel  planes (+ the undistortion maps) -> (xDec, yDec) or (-1, -1) per pixel, valid pixels per block
//   graycode_scan_kernel    block counts -> exclusive prefix sum + total
//   graycode_cloud_kernel   decoded pixels (+ block offsets) -> points, compacted in raster order or dense with NaN
// The region's pixels are one flattened index p = ry * w + rx (npix = h w < 2^31), cut into blocks of GRAYCODE_BLOCK consecutive
// pixels: one workgroup per block, thread t owns the pixels 4 t .. 4 t + 3 of its block.  The decode and the cloud kernel use
// the same partition, so a valid pixel's place in the compacted output is offset[block] + its rank inside the block -- counted
// with ballots and popcounts within a wave and through LDS across the four waves: integers, plain stores, a fixed order, no
// atomics, the same output on every run.
// The decode's front is shared with phaseshift_decode_kernel (phaseshift_kernels.hip.h): PlaneStack, the arguments both begin
// with, and plane_stack_frame, which finds a thread's pixels, taps and window and the mode its planes are read in (graycode_fetch).
#pragma once
#include <type_traits>
#include "common.hip.h"
#include "ftp_cloud_kernels.hip.h"

namespace ssamd {

constexpr int GRAYCODE_THREADS = 256;
constexpr int GRAYCODE_WAVES = GRAYCODE_THREADS / 64;
constexpr int GRAYCODE_PER_THREAD = 4;
constexpr int GRAYCODE_BLOCK = GRAYCODE_THREADS * GRAYCODE_PER_THREAD;      // SSAMD_GRAYCODE_BLOCK of include/ssamd_graycode.h

// What every decoder of a plane stack is given: n gray planes of one camera, the undistortion maps they are sampled through (or
// none) and the region to decode.  GrayDecodeArgs and PhaseShiftArgs (phaseshift_kernels.hip.h) begin with it; plane_stack_check
// (host_graycode.h) fills it, plane_stack_frame reads it.
struct PlaneStack {
    const uint8_t *planes;          // [n][hc][wc]
    const float *mapx, *mapy;       // [hc][wc] undistortion maps (MAPS) or unused
    long long plane_stride;         // hc * wc < 2^31
    long long npix;                 // h * w < 2^31
    int hc, wc, x0, y0, w;
};

struct GrayDecodeArgs {
    PlaneStack stack;               // plane 2 k is bit k's pattern image, 2 k + 1 its inverse, columns first, MSB first
    int32_t *out;                   // [h][w][2]
    int32_t *counts;                // [ceil(npix / GRAYCODE_BLOCK)] or NULL
    int ncol, nrow, pw, ph, thr;    // bits per code, projector size, white threshold 0 .. 256
};

// The four taps of cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) on one 8-bit plane (remap_pixel of rig_kernels.hip.h, one
// channel): byte offsets inside a plane and the weights a b in 0 .. 1024, 0 for a tap outside the image (its offset is 0) and
// for map coordinates that are not finite or whose product with 32 leaves int32.  They depend on the pixel alone, not on the plane.
struct GrayTaps {
    uint32_t off[4];
    int wt[4];
    int cx, cy;         // the upper left tap's cell ...
    bool interior;      // ... if all four taps lie inside the image
};

__device__ __forceinline__ GrayTaps graycode_taps(float mx, float my, int hc, int wc)
{
    GrayTaps t;
#pragma unroll
    for (int i = 0; i < 4; ++i) { t.off[i] = 0u; t.wt[i] = 0; }
    t.cx = t.cy = 0;
    t.interior = false;
    if (!(fabsf(mx) < 0x1p26f && fabsf(my) < 0x1p26f)) return t;
    const long long qx = llrint((double)mx * 32.0), qy = llrint((double)my * 32.0);
    const long long cx = qx >> 5, cy = qy >> 5;
    const int fx = (int)(qx & 31), fy = (int)(qy & 31);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const long long xx = cx + dx, yy = cy + dy;
            if (xx >= 0 && xx < wc && yy >= 0 && yy < hc) {
                t.off[2 * dy + dx] = (uint32_t)(yy * wc + xx);
                t.wt[2 * dy + dx] = (dy ? fy : 32 - fy) * (dx ? fx : 32 - fx);
            }
        }
    if (cx >= 0 && cx + 1 < wc && cy >= 0 && cy + 1 < hc) {
        t.cx = (int)cx; t.cy = (int)cy;
        t.interior = true;
    }
    return t;
}

// Sum of the valid flags of a workgroup's pixels (thread: `mine` of its four) -> every thread gets the workgroup's total and
// `before`, the number of valid pixels of the threads before it.  Four 64-bit ballots per wave (one per pixel slot), popcounts
// below the lane, the waves' totals through LDS.
__device__ __forceinline__ int graycode_block_rank(const bool (&valid)[GRAYCODE_PER_THREAD], int *wave_total, int &before)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    int in_wave = 0, lanes_before = 0;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        const u64 m = __ballot(valid[j]);
        in_wave += __popcll(m);
        lanes_before += __popcll(m & below);
    }
    if (lane == 0) wave_total[wave] = in_wave;
    __syncthreads();
    int total = 0;
    before = lanes_before;
#pragma unroll
    for (int k = 0; k < GRAYCODE_WAVES; ++k) {
        const int t = wave_total[k];
        if (k < wave) before += t;
        total += t;
    }
    return total;
}

// The two codes of a thread's four pixels: the bit loop of getProjPixel over the n planes.  How a plane is read is the mode, fixed
// outside the loop: GRAY_ROW4 one (unaligned) 4-byte load, the four pixels being consecutive bytes; GRAY_BYTES a byte per living
// pixel; GRAY_TAPS four byte gathers per pixel, (S + 512) >> 10; GRAY_WINDOW the same sums with the sixteen taps of the thread's
// four pixels cut out of three (unaligned) 8-byte loads, the rows win.y0 .. + 2 from column win.x0 on (GrayWindow).
enum { GRAY_ROW4 = 0, GRAY_BYTES = 1, GRAY_TAPS = 2, GRAY_WINDOW = 3 };

// Undistortion maps are smooth and close to the identity: the taps of four consecutive pixels then lie within 8 columns and 3
// rows of the source, and 3 loads per plane do the work of 16 byte gathers.  `ok` if they do, for four living pixels with all
// taps inside the image, and the third row's 8 bytes end inside the plane; shift[j] = 8 (cx_j - x0), lower[j] = cy_j - y0.
struct GrayWindow {
    uint32_t off;
    int shift[GRAYCODE_PER_THREAD];
    bool lower[GRAYCODE_PER_THREAD];
    bool ok;
};

__device__ __forceinline__ GrayWindow graycode_window(const GrayTaps (&taps)[GRAYCODE_PER_THREAD], const bool (&live)[GRAYCODE_PER_THREAD],
                                                      int wc, long long plane_stride)
{
    GrayWindow win;
    int x0 = taps[0].cx, x1 = x0, y0 = taps[0].cy, y1 = y0;
    win.ok = true;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        win.ok = win.ok && live[j] && taps[j].interior;
        x0 = min(x0, taps[j].cx); x1 = max(x1, taps[j].cx);
        y0 = min(y0, taps[j].cy); y1 = max(y1, taps[j].cy);
    }
    win.ok = win.ok && x1 - x0 <= 6 && y1 - y0 <= 1 && (long long)(y0 + 2) * wc + x0 + 8 <= plane_stride;
    win.off = (uint32_t)y0 * (uint32_t)wc + (uint32_t)x0;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        win.shift[j] = 8 * (taps[j].cx - x0);
        win.lower[j] = taps[j].cy != y0;
    }
    return win;
}

// One plane's values at a thread's four pixels, read in the mode fixed outside the plane loop (graycode_codes, and
// phaseshift_coords of phaseshift_kernels.hip.h).
template <int MODE>
__device__ __forceinline__ void graycode_fetch(const uint8_t *__restrict__ pl, int wc, const bool (&live)[GRAYCODE_PER_THREAD],
                                               const uint32_t (&at)[GRAYCODE_PER_THREAD], const GrayTaps *taps, const GrayWindow *win,
                                               int (&v)[GRAYCODE_PER_THREAD])
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
    if (MODE == GRAY_WINDOW) {
        const uint64_t r0 = *reinterpret_cast<const u64_unaligned *>(pl + win->off);
        const uint64_t r1 = *reinterpret_cast<const u64_unaligned *>(pl + win->off + wc);
        const uint64_t r2 = *reinterpret_cast<const u64_unaligned *>(pl + win->off + 2 * wc);
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
            const GrayTaps &t = taps[j];
            const uint32_t top = (uint32_t)((win->lower[j] ? r1 : r0) >> win->shift[j]), bot = (uint32_t)((win->lower[j] ? r2 : r1) >> win->shift[j]);
            v[j] = (t.wt[0] * (int)(top & 0xffu) + t.wt[1] * (int)((top >> 8) & 0xffu) + t.wt[2] * (int)(bot & 0xffu) +
                    t.wt[3] * (int)((bot >> 8) & 0xffu) + 512) >> 10;
        }
    } else if (MODE == GRAY_TAPS) {
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
            const GrayTaps &t = taps[j];
            v[j] = (t.wt[0] * (int)pl[t.off[0]] + t.wt[1] * (int)pl[t.off[1]] + t.wt[2] * (int)pl[t.off[2]] + t.wt[3] * (int)pl[t.off[3]] + 512) >> 10;
        }
    } else if (MODE == GRAY_ROW4) {
        const uint32_t q = *reinterpret_cast<const u32_unaligned *>(pl + at[0]);
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) v[j] = (int)((q >> (8 * j)) & 0xffu);
    } else {
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) v[j] = live[j] ? (int)pl[at[j]] : 0;
    }
}

// The front of a decoder: a thread's four pixels from p0 on -- live[j] if pixel p0 + j is inside the region, at[j] its offset inside
// a plane (and inside the maps) --, with MAPS their taps and window, and the mode all planes are read in.  body(mode, at, taps, win)
// runs once, with the mode as a compile-time constant (std::integral_constant): the plane loop of graycode_codes or
// phaseshift_coords.  Without maps a thread whose four pixels are alive and consecutive bytes of a plane reads them with one load.
template <bool MAPS, class Body>
__device__ __forceinline__ void plane_stack_frame(const PlaneStack &S, long long p0, bool (&live)[GRAYCODE_PER_THREAD], Body body)
{
    uint32_t at[GRAYCODE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        live[j] = p0 + j < S.npix;
        const uint32_t p = live[j] ? (uint32_t)(p0 + j) : 0u;
        const uint32_t ry = p / (uint32_t)S.w, rx = p - ry * (uint32_t)S.w;
        at[j] = (uint32_t)(S.y0 + (int)ry) * (uint32_t)S.wc + (uint32_t)(S.x0 + (int)rx);
    }
    if (MAPS) {
        GrayTaps taps[GRAYCODE_PER_THREAD];
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j)      // (a pixel past the end: no taps)
            taps[j] = graycode_taps(live[j] ? S.mapx[at[j]] : __builtin_nanf(""), live[j] ? S.mapy[at[j]] : 0.f, S.hc, S.wc);
        const GrayWindow win = graycode_window(taps, live, S.wc, S.plane_stride);
        if (win.ok) body(std::integral_constant<int, GRAY_WINDOW>(), at, taps, &win);
        else body(std::integral_constant<int, GRAY_TAPS>(), at, taps, nullptr);
    } else if (live[GRAYCODE_PER_THREAD - 1] && at[GRAYCODE_PER_THREAD - 1] == at[0] + (GRAYCODE_PER_THREAD - 1)) {
        body(std::integral_constant<int, GRAY_ROW4>(), at, nullptr, nullptr);
    } else {
        body(std::integral_constant<int, GRAY_BYTES>(), at, nullptr, nullptr);
    }
}

template <int MODE>
__device__ __forceinline__ void graycode_codes(const GrayDecodeArgs &A, const bool (&live)[GRAYCODE_PER_THREAD], const uint32_t (&at)[GRAYCODE_PER_THREAD],
                                               const GrayTaps *taps, const GrayWindow *win, int (&code)[2][GRAYCODE_PER_THREAD],
                                               bool (&err)[GRAYCODE_PER_THREAD])
{
    const PlaneStack &S = A.stack;
    const uint8_t *pl = S.planes;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) err[j] = false;
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        int bin[GRAYCODE_PER_THREAD], dec[GRAYCODE_PER_THREAD];
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) { bin[j] = 0; dec[j] = 0; }
        const int nbits = axis ? A.nrow : A.ncol;
#pragma unroll(MODE == GRAY_ROW4 ? 4 : MODE == GRAY_WINDOW ? 2 : 1)
        for (int k = 0; k < nbits; ++k) {
            int v1[GRAYCODE_PER_THREAD], v2[GRAYCODE_PER_THREAD];
            graycode_fetch<MODE>(pl, S.wc, live, at, taps, win, v1);
            graycode_fetch<MODE>(pl + S.plane_stride, S.wc, live, at, taps, win, v2);
            pl += 2 * S.plane_stride;
#pragma unroll
            for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
                const int d = v1[j] - v2[j];
                err[j] = err[j] || (d < 0 ? -d : d) < A.thr;
                bin[j] ^= (int)(d > 0);
                dec[j] = (dec[j] << 1) | bin[j];
            }
        }
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) code[axis][j] = dec[j];
    }
}

// getProjPixel (OpenCV structured_light/src/graycodepattern.cpp) for every pixel of the region.  Per bit, v1 the pattern plane
// and v2 its inverse: error if |v1 - v2| < thr; the Gray bit is v1 > v2; Gray -> binary is the MSB-first prefix XOR; after both
// codes, error if xDec >= pw or yDec >= ph.  Without maps a thread whose four pixels lie in one region row reads each plane
// with one (unaligned) 4-byte load; with maps every plane is sampled through the pixel's four taps, which are computed once, and
// a thread whose sixteen taps lie close together cuts them out of three 8-byte loads per plane.
// HBM floor per pixel: n plane bytes (+ 8 map bytes) in, 8 out.  out must be 16-byte aligned.
template <bool MAPS>
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_decode_kernel(const GrayDecodeArgs A)
{
    __shared__ int wave_total[GRAYCODE_WAVES];
    const long long p0 = (long long)blockIdx.x * GRAYCODE_BLOCK + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    bool live[GRAYCODE_PER_THREAD], err[GRAYCODE_PER_THREAD];
    int code[2][GRAYCODE_PER_THREAD];
    plane_stack_frame<MAPS>(A.stack, p0, live, [&](auto mode, const uint32_t (&at)[GRAYCODE_PER_THREAD], const GrayTaps *taps, const GrayWindow *win) {
        graycode_codes<decltype(mode)::value>(A, live, at, taps, win, code, err);
    });
    bool valid[GRAYCODE_PER_THREAD];
    int2 px[GRAYCODE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        valid[j] = live[j] && !err[j] && code[0][j] < A.pw && code[1][j] < A.ph;
        px[j] = valid[j] ? make_int2(code[0][j], code[1][j]) : make_int2(-1, -1);
    }
    if (live[GRAYCODE_PER_THREAD - 1]) {
        int4 *const o = reinterpret_cast<int4 *>(A.out + 2 * p0);
        o[0] = make_int4(px[0].x, px[0].y, px[1].x, px[1].y);
        o[1] = make_int4(px[2].x, px[2].y, px[3].x, px[3].y);
    } else {
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j)
            if (live[j]) reinterpret_cast<int2 *>(A.out)[p0 + j] = px[j];
    }
    if (A.counts) {                                           // (uniform: a kernel argument)
        int before;
        const int total = graycode_block_rank(valid, wave_total, before);
        if (threadIdx.x == 0) A.counts[blockIdx.x] = total;
    }
}

// counts [n] -> offsets [n + 1]: offsets[i] = counts[0] + .. + counts[i - 1], offsets[n] = the total (< 2^31: there are fewer
// pixels).  ONE workgroup walks the array GRAYCODE_BLOCK entries at a time (a 1080p frame has about 2000): a thread sums its
// four entries, a wave scans its 64 sums with shuffles, the four wave sums and the running carry go through LDS.
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_scan_kernel(const int32_t *__restrict__ counts, int32_t *__restrict__ offsets, int n)
{
    __shared__ int wave_sum[GRAYCODE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += GRAYCODE_BLOCK) {
        const int i0 = base + GRAYCODE_PER_THREAD * (int)threadIdx.x;
        int c[GRAYCODE_PER_THREAD], mine = 0;
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
            c[j] = i0 + j < n ? counts[i0 + j] : 0;
            mine += c[j];
        }
        int incl = mine;                                      // inclusive scan over the wave's lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int run = carry + incl - mine, chunk = 0;
#pragma unroll
        for (int k = 0; k < GRAYCODE_WAVES; ++k) {
            const int t = wave_sum[k];
            if (k < wave) run += t;
            chunk += t;
        }
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
            if (i0 + j < n) offsets[i0 + j] = run;
            run += c[j];
        }
        carry += chunk;
        __syncthreads();                                      // wave_sum is rewritten by the next round
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

// decoded [h][w][2] -> points.  Every valid pixel (xDec >= 0) is triangulated from its centre (x + 0.5, y + 0.5) and the
// projector pixel's centre (xDec + 0.5, yDec + 0.5) by ftp_triangulate.  With `offsets` the block's points go to
// out + 3 (offsets[block] + rank): the (n, 1, 3) array of the reference, in raster order.  With offsets == NULL the output is
// dense, [h][w][3], NaN at the invalid pixels.  Either way the block's points are gathered in LDS (24 KiB) and leave as
// contiguous 8-byte stores.  decoded must be 16-byte aligned.
template <int MODEL>
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_cloud_kernel(const int32_t *__restrict__ decoded, const int32_t *__restrict__ offsets,
                                                                          double *__restrict__ out, long long npix, int w, int x0, int y0,
                                                                          const FtpCloudGeom G)
{
#pragma clang fp contract(off)
    __shared__ double stage[GRAYCODE_BLOCK * 3];
    __shared__ int wave_total[GRAYCODE_WAVES];
    const long long block0 = (long long)blockIdx.x * GRAYCODE_BLOCK;
    const long long p0 = block0 + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    int2 px[GRAYCODE_PER_THREAD];
    bool live[GRAYCODE_PER_THREAD], valid[GRAYCODE_PER_THREAD];
    if (p0 + GRAYCODE_PER_THREAD <= npix) {
        const int4 a = reinterpret_cast<const int4 *>(decoded + 2 * p0)[0], b = reinterpret_cast<const int4 *>(decoded + 2 * p0)[1];
        px[0] = make_int2(a.x, a.y); px[1] = make_int2(a.z, a.w); px[2] = make_int2(b.x, b.y); px[3] = make_int2(b.z, b.w);
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) live[j] = true;
    } else {
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
            live[j] = p0 + j < npix;
            px[j] = live[j] ? reinterpret_cast<const int2 *>(decoded)[p0 + j] : make_int2(-1, -1);
        }
    }
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) valid[j] = live[j] && px[j].x >= 0;
    const bool dense = offsets == nullptr;
    int rank, total;
    if (dense) {                                              // (uniform: a kernel argument)
        rank = GRAYCODE_PER_THREAD * (int)threadIdx.x;
        const long long left = npix - block0;
        total = (int)(left < GRAYCODE_BLOCK ? left : GRAYCODE_BLOCK);
    } else {
        total = graycode_block_rank(valid, wave_total, rank);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        if (valid[j]) {
            const uint32_t p = (uint32_t)(p0 + j);
            const uint32_t ry = p / (uint32_t)w, rx = p - ry * (uint32_t)w;
            double o[3];
            ftp_triangulate<MODEL>(G, ((double)rx + (double)x0) + 0.5, ((double)ry + (double)y0) + 0.5, (double)px[j].x + 0.5,
                                   (double)px[j].y + 0.5, o);
            stage[3 * rank] = o[0]; stage[3 * rank + 1] = o[1]; stage[3 * rank + 2] = o[2];
            ++rank;
        } else if (dense && live[j]) {
            stage[3 * rank] = nan; stage[3 * rank + 1] = nan; stage[3 * rank + 2] = nan;
            ++rank;
        }
    }
    __syncthreads();
    double *const dst = out + 3 * (dense ? block0 : (long long)offsets[blockIdx.x]);
    for (int i = threadIdx.x; i < 3 * total; i += GRAYCODE_THREADS) dst[i] = stage[i];
}

}  // namespace ssamd
