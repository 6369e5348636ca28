// Gray-code active stereo with two calibrated cameras and one uncalibrated projector: what the reference's GrayCodeDouble.getCloud
// (active.py:1508-1608) sets out to do.  Each camera's decoded map (graycode_decode_kernel) says which projector pixel a camera
// pixel sees; a projector pixel seen by both cameras is a camera-camera correspondence.  Three kernels:
//   graycode_scatter_kernel       decoded [h][w][2] of ONE camera -> that camera's projector-shaped table (the inversion)
//   graycode_match_kernel         both tables -> matches [Hp][Wp][4] = (x1, y1, x2, y2) pixel centres or NaN, matched cells per block
//   graycode_stereo_cloud_kernel  matches (+ block offsets), or point pairs of the caller's -> points, by rectified_triangulate
// All three use the partition of graycode_kernels.hip.h: one flattened index, GRAYCODE_BLOCK consecutive elements per workgroup,
// thread t owns the elements 4 t .. 4 t + 3 of its block; graycode_scan_kernel turns the match counts into offsets.
//
// Two reductions of the camera pixels that decode to one projector pixel (cell c = yDec * pw + xDec):
//   STEREO_LAST  the reference's loop, where a later pixel overwrites an earlier one: the pixel with the largest key
//                y * stride + x (absolute image coordinates, stride > every x) wins.  int32 table cleared to -1, integer atomic max.
//   STEREO_MEAN  the centroid of those pixels: u64 sum of x, u64 sum of y, u32 count per cell, cleared to 0, integer atomic adds.
// Integer max and integer sums do not depend on the order of arrival: the tables, and with them every output, are the same bytes
// on every run.  No float atomics.  The atomics are relaxed, agent scope and their results unused (no-return instructions);
// the table is cleared by a memset and read by the match kernel on the same stream, and kernel boundaries order the three.
#pragma once
#include "common.hip.h"
#include "ftp_cloud_kernels.hip.h"
#include "graycode_kernels.hip.h"

namespace ssamd {

enum { STEREO_LAST = 0, STEREO_MEAN = 1 };

// One camera's table, `cells` = ph * pw < 2^31 entries each.  STEREO_LAST reads `key` alone, STEREO_MEAN the other three.
struct StereoTable {
    int32_t *key;                   // [cells] the winning pixel's y * stride + x, or -1
    unsigned long long *sx, *sy;    // [cells] sums of the absolute x and y
    uint32_t *cnt;                  // [cells] pixels summed
    int stride;                     // of the key: x0 + w of the camera's region, (y0 + h) * stride < 2^31
};

// bytes of one camera's table, a multiple of 8 (SSAMD_GRAYCODE_STEREO_SCRATCH of include/ssamd_graycode_stereo.h is twice this)
__host__ __device__ inline size_t stereo_table_bytes(long long cells, int mode)
{
    return (size_t)((mode == STEREO_MEAN ? 20 * cells : 4 * cells) + 7) & ~(size_t)7;
}

// decoded [h][w][2] of one camera (region origin x0, y0 in its image) -> its table.  A thread first merges runs of its four
// consecutive pixels that decode to the same cell -- neighbours usually do when the camera out-resolves the projector -- into one
// update: the last pixel of the run (LAST: keys rise with the pixel index) or the run's sums (MEAN).  A pixel whose code lies
// outside the pw x ph table (only a caller's own map can hold one) is skipped like an invalid one: no store out of bounds.
// decoded must be 16-byte aligned.
template <int MODE>
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_scatter_kernel(const int32_t *__restrict__ decoded, long long npix, int w, int x0, int y0,
                                                                            int pw, int ph, const StereoTable T)
{
    const long long p0 = (long long)blockIdx.x * GRAYCODE_BLOCK + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    if (p0 >= npix) return;
    int2 px[GRAYCODE_PER_THREAD];
    if (p0 + GRAYCODE_PER_THREAD <= npix) {
        const int4 a = reinterpret_cast<const int4 *>(decoded + 2 * p0)[0], b = reinterpret_cast<const int4 *>(decoded + 2 * p0)[1];
        px[0] = make_int2(a.x, a.y); px[1] = make_int2(a.z, a.w); px[2] = make_int2(b.x, b.y); px[3] = make_int2(b.z, b.w);
    } else {
#pragma unroll
        for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) px[j] = p0 + j < npix ? reinterpret_cast<const int2 *>(decoded)[p0 + j] : make_int2(-1, -1);
    }
    int cell[GRAYCODE_PER_THREAD + 1];
    uint32_t ax[GRAYCODE_PER_THREAD], ay[GRAYCODE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        const bool ok = px[j].x >= 0 && px[j].x < pw && px[j].y >= 0 && px[j].y < ph;
        cell[j] = ok ? px[j].y * pw + px[j].x : -1;               // < 2^31: a cell of the table
        const uint32_t p = (uint32_t)(p0 + j);                    // (past the end: cell -1, the coordinates are not used)
        const uint32_t ry = p / (uint32_t)w, rx = p - ry * (uint32_t)w;
        ax[j] = (uint32_t)x0 + rx; ay[j] = (uint32_t)y0 + ry;
    }
    cell[GRAYCODE_PER_THREAD] = -2;                               // ends the last run
    unsigned long long sx = 0, sy = 0;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        if (cell[j] < 0) continue;
        if (MODE == STEREO_MEAN) { sx += ax[j]; sy += ay[j]; ++n; }
        if (cell[j] == cell[j + 1]) continue;                     // the run goes on
        if (MODE == STEREO_LAST) {
            (void)__hip_atomic_fetch_max(T.key + cell[j], (int)(ay[j] * (uint32_t)T.stride + ax[j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            (void)__hip_atomic_fetch_add(T.sx + cell[j], sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(T.sy + cell[j], sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(T.cnt + cell[j], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sx = 0; sy = 0; n = 0;
        }
    }
}

// The pixel a table holds for cell c -> (x, y) as doubles, false if no pixel decoded to it.  MEAN: (double) sum / (double) count,
// one IEEE division each (the conversions are exact below 2^53).
template <int MODE>
__device__ __forceinline__ bool stereo_cell(const StereoTable &T, long long c, double &x, double &y)
{
    if (MODE == STEREO_LAST) {
        const int k = T.key[c];
        if (k < 0) return false;
        const int yy = k / T.stride;
        x = (double)(k - yy * T.stride); y = (double)yy;
        return true;
    }
    const uint32_t n = T.cnt[c];
    if (n == 0) return false;
    x = (double)T.sx[c] / (double)n; y = (double)T.sy[c] / (double)n;
    return true;
}

// Both tables -> matches [cells][4]: (x1 + 0.5, y1 + 0.5, x2 + 0.5, y2 + 0.5), the pixel centres the reference's `corresp += 0.5`
// intends, for a projector pixel both cameras see, four NaN for any other; counts[block] = the matched cells of the block (or
// counts == NULL).  A thread's four cells are 128 contiguous bytes.  matches must be 16-byte aligned.
template <int MODE>
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_match_kernel(const StereoTable T1, const StereoTable T2, long long cells,
                                                                          double *__restrict__ matches, int32_t *__restrict__ counts)
{
    __shared__ int wave_total[GRAYCODE_WAVES];
    const long long c0 = (long long)blockIdx.x * GRAYCODE_BLOCK + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    bool valid[GRAYCODE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        valid[j] = false;
        if (c0 + j >= cells) continue;
        double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        const bool one = stereo_cell<MODE>(T1, c0 + j, x1, y1), two = stereo_cell<MODE>(T2, c0 + j, x2, y2);
        valid[j] = one && two;
        double2 *const o = reinterpret_cast<double2 *>(matches + 4 * (c0 + j));
        o[0] = valid[j] ? make_double2(x1 + 0.5, y1 + 0.5) : make_double2(nan, nan);
        o[1] = valid[j] ? make_double2(x2 + 0.5, y2 + 0.5) : make_double2(nan, nan);
    }
    if (counts) {                                             // (uniform: a kernel argument)
        int before;
        const int total = graycode_block_rank(valid, wave_total, before);
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
    }
}

// Point pairs -> points, by rectified_triangulate and nothing else (both images were undistorted: no undistortPoints).
//   PAIRS false: a = matches [n][4] of graycode_match_kernel (16-byte aligned), b unused.  With `offsets` the block's points go
//                to out + 3 (offsets[block] + rank), (total, 3) in projector raster order; with offsets == NULL out is [n][3].
//   PAIRS true : a = points of image 1 [n][2], b = points of image 2 [n][2], a caller's own; out is [n][3] (offsets NULL).
// A pair that holds a NaN gives three NaN (dense) or is left out (compacted: the match kernel counted it so).  The block's points
// are gathered in LDS (24 KiB) and leave as contiguous 8-byte stores, as graycode_cloud_kernel's do.
template <bool PAIRS>
__global__ __launch_bounds__(GRAYCODE_THREADS) void graycode_stereo_cloud_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                                                 const int32_t *__restrict__ offsets, double *__restrict__ out,
                                                                                 long long n, const FtpCloudGeom G)
{
#pragma clang fp contract(off)
    __shared__ double stage[GRAYCODE_BLOCK * 3];
    __shared__ int wave_total[GRAYCODE_WAVES];
    const long long block0 = (long long)blockIdx.x * GRAYCODE_BLOCK;
    const long long p0 = block0 + GRAYCODE_PER_THREAD * (int)threadIdx.x;
    double m[GRAYCODE_PER_THREAD][4];
    bool live[GRAYCODE_PER_THREAD], valid[GRAYCODE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        live[j] = p0 + j < n;
        valid[j] = false;
        if (!live[j]) continue;
        if (PAIRS) {
            m[j][0] = a[2 * (p0 + j)]; m[j][1] = a[2 * (p0 + j) + 1]; m[j][2] = b[2 * (p0 + j)]; m[j][3] = b[2 * (p0 + j) + 1];
        } else {
            const double2 lo = reinterpret_cast<const double2 *>(a + 4 * (p0 + j))[0], hi = reinterpret_cast<const double2 *>(a + 4 * (p0 + j))[1];
            m[j][0] = lo.x; m[j][1] = lo.y; m[j][2] = hi.x; m[j][3] = hi.y;
        }
        valid[j] = m[j][0] == m[j][0] && m[j][1] == m[j][1] && m[j][2] == m[j][2] && m[j][3] == m[j][3];
    }
    const bool dense = offsets == nullptr;
    int rank, total;
    if (dense) {                                              // (uniform: a kernel argument)
        rank = GRAYCODE_PER_THREAD * (int)threadIdx.x;
        const long long left = n - block0;
        total = (int)(left < GRAYCODE_BLOCK ? left : GRAYCODE_BLOCK);
    } else {
        total = graycode_block_rank(valid, wave_total, rank);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int j = 0; j < GRAYCODE_PER_THREAD; ++j) {
        if (valid[j]) {
            double o[3];
            rectified_triangulate(G, m[j][0], m[j][1], m[j][2], m[j][3], o);
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
