// K11: numpy's phase unwrap (np.unwrap, float path; numpy/lib/_function_base_impl.py) -- what the reference's getCloud runs by
// default (simplestereo/active.py:739-745: np.unwrap along axis 1, then along axis 0), fp64 and bit-identical to numpy.
//
// Along one line p[0 .. len-1], with hi = period / 2, lo = -hi:
//     dd    = p[i] - p[i-1]
//     m     = fmod(dd - lo, period);  if (m != 0) { if (m < 0) m += period; } else m = +0.0         (np.mod)
//     ddmod = m + lo;                 if (ddmod == lo && dd > 0) ddmod = hi
//     c[i]  = ddmod - dd;             if (|dd| < discont) c[i] = 0.0
//     s[i]  = s[i-1] + c[i]           (np.cumsum: strictly left to right)
//     out[0] = p[0];  out[i] = p[i] + s[i]
// Every operation is fp64 and rounded once.  The corrections are not exact multiples of the period, so the running sum rounds
// and its ORDER is observable: a blocked or tree scan gives other bits.  Only that one add per sample is serial; dd, c and
// p + s are pointwise.  Both kernels separate the two: all lanes compute c into LDS from coalesced loads, one lane per line adds
// them up in order (its LDS reads do not depend on the chain and are issued a batch ahead of it), all lanes write p + s.
// c is never -0.0 (x - x = +0.0), so a line's sum may start from +0.0 and padding corrections of +0.0 change nothing.
//
// In place (out == p) is allowed: a chunk or tile is loaded completely before any of it is stored, and the sample before it
// comes from the carried state, not from memory.
#pragma once
#include "common.hip.h"
#include "np_unwrap_plan.h"

namespace ssamd {

// the correction of one sample; |dd| < discont is tested first (a NaN dd or discont fails it and takes the full path, as in numpy,
// where the zeroing is the last step and never applies to them)
__device__ __forceinline__ double npu_correction(double cur, double prev, double discont, double period, double hi, double lo)
{
#pragma clang fp contract(off)
    const double dd = cur - prev;
    if (fabs(dd) < discont) return 0.0;
    double m = fmod(dd - lo, period);                    // exact remainder (device library)
    if (m != 0) {
        if (m < 0) m += period;
    } else {
        m = 0.0;
    }
    double ddmod = m + lo;
    if (ddmod == lo && dd > 0) ddmod = hi;
    return ddmod - dd;
}

// s[k] = s[k-1] + c[k] over the first n (a multiple of NPU_WALK) corrections of an LDS array, in place, by the calling lane; the
// next batch is read before the chain of the current one, so the array extends NPU_WALK entries past n (read, never used).
// npu_walk_line: a line of consecutive doubles, read and written as double2.  npu_walk_column: one column of a tile, `stride`
// doubles from row to row.
__device__ __forceinline__ double npu_walk_line(double2 *cs, int n, double s)
{
#pragma clang fp contract(off)
    double2 nx[NPU_WALK / 2];
#pragma unroll
    for (int j = 0; j < NPU_WALK / 2; ++j) nx[j] = cs[j];
    for (int k0 = 0; k0 < n; k0 += NPU_WALK) {
        double2 a[NPU_WALK / 2];
#pragma unroll
        for (int j = 0; j < NPU_WALK / 2; ++j) a[j] = nx[j];
#pragma unroll
        for (int j = 0; j < NPU_WALK / 2; ++j) nx[j] = cs[(k0 + NPU_WALK) / 2 + j];
#pragma unroll
        for (int j = 0; j < NPU_WALK / 2; ++j) {
            s += a[j].x; a[j].x = s;
            s += a[j].y; a[j].y = s;
        }
#pragma unroll
        for (int j = 0; j < NPU_WALK / 2; ++j) cs[k0 / 2 + j] = a[j];
    }
    return s;
}

__device__ __forceinline__ double npu_walk_column(double *cs, int stride, int n, double s)
{
#pragma clang fp contract(off)
    double nx[NPU_WALK];
#pragma unroll
    for (int j = 0; j < NPU_WALK; ++j) nx[j] = cs[j * stride];
    for (int k0 = 0; k0 < n; k0 += NPU_WALK) {
        double a[NPU_WALK];
#pragma unroll
        for (int j = 0; j < NPU_WALK; ++j) a[j] = nx[j];
#pragma unroll
        for (int j = 0; j < NPU_WALK; ++j) nx[j] = cs[(k0 + NPU_WALK + j) * stride];
#pragma unroll
        for (int j = 0; j < NPU_WALK; ++j) { s += a[j]; a[j] = s; }
#pragma unroll
        for (int j = 0; j < NPU_WALK; ++j) cs[(k0 + j) * stride] = a[j];
    }
    return s;
}

// Row form: one wave per line (blockIdx.x), the line at p + blockIdx.x * len, contiguous.  Lane l holds the samples
// base + 64 j + l of a chunk, so every load and store of the wave is one contiguous 512 bytes; the sample before it comes from
// the lane below (from lane 63 of the previous j, from the carried sample for the first of the chunk).
__global__ __launch_bounds__(NPU_ROW_THREADS) void np_unwrap_row_kernel(const double *p, double *out, long long len, double discont,
                                                                        double period, double hi, double lo)
{
#pragma clang fp contract(off)
    __shared__ double2 cs2[(NPU_ROW_CHUNK + NPU_WALK) / 2];      // the last NPU_WALK doubles are never written: the walk's read-ahead
                                                                 // lands there after the last batch and its values are dropped
    double *cs = reinterpret_cast<double *>(cs2);
    const int lane = threadIdx.x;
    const double *P = p + (size_t)blockIdx.x * (size_t)len;
    double *O = out + (size_t)blockIdx.x * (size_t)len;
    double s = 0.0;                                      // the running sum (lane 0)
    double carry = 0.0;                                  // the sample before the chunk
    for (long long base = 0; base < len; base += NPU_ROW_CHUNK) {
        double v[NPU_ROW_PER];
#pragma unroll
        for (int j = 0; j < NPU_ROW_PER; ++j) {
            const long long x = base + j * 64 + lane;
            v[j] = x < len ? P[x] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < NPU_ROW_PER; ++j) {
            const long long x = base + j * 64 + lane;
            double prev = __shfl_up(v[j], 1);
            const double wrapped = j == 0 ? carry : __shfl(v[j > 0 ? j - 1 : 0], 63);
            if (lane == 0) prev = wrapped;
            cs[j * 64 + lane] = (x == 0 || x >= len) ? 0.0 : npu_correction(v[j], prev, discont, period, hi, lo);
        }
        carry = __shfl(v[NPU_ROW_PER - 1], 63);
        __syncthreads();
        if (lane == 0) {
            const long long left = len - base;
            const int n = left < NPU_ROW_CHUNK ? (int)((left + NPU_WALK - 1) / NPU_WALK * NPU_WALK) : NPU_ROW_CHUNK;
            s = npu_walk_line(cs2, n, s);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NPU_ROW_PER; ++j) {
            const long long x = base + j * 64 + lane;
            if (x < len) O[x] = x == 0 ? v[j] : v[j] + cs[j * 64 + lane];      // out[0] is p[0] itself (-0.0 stays -0.0)
        }
    }
}

// Column form: workgroup blockIdx.x = (outer index o, lane group g); thread (lx, ry) = (tid % 16, tid / 16) owns column
// 16 g + lx and, of every tile of 128 rows, the 8 consecutive rows t0 + 8 ry ...: nine independent loads (its rows and the one
// above), seven of the eight differences from its own registers.  The row above a tile is its column's carried sample (LDS, written
// by the thread that held it); lane lx of the first wave adds the tile's corrections of column lx in order.
__global__ __launch_bounds__(NPU_COL_THREADS) void np_unwrap_col_kernel(const double *p, double *out, long long len, long long inner,
                                                                        long long groups, double discont, double period, double hi,
                                                                        double lo)
{
#pragma clang fp contract(off)
    __shared__ double cs[(NPU_COL_ROWS + NPU_WALK) * NPU_COL_LANES];      // the last NPU_WALK rows: read-ahead only, never written or used
    __shared__ double last[NPU_COL_LANES];
    constexpr int L = NPU_COL_LANES, PER = NPU_COL_PER, RW = NPU_COL_THREADS / NPU_COL_LANES;
    const int tid = threadIdx.x, lx = tid % L, ry = tid / L;
    const long long o = blockIdx.x / groups, g = blockIdx.x % groups;
    const long long col = g * L + lx;
    const bool live = col < inner;
    const size_t off = (size_t)o * (size_t)len * (size_t)inner + (size_t)(live ? col : 0);
    const double *P = p + off;
    double *O = out + off;
    double s = 0.0;                                      // the running sum of column lx (threads 0 .. 15)
    for (long long t0 = 0; t0 < len; t0 += NPU_COL_ROWS) {
        const long long r0 = t0 + ry * PER;
        double v[PER], above = 0.0;
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = (live && r0 + j < len) ? P[(size_t)(r0 + j) * (size_t)inner] : 0.0;
        if (ry == 0) { if (t0 > 0) above = last[lx]; }
        else if (live && r0 - 1 < len) above = P[(size_t)(r0 - 1) * (size_t)inner];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long long r = r0 + j;
            const double prev = j == 0 ? above : v[j > 0 ? j - 1 : 0];
            cs[(ry * PER + j) * L + lx] = (!live || r == 0 || r >= len) ? 0.0 : npu_correction(v[j], prev, discont, period, hi, lo);
        }
        __syncthreads();
        if (tid < L) {
            const long long left = len - t0;
            const int n = left < NPU_COL_ROWS ? (int)((left + NPU_WALK - 1) / NPU_WALK * NPU_WALK) : NPU_COL_ROWS;
            s = npu_walk_column(cs + lx, L, n, s);
        }
        if (ry == RW - 1) last[lx] = v[PER - 1];         // read by the threads of ry == 0 before the barrier above, next after the one below
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long long r = r0 + j;
            if (live && r < len) O[(size_t)r * (size_t)inner] = r == 0 ? v[j] : v[j] + cs[(ry * PER + j) * L + lx];
        }
    }
}

}  // namespace ssamd
