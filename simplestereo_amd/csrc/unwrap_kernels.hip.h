// K9: infinite-impulse-response phase unwrapping (Estrada et al. 2011), the reference's second native extension
// _unwrapping.infiniteImpulseResponse (simplestereo/_unwrapping.cpp:50-156, wrapper unwrapping.py:10-41), fp64 and bit-identical.
//
// The reference visits the pixels in a fixed order and sets a "visited" flag after each step; a step averages, over the
// flagged pixels c of the clipped 3x3 window in row-major order, u_c + tau * W(cur - u_c) (W wraps into [-pi, pi)), and divides
// by their count.  Passes: row 0 forward (x = 0..w-1), row 0 backward (x = w-1..1), then every row forward.  In the main pass,
// pixel (y, x) of a row y >= 1 reads exactly (y-1, x-1), (y-1, x), (y-1, x+1) and (y, x-1): the row above up to column x + 1
// and its own left neighbour.  So with a skew t = x + 2y, all pixels of one step t are independent and each sees the same
// operands in the same order as in the serial loop -- a wavefront, not a change of arithmetic.
//
// One workgroup per map (a batch of n maps is a grid of n workgroups; nothing crosses workgroups).  Thread r of the workgroup
// owns row y0 + r of a band of R rows and computes column t - 2r at step t.  The value it needs from the row above at step t,
// (y-1, x+1), is what thread r-1 produced at step t-1: it goes through a double-buffered LDS slot, one barrier per step,
// and the thread keeps the two previous ones (y-1, x), (y-1, x-1) in registers.  The last row of a band is kept in an LDS line
// of w doubles, which the first thread of the next band reads as its row above; before the first band, thread 0 runs the two
// serial row-0 passes in that same line (so at most 16384 columns: 128 KiB of LDS).  Each thread loads its row's phase
// eight columns ahead.  Steps per band: w + 2 (rows - 1).
#pragma once
#include "common.hip.h"

namespace ssamd {

static constexpr int UNWRAP_MAX_W = 16384;        // LDS line of w doubles (+ 2 x rows doubles of exchange slots) per workgroup
static constexpr int UNWRAP_MAX_ROWS = 1024;      // rows per band = threads per workgroup

// fmod(x, 2 * M_PI), exactly as IEEE fmod (which is exact: the remainder is representable).  For |x| < 2^40 the quotient
// k = trunc(x / m) is found from x * (1/m) -- off by at most one (relative error ~2^-52 on a quotient < 2^38) -- and corrected by
// the sign of the remainder; with the right k, fma(-k, m, x) is the exact remainder rounded once, i.e. the remainder itself.
// Larger and non-finite arguments go to the library fmod.
// Only the corrections towards zero can happen: the double 1.0 / m lies ABOVE the exact reciprocal of the double m (their
// product exceeds 1 by 2.3e-17), so for x >= 0 the rounded product x * (1/m) is never below floor(x / m) (an integer
// < 2^38, representable; rounding is monotonic) and k is the true quotient or one more: r lies in (-m, m), never r >= m; the
// same mirrored for x < 0.  The two branches `r >= m` / `r <= -m` are kept as a guard and are dead for every double
// (tests/test_unwrap_cpu.py takes the census of the branches on the probes of tests/test_gpu_unwrap_limits.py).
__host__ __device__ __forceinline__ double unwrap_fmod_2pi(double x)
{
#pragma clang fp contract(off)
    const double m = 2 * M_PI;
    if (!(fabs(x) < 0x1p40)) return fmod(x, m);
    double k = trunc(x * (1.0 / m));
    double r = fma(-k, m, x);
    if (x >= 0) {
        if (r < 0) k -= 1;
        else if (r >= m) k += 1;
        else return r;
    } else {
        if (r > 0) k += 1;
        else if (r <= -m) k -= 1;
        else return r;
    }
    return fma(-k, m, x);
}

// W(a) of _unwrapping.cpp:22-26: wrap into [-pi, pi).  (fmod's -0 / +0 remainders give the same result.)
__host__ __device__ __forceinline__ double unwrap_W(double a)
{
#pragma clang fp contract(off)
    const double r = unwrap_fmod_2pi(a + M_PI);
    return r >= 0 ? (r - M_PI) : (r + M_PI);
}

// one term of a step (_unwrapping.cpp:106-110): u + tau * W(cur - u), no contraction
__host__ __device__ __forceinline__ void unwrap_term(double &temp, int &S, double u, double cur, double tau)
{
#pragma clang fp contract(off)
    temp += u + tau * unwrap_W(cur - u);
    S += 1;
}

__host__ __device__ __forceinline__ double unwrap_finish(double temp, int S, double cur)
{
    return S > 0 ? temp / (double)S : cur;          // a true division, as the reference
}

// the eight phase values of columns x0 .. x0+7 of one row (0 outside [0, w))
__device__ __forceinline__ void unwrap_load8(const double *__restrict__ row, int x0, int w, double (&v)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int x = x0 + j;
        v[j] = (x >= 0 && x < w) ? row[x] : 0.0;
    }
}

// Dynamic LDS: line[w] then slot[2][blockDim.x] (doubles).  Requires blockDim.x a multiple of 64, <= UNWRAP_MAX_ROWS, and
// w <= UNWRAP_MAX_W (checked by the host).
__global__ __launch_bounds__(UNWRAP_MAX_ROWS) void iir_unwrap_kernel(const double *__restrict__ phase, double *__restrict__ out,
                                                                     int h, int w, double tau)
{
#pragma clang fp contract(off)
    extern __shared__ double uw_lds[];
    double *line = uw_lds;
    double *slot = uw_lds + w;
    const int R = blockDim.x, r = threadIdx.x;
    const size_t map_off = (size_t)blockIdx.x * h * w;
    const double *P = phase + map_off;
    double *O = out + map_off;

    // ---- row 0, passes 1 and 2 (_unwrapping.cpp:95-131): serial, thread 0, in the LDS line
    if (r == 0) {
        double nxt[8], cu[8];
        unwrap_load8(P, 0, w, nxt);
        double prev = 0.0;
        for (int c = 0; c < w; c += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cu[j] = nxt[j];
            unwrap_load8(P, c + 8, w, nxt);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int x = c + j;
                if (x < w) {
                    double temp = 0.0; int S = 0;
                    if (x > 0) unwrap_term(temp, S, prev, cu[j], tau);          // (0, x-1): the only flagged neighbour
                    prev = unwrap_finish(temp, S, cu[j]);
                    line[x] = prev;
                }
            }
        }
        // backward, x = w-1 .. 1: flagged are (0, x-1), (0, x) (pass-1 values) and (0, x+1) (its pass-2 value)
        const int top = ((w - 1) & ~7);
        unwrap_load8(P, top, w, nxt);
        double right = 0.0;
        for (int c = top; c >= 0; c -= 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cu[j] = nxt[j];
            unwrap_load8(P, c - 8, w, nxt);
#pragma unroll
            for (int j = 7; j >= 0; --j) {
                const int x = c + j;
                if (x >= 1 && x < w) {
                    double temp = 0.0; int S = 0;
                    unwrap_term(temp, S, line[x - 1], cu[j], tau);
                    unwrap_term(temp, S, line[x], cu[j], tau);
                    if (x + 1 < w) unwrap_term(temp, S, right, cu[j], tau);
                    right = unwrap_finish(temp, S, cu[j]);
                    line[x] = right;
                }
            }
        }
    }
    __syncthreads();

    // ---- main pass (_unwrapping.cpp:134-149) as a wavefront, one band of R rows at a time
    for (int y0 = 0; y0 < h; y0 += R) {
        const int nb = min(R, h - y0);
        const int y = y0 + r;
        const bool live = r < nb;
        const double *prow = P + (size_t)(live ? y : y0) * w;
        double *orow = O + (size_t)(live ? y : y0) * w;
        const int steps = w + 2 * (nb - 1);
        const bool first_row = (y == 0);
        const bool line_above = (r == 0 && y0 > 0);     // the row above is the previous band's last row, in the line
        double a0 = 0.0, a1 = 0.0, a2 = line_above ? line[0] : 0.0;   // (y-1, x-1), (y-1, x), (y-1, x+1)
        double left = 0.0;                               // (y, x-1)
        double nxt[8], cu[8];
        unwrap_load8(prow, -2 * r, live ? w : 0, nxt);
        for (int c = 0; c < steps; c += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cu[j] = nxt[j];
            unwrap_load8(prow, c + 8 - 2 * r, live ? w : 0, nxt);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = c + j;
                const int x = t - 2 * r;
                // receive (y-1, x+1): produced by thread r-1 at step t-1 (or read from the line)
                double recv = 0.0;
                if (line_above) recv = (x + 1 < w) ? line[x + 1] : 0.0;
                else if (r > 0) recv = slot[((t - 1) & 1) * R + r - 1];
                a0 = a1; a1 = a2; a2 = recv;
                if (live && x >= 0 && x < w) {
                    const double cur = cu[j];
                    double temp = 0.0; int S = 0;
                    if (first_row) {
                        // row 0: (0, x-1) final, (0, x) and (0, x+1) still hold their pass-2 values ((0, 0) its pass-1 value)
                        if (x > 0) unwrap_term(temp, S, left, cur, tau);
                        unwrap_term(temp, S, line[x], cur, tau);
                        if (x + 1 < w) unwrap_term(temp, S, line[x + 1], cur, tau);
                    } else {
                        if (x > 0) unwrap_term(temp, S, a0, cur, tau);
                        unwrap_term(temp, S, a1, cur, tau);
                        if (x + 1 < w) unwrap_term(temp, S, a2, cur, tau);
                        if (x > 0) unwrap_term(temp, S, left, cur, tau);
                    }
                    const double v = unwrap_finish(temp, S, cur);
                    left = v;
                    orow[x] = v;
                    slot[(t & 1) * R + r] = v;
                    if (r == R - 1) line[x] = v;        // hand-off to the next band (its first thread reads it after this band)
                }
                __syncthreads();
            }
        }
    }
}

}  // namespace ssamd
