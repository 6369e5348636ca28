// K2: from winner-take-all keys to the disparity map -- plain decode, or left-right check with occlusion filling.  The ASW and
// the GSW operators both finish with these.
#pragma once
#include "common.hip.h"

namespace ssamd {

// K2a: decode left keys (non-consistent mode).  disparity = d of the best key, or x
// when the candidate loop was empty (dBest stays 0, _passive.cpp:54,98).
// right_keys != 0: the keys are right-referenced (low word = best LEFT column of the right pixel, 0 when its
// candidate loop was empty, _passive.cpp:209) -- only used by the verification dump ssamd_asw_argmins.
__global__ __launch_bounds__(256) void wta_decode_kernel(const u64 *__restrict__ keyL, int16_t *__restrict__ disp,
                                                         int rows, int W, int right_keys)
{
    const long long n = (long long)rows * W;
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; idx < n; idx += stride) {
        const u64 k = keyL[idx];
        const int x = right_keys ? 0 : (int)(idx % W);
        disp[idx] = (k == KEY_NONE) ? (int16_t)x : (int16_t)(uint32_t)k;
    }
}

// K2b: left-right check + occlusion filling, one workgroup per image row
// (_passive.cpp:250-285; GSW 661-696).  keyR low word = best left column for the
// right pixel, 0 when its candidate loop was empty (dBest stays 0, :209).
// A left pixel is invalidated iff some right pixel selects it while the left
// disparity disagrees; this is order independent, unlike the reference's
// sequential formulation.  Runs of invalid pixels take min(left,right) valid
// neighbour, or the single valid neighbour at the image border.  A fully invalid
// row keeps -1 (the reference reads out of bounds there).
__global__ __launch_bounds__(256) void lr_check_fill_kernel(const u64 *__restrict__ keyL, const u64 *__restrict__ keyR,
                                                            int16_t *__restrict__ disp, int rows, int W)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int16_t *d = reinterpret_cast<int16_t *>(smem);
    unsigned char *inv = reinterpret_cast<unsigned char *>(smem + (((size_t)W * 2 + 15) & ~(size_t)15));
    const int y = blockIdx.x;
    const u64 *kl = keyL + (size_t)y * W, *kr = keyR + (size_t)y * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const u64 k = kl[x];
        d[x] = (k == KEY_NONE) ? (int16_t)x : (int16_t)(uint32_t)k;
        inv[x] = 0;
    }
    __syncthreads();
    for (int xr = threadIdx.x; xr < W; xr += blockDim.x) {
        const u64 k = kr[xr];
        const int best = (k == KEY_NONE) ? 0 : (int)(uint32_t)k;
        if ((int)d[best] != best - xr) inv[best] = 1;
    }
    __syncthreads();
    int16_t *out = disp + (size_t)y * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        int16_t v = d[x];
        if (inv[x]) {
            int lo = x - 1, hi = x + 1;
            while (lo >= 0 && inv[lo]) --lo;
            while (hi < W && inv[hi]) ++hi;
            if (lo < 0 && hi >= W) v = -1;
            else if (lo < 0) v = d[hi];
            else if (hi >= W) v = d[lo];
            else v = min(d[lo], d[hi]);
        }
        out[x] = v;
    }
}

}  // namespace ssamd
