// The ASW pre-pass kernels: the truncated-absolute-difference volume the phase-shifted and the wave kernels fetch their e tiles
// from (K0e), alone or in one launch with the Lab records (K0).
#pragma once
#include "common.hip.h"
#include "lab_kernels.hip.h"

namespace ssamd {

// K0e: the truncated absolute differences e[r][u][d] = min(40, |dB|+|dG|+|dR|) of L[r][u] and R[r][u-d]
// (_passive.cpp:77-79) for every image row the launch touches, as bytes in exactly the layout of the kernel's e
// tiles: [disparity chunk z][row][column u + pad][Se bytes = one dword per 4 disparities, padded].  e depends on
// (r, u, d) only, so each value is needed by the up to winSize window rows of winSize output rows: built once here
// (H*W*nD bytes: 0.4 GB at 1080p / 193, a 0.1 ms HBM-bound kernel) instead of winSize times inside the aggregation
// kernel, whose workgroups then fetch their tiles with LDS-DMA (global_load_lds_dwordx4: no VALU work, no
// registers).  Columns or disparities outside the image get 0; their taps carry weight 0.
// Workgroup = one image row x 64 columns x one disparity chunk.  The pixels are staged in LDS (coalesced record
// reads), every thread then produces whole dwords (4 disparities) of one column, and the 64 x Se byte block -- a
// contiguous piece of the volume -- is written with consecutive lanes on consecutive dwords.
static constexpr int TADV_COLS = 64;
// One tile (bx, by, bz) of the volume.  BYTES: the pixels come straight from the caller's uint8 [H][W][3] images instead of the
// records -- the volume then does not depend on the Lab conversion and both run in ONE launch (asw_prepass_kernel below).
template <bool BYTES>
__device__ __forceinline__ void asw_tad_tile(const void *__restrict__ srcL, const void *__restrict__ srcR, unsigned char *__restrict__ evol,
                                             int W, int pad, int minD, int Dc, int Se, int erow0, int erows, int evolW, int rd, long long npix_total,
                                             int bx, int by, int bz, char *smem)
{
    uint32_t *const sL = reinterpret_cast<uint32_t *>(smem);                 // [TADV_COLS]
    uint32_t *const sR = sL + TADV_COLS;                                     // [TADV_COLS + Dc]: right columns u0 - dhi .. u0 + 63 - dlo
    const int r = erow0 + by, z = bz, uc0 = bx * TADV_COLS;
    const int P = Se >> 2, dlo = minD + z * Dc, dhi = dlo + Dc - 1;
    const int u0 = uc0 - pad, xr0 = u0 - dhi;
    auto pixel = [&](const void *src, int col) -> uint32_t {
        const size_t q = (size_t)r * W + col;
        if constexpr (BYTES) {
            return load_bgr(reinterpret_cast<const uint8_t *>(src), (long long)q, npix_total);
        } else {
            return reinterpret_cast<const PixRec *>(src)[q].bgrx;
        }
    };
    for (int k = threadIdx.x; k < 2 * TADV_COLS + Dc; k += blockDim.x) {
        const bool isL = k < TADV_COLS;
        const int col = isL ? u0 + k : xr0 + (k - TADV_COLS);
        // bit 31 marks a column outside the image (pixel bytes never set it): its e values are 0
        const uint32_t v = (unsigned)col < (unsigned)W ? pixel(isL ? srcL : srcR, col) : 0x80000000u;
        (isL ? sL : sR)[isL ? k : k - TADV_COLS] = v;
    }
    __syncthreads();
    const int ncols = min(TADV_COLS, evolW - uc0);
    uint32_t *const out = reinterpret_cast<uint32_t *>(evol + (((size_t)z * erows + by) * (size_t)evolW + uc0) * Se);
    // rd = 4: dword `slot` of a column holds the disparities dlo + 4 slot + 0..3;  rd = 6 (asw_wave6_kernel.hip.h): a
    // disparity group is an 8-byte slot, dword 2 g holds dlo + 6 g + 0..3 and dword 2 g + 1 holds dlo + 6 g + 4, 5
    auto dword = [&](int c, int slot, uint32_t lp) {
        uint32_t v = 0;
        const int d0 = rd == 6 ? 6 * (slot >> 1) + 4 * (slot & 1) : 4 * slot, nv = rd == 6 && (slot & 1) ? 2 : 4;
        if (!(lp >> 31) && d0 < Dc) {
            // R[u - d] for d = dlo + d0 + q  ->  staged index c + (Dc - 1) - d0 - q
            const uint32_t *const rp = sR + c + (Dc - 1) - d0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t rv = q < nv && d0 + q < Dc ? rp[-q] : 0x80000000u;
                if (!(rv >> 31)) v |= asw_tad(lp, rv) << (8 * q);
            }
        }
        return v;
    };
    if ((P & 3) == 0) {
        // rows of whole 16-byte blocks (the phase-shifted kernel's layout): a thread produces 16 disparities and one
        // 16-byte store -- 1 KiB per wave and store instruction instead of 256 B
        const int P4 = P >> 2;
        uint4 *const out4 = reinterpret_cast<uint4 *>(out);
        for (int k = threadIdx.x; k < ncols * P4; k += blockDim.x) {
            const int c = k / P4, s4 = 4 * (k - c * P4);
            const uint32_t lp = sL[c];
            out4[k] = make_uint4(dword(c, s4, lp), dword(c, s4 + 1, lp), dword(c, s4 + 2, lp), dword(c, s4 + 3, lp));
        }
        return;
    }
    for (int k = threadIdx.x; k < ncols * P; k += blockDim.x) {
        const int c = k / P, slot = k - c * P;
        out[k] = dword(c, slot, sL[c]);
    }
}

__global__ __launch_bounds__(256) void asw_tad_volume_kernel(const PixRec *__restrict__ recL, const PixRec *__restrict__ recR,
                                                             unsigned char *__restrict__ evol, int W, int pad, int minD, int Dc,
                                                             int Se, int erow0, int erows, int evolW, int rd = 4)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    asw_tad_tile<false>(recL, recR, evol, W, pad, minD, Dc, Se, erow0, erows, evolW, rd, 0, blockIdx.x, blockIdx.y, blockIdx.z, smem);
}

// K0 + K0e in ONE launch (round 5): the first `lab_blocks` workgroups convert the pixels of the rows [erow0, erow0 + erows) of both
// images into records (bgr2lab_records_pair_kernel's job by the same function, lab_records_pair), the others each build one tile of
// the volume from the images' bytes.  The two jobs do not depend on each other, so a small-frame call is two dependent launches instead of three
// (a launch-to-launch dependency costs more than either kernel at Tsukuba size).  bgrL / bgrR: the sub-image's row 0.
struct AswPrepassArgs {
    const uint8_t *bgrL, *bgrR;
    PixRec *recL, *recR;
    unsigned char *evol;
    long long npix_total;            // pixels of the whole sub-image (bounds of the 4-byte pixel reads)
    int W, pad, minD, Dc, Se, erow0, erows, evolW, rd;
    int lab_blocks, ex, ey;          // grid: lab_blocks + ex * ey * ez workgroups
};
__global__ __launch_bounds__(256) void asw_prepass_kernel(const AswPrepassArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < P.lab_blocks) {
        SSAMD_LAB_TABLES_IN_LDS(T)
        const long long np = (long long)P.erows * P.W, first = (long long)P.erow0 * P.W;
        const uint8_t *const bl = P.bgrL + 3 * first, *const br = P.bgrR + 3 * first;
        lab_records_pair(P.recL + first, P.recR + first, np, P.lab_blocks, T,
                         [&](bool right, long long p) { return load_bgr(right ? br : bl, p, np); });
        return;
    }
    const int b = (int)blockIdx.x - P.lab_blocks, bx = b % P.ex, by = (b / P.ex) % P.ey, bz = b / (P.ex * P.ey);
    asw_tad_tile<true>(P.bgrL, P.bgrR, P.evol, P.W, P.pad, P.minD, P.Dc, P.Se, P.erow0, P.erows, P.evolW, P.rd, P.npix_total, bx, by, bz, smem);
}

}  // namespace ssamd
