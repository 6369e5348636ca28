// K1w6: asw_aggregate_wave_kernel with SIX disparities per lane (4 columns x 6 disparities), round 3 (gfx950).
//
// Every BASELINE disparity range is 2^k + 1 values (maxDisparity is inclusive); the class default of both reference
// classes and of the reference's only example, maxDisparity = 16, is 17.  With four disparities per lane that needs five
// disparity groups = 20 padded disparities (15 % of the tap work on candidates that do not exist) and 12 column groups
// x 5 = 60 of 64 lanes.  Three groups of SIX cover 18, 21 column groups x 3 = 63 lanes, and a strip of 84 columns
// builds its 84 + 101 support-weight centres in three merged rounds where the 48-column strip needs two: per column
// of a tap column (3 x 12 + 87) / 84 = 1.46 issue slots instead of (2 x 12 + 59) / 48 = 1.73.
//
// Same algebra, same tap order per (x, d) -- window rows, then tap columns -- therefore the same sums bit for bit as the
// other ASW kernels (tests/test_gpu_asw.py compares them).  What differs from asw_aggregate_wave_kernel:
//   * e tile: one 8-byte slot per disparity group and tap column (bytes 0..5 = the six truncated differences, written by
//     asw_tad_volume_kernel in its rd = 6 mode), read with one ds_read_b64;
//   * right weights: nine consecutive floats from an 8-byte-aligned address (the groups are six apart), five ds_read_b64;
//   * the build is always the merged one (one list of left and right centres).
// Everything up to and including that build, and the staging of an image row, is the wave kernel's text (asw_wave_front.inc,
// asw_wave_row.inc); what is written here is the e window and the tap step.
// Shares AswWaveArgs / AswWaveGeom (RD = 6, Se = bytes per e column) and the host path of the wave kernel.
#pragma once
#include "asw_wave_kernel.hip.h"

namespace ssamd {

struct AswRow6 {
    float e[6], c[6];
};

__device__ __forceinline__ void asw_row_unpack6(AswRow6 &row, const uint2 packed)
{
#pragma unroll
    for (int di = 0; di < 6; ++di) {
        const uint32_t wrd = di < 4 ? packed.x : packed.y;
        const float e = (float)((wrd >> (8 * (di & 3))) & 0xffu);   // v_cvt_f32_ubyteN
        row.e[di] = e;
        row.c[di] = ASW_TAD_CAP - e;
    }
}

// KM: build rounds known at compile time (3 for the class default), 0: counted at run time
// A straight-line build keeps the window centres in registers (CREG, asw_wave_front.inc): no cen array in LDS, two instead of
// three reads per weight pair.
// (Round 4 also built a 128-VGPR form -- four waves per SIMD, build rounds one after the other -- and an e tile without its spare
//  slot, Se = 24: the 96 registers of accumulators and e window leave too little, 6.49 vs 6.07 ms at 1080p / D 0..16 and 4.15 vs
//  3.45 ms with register centres; Se = 24 bought a resident wave at win >= 31 and cost 10-16 % below.  profiles/r04_wave6_*.txt.)
template <bool WITH_COSTS, int KM>
__global__ __launch_bounds__(256, 3) void asw_aggregate_wave6_kernel(const AswWaveArgs A)
{
    // the register-centre build keeps 2 KM tap reads in flight next to 96 registers of accumulators and e window; every instance
    // (asw_instances.inc: KM 0, 2, 3) is measured, and a fourth round has to be measured before it ships
    static_assert(KM <= 3, "asw_wave_front.inc: a register-centre build of KM > 3 rounds has never been measured with this kernel");
    constexpr int RX = 4, RD = 6, NWR = 10;          // nine right weights used, read as five pairs
    constexpr bool CREG = KM > 0;                    // (AswWaveGeom::creg must agree: asw_pick_wave_kernel)
    // ---- LDS slice, strip, accumulators, window centres, the merged support-weight build: shared with asw_aggregate_wave_kernel
#include "asw_wave_front.inc"
    auto build = [&](int j, float pj0, float pj1) { build_merged(sbase + g.off_pixL + 16 * j, sbase + g.off_cen, sbase + g.off_w, pj0, pj1); };

    const int i_lo = max(0, p - y), i_hi = min(win, A.H + p - y);
    int proxv = 0;
    for (int i = i_lo; i < i_hi; ++i) {
        const int r = y - p + i;
        asw_wave_sync();                 // the previous window row's taps are done with the pixel and e rows
        // ---- this image row: e tile by LDS-DMA (one contiguous block of the volume), proxv, Lab of the tap columns
#include "asw_wave_row.inc"
        asw_wave_sync();
        // e window: rows ul = RX xg + n of the tile, 8-byte slot dg
        // (lanes past the last column group -- lane 63 of the 21 x 3 class-default strip -- read the last group's e rows: the tile has no slack behind it)
        const unsigned char *erow = eT + (RX * min(xg, g.NXG - 1)) * Se + 8 * dg;
        AswRow6 ew[RX];
#pragma unroll
        for (int n = 0; n < RX - 1; ++n) {
            asw_row_unpack6(ew[n], *reinterpret_cast<const uint2 *>(erow));
            erow += Se;
        }
        const float *const wlp = wS + RX * xg;
        const float *const wrp = wS + g.SLw + (RX * xg - RD * dg + Dc - RD);

        for (int j0 = 0; j0 < win; j0 += RX) {
#define SSAMD_W6STEP(JJ)                                                                            \
    if (j0 + (JJ) < win) {                                                                          \
        const int j = j0 + (JJ);                                                                    \
        if (((JJ) & 1) == 0) {                                                                      \
            asw_wave_order();                                                                       \
            build(j, __builtin_bit_cast(float, __builtin_amdgcn_readlane(proxv, j)),                \
                  __builtin_bit_cast(float, __builtin_amdgcn_readlane(proxv, j + 1)));              \
            asw_wave_order();                                                                       \
        }                                                                                           \
        const float *const wl_ = wlp + ((JJ) & 1) * wrow, *const wr_ = wrp + ((JJ) & 1) * wrow;     \
        const uint2 epk = *reinterpret_cast<const uint2 *>(erow);                                   \
        erow += Se;                                                                                 \
        float wl[RX], wr[NWR];                                                                      \
        {                                                                                           \
            const float4 v0 = *reinterpret_cast<const float4 *>(wl_);                              \
            wl[0] = v0.x; wl[1] = v0.y; wl[2] = v0.z; wl[3] = v0.w;                                 \
            _Pragma("unroll") for (int k = 0; k < NWR / 2; ++k) {                                   \
                const float2 rr = *reinterpret_cast<const float2 *>(wr_ + 2 * k);                   \
                wr[2 * k] = rr.x; wr[2 * k + 1] = rr.y;                                             \
            }                                                                                       \
        }                                                                                           \
        _Pragma("unroll") for (int xi = 0; xi < RX; ++xi) {                                         \
            if (xi == RX - 1) asw_row_unpack6(ew[((JJ) + RX - 1) % RX], epk);                       \
            const AswRow6 &row_ = ew[((JJ) + xi) % RX];                                             \
            _Pragma("unroll") for (int di = 0; di < RD; ++di) {                                     \
                const float w_ = wl[xi] * wr[xi - di + RD - 1];                                     \
                accN[xi][di] = fmaf(w_, row_.e[di], accN[xi][di]);                                  \
                accS[xi][di] = fmaf(w_, row_.c[di], accS[xi][di]);                                  \
            }                                                                                       \
        }                                                                                           \
    }
            SSAMD_W6STEP(0) SSAMD_W6STEP(1) SSAMD_W6STEP(2) SSAMD_W6STEP(3)
#undef SSAMD_W6STEP
        }
    }

    // ---- weighted average (_passive.cpp:88), the two winner-take-all reductions (inside the wave), near-tie selection, outputs:
    //      asw_epilogue.inc, after bestL / bestR are cleared
    asw_wave_sync();
    for (int k = lane; k < Txw; k += 64) bestL[k] = KEY_NONE;        // (these share the pixel rows' space)
    for (int k = lane; k <= nRcw; k += 64) bestR[k] = KEY_NONE;
    asw_wave_sync();
#define ASW_EPI_RD 6
#define ASW_EPI_LIVE active
#define ASW_EPI_XG(live) xg
#define ASW_EPI_DG(live) dg
#define ASW_EPI_TX Txw
#define ASW_EPI_NRC nRcw
#define ASW_EPI_TID lane
#define ASW_EPI_NTHR 64
#define ASW_EPI_SYNC() asw_wave_sync()
#define ASW_EPI_ROW orow
#include "asw_epilogue.inc"
}

}  // namespace ssamd
