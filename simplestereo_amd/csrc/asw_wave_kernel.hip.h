// K1w: ASW aggregation for SMALL disparity ranges (the class default maxDisparity = 16; gfx950).
//
// Same algebra, same 8 x 4 register tile, same tap order -- therefore the same sums bit for bit -- as
// asw_aggregate_kernel / asw_aggregate_pipe_kernel; what changes is who builds the support weights.
//
// With few disparities the workgroup kernels starve: a tile of Tx columns x Dc disparities has only Tx * Dc / 32
// threads but needs 2 Tx + Dc weights per tap column in LDS, so at Dc = 20 the double-buffered weight rows allow two
// 4-wave groups per CU (two waves per SIMD), and 28 % of the instructions are support weights behind barriers
// (profiles/r02_asw_default_d16_rocprof_summary.txt: 10.1 ms for 1080p / D 0..16 / win 35 against ~4 ms of work).
//
// Here a WAVE is the unit.  Its 64 lanes are NXG = 64 / DG column groups x all DG disparity groups of one output row
// (lane = xg * DG + dg), i.e. a strip of 8 * NXG columns with the whole disparity range.  Per tap column the wave
//   1. evaluates the 2 * Txw + Dc - 1 support weights its own taps need -- one centre per lane, consecutive lanes
//      consecutive centres -- into a wave-private LDS row (no redundancy inside the strip: every weight is used by
//      all of the wave's disparities),
//   2. runs the 32 taps per lane of that column from it.
// LDS traffic from one wave is served in order, so step 2 sees step 1 without any workgroup barrier; waves never
// wait for each other (a workgroup is just four independent waves), and a wave needs ~13 KB of LDS (pixel row,
// centre pixels, e rows, one weight row), so twelve waves per CU stay resident at 163 VGPRs.
// e tiles come from the TAD volume of asw_tad_volume_kernel (LDS-DMA, one image row at a time).
// Used when the whole range fits one chunk of at most 16 disparity groups (nD <= 64 since round 3; 48 in round 2).
#pragma once
#include "asw_shared.hip.h"
#include <type_traits>

namespace ssamd {

struct AswWaveGeom {
    int RX, DG, NXG, Txw, Dc, lanes;        // columns per lane (8 or 4); disparity groups, column groups and columns per wave, lanes in use
    int nLw, nRcw, nRw;                     // left tap columns, right centres, right tap columns of a wave's strip
    int SLw, SRw, Se;                       // floats per weight row (left / right part), bytes per e column
    int waves;                              // waves per workgroup
    int merged, K;                          // round 3: left and right centres in ONE list of K = ceil((Txw + nRcw) / 64) build rounds
    int RD;                                 // disparities per lane: 4, or 6 (asw_wave6_kernel.hip.h: 8-byte e slots, Se = 8 * odd)
    int creg;                               // round 4: 1 = the window centres live in registers (no cen array in LDS; straight-line merged build only)
    int off_w, off_cen, off_pixL, off_pixR, off_e, off_bestL, off_bestR;     // offsets inside a wave's LDS slice
    int wave_lds;                           // bytes of LDS per wave
};

struct AswWaveArgs {
    const PixRec *recL, *recR;
    const float *prox;
    u64 *keyL, *keyR;
    int16_t *disp;               // non-null: no right-referenced pass -> the wave writes the disparities itself
    float *costs;                // optional raw cost dump
    int cost_keys;               // 1: cost images instead of costs (AswArgs::cost_keys)
    const unsigned char *evol;   // TAD volume (required)
    int erow0, erows, evolW;
    int H, W, win, pad, minD, maxD, row0, rows, ystep;
    int yb0, yskip_at, yskip;    // first workgroup row; second row range (AswArgs::yb0, yskip)
    float kC;
    AswExactQueue xq;            // exact mode: near-tie queue (AswArgs::xq)
    AswWaveGeom g;
};

// wave-local ordering of LDS traffic: nothing may be moved across by the compiler, everything issued has completed
__device__ __forceinline__ void asw_wave_sync()
{
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// LDS instructions of one wave execute in issue order, so a wave's ds_read sees its own earlier ds_write without
// waiting for it; only the compiler must keep the order.
__device__ __forceinline__ void asw_wave_order()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// KL, KR: build rounds (64 centres each) of the left and of the right part when the host knows them at compile time
// (the build is then straight-line code with immediate offsets); 0: counted at run time.
// KM (round 3): rounds of the MERGED build; CREG (round 4): the window centres in registers, which is what the straight-line
// merged build of the 4-column tile does -- both are explained with the build they select, in asw_wave_front.inc.
template <bool WITH_COSTS, int RX, int KL = 0, int KR = 0, int KM = 0>
__global__ __launch_bounds__(256, RX == 8 ? 3 : 4) void asw_aggregate_wave_kernel(const AswWaveArgs A)
{
    static_assert((KL == 0 && KR == 0) || RX == 8, "straight-line separate rounds: measured and instantiated with the 8-column tile only");
    constexpr int NWR = asw_nwr(RX), RD = ASW_RD;
    constexpr bool CREG = RX == 4 && KM > 0;         // (AswWaveGeom::creg must agree: asw_pick_wave_kernel)
    // ---- LDS slice, strip, accumulators, window centres, the merged support-weight build: shared with asw_aggregate_wave6_kernel
#include "asw_wave_front.inc"
    // the separate-rounds build (KL / KR, or counted): the left and the right part of the centre list one after the other
    auto build_part = [&](auto rounds, uint32_t tap_b, uint32_t cen_b, uint32_t dst_b, int n, float pj0, float pj1) {
        asm volatile("" : "+s"(tap_b), "+s"(cen_b), "+s"(dst_b));        // opaque: base + lane sums are formed here, per build
        const uint32_t row1 = (uint32_t)wrow * 4;
        constexpr int K = decltype(rounds)::value;
        if constexpr (K > 0) {                           // round count known (8-column tile only): one address per array, immediate offsets
            const uint32_t ca = cen_b + lane16, ta = tap_b + lane16, da = dst_b + lane4, db_ = da + row1;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const float4 ce0 = ld4(ca + 1024 * r), ta0 = ld4(ta + 1024 * r), tb0 = ld4(ta + 1024 * r + 16);
                asm volatile("" ::"v"(ce0.w), "v"(ta0.w), "v"(tb0.w));   // keeps the reads ds_read_b128
                *(lds_f1)(da + 256 * r) = weight(ce0, ta0, pj0);
                *(lds_f1)(db_ + 256 * r) = weight(ce0, tb0, pj1);
            }
            return;
        }
        int k = 0;
        // 4-column tile: two rounds per trip, all six reads in flight together (the 8-column tile has no registers for that)
        if constexpr (RX == 4) for (; k + 64 < n; k += 128) {
            const uint32_t ca = cen_b + lane16 + k * 16, ta = tap_b + lane16 + k * 16, da = dst_b + lane4 + k * 4;
            const float4 ce0 = ld4(ca), ta0 = ld4(ta), tb0 = ld4(ta + 16);
            const float4 ce1 = ld4(ca + 1024), ta1 = ld4(ta + 1024), tb1 = ld4(ta + 1040);
            asm volatile("" ::"v"(ce0.w), "v"(ta0.w), "v"(tb0.w), "v"(ce1.w), "v"(ta1.w), "v"(tb1.w) : "memory");   // also keeps the reads ds_read_b128
            *(lds_f1)da = weight(ce0, ta0, pj0);
            *(lds_f1)(da + 256) = weight(ce1, ta1, pj0);
            *(lds_f1)(da + row1) = weight(ce0, tb0, pj1);
            *(lds_f1)(da + row1 + 256) = weight(ce1, tb1, pj1);
        }
        for (; k < n; k += 64) {                         // single rounds
            const uint32_t ca = cen_b + lane16 + k * 16, ta = tap_b + lane16 + k * 16, da = dst_b + lane4 + k * 4;
            const float4 ce0 = ld4(ca), ta0 = ld4(ta), tb0 = ld4(ta + 16);
            asm volatile("" ::"v"(ce0.w), "v"(ta0.w), "v"(tb0.w) : "memory");
            *(lds_f1)da = weight(ce0, ta0, pj0);
            *(lds_f1)(da + row1) = weight(ce0, tb0, pj1);
        }
    };
    auto build = [&](int j, float pj0, float pj1) {
        if (KM > 0 || (KL == 0 && KR == 0 && g.merged)) {
            build_merged(sbase + g.off_pixL + 16 * j, sbase + g.off_cen, sbase + g.off_w, pj0, pj1);
            return;
        }
        build_part(std::integral_constant<int, KL>{}, sbase + g.off_pixL + 16 * j, sbase + g.off_cen, sbase + g.off_w, Txw, pj0, pj1);
        build_part(std::integral_constant<int, KR>{}, sbase + g.off_pixR + 16 * j, sbase + g.off_cen + 16 * Txw, sbase + g.off_w + 4 * g.SLw,
                   nRcw, pj0, pj1);
    };

    const int i_lo = max(0, p - y), i_hi = min(win, A.H + p - y);
    int proxv = 0;
    for (int i = i_lo; i < i_hi; ++i) {
        const int r = y - p + i;
        asw_wave_sync();                 // the previous window row's taps are done with the pixel and e rows
        // ---- this image row: e tile by LDS-DMA (one contiguous block of the volume), proxv, Lab of the tap columns
#include "asw_wave_row.inc"
        asw_wave_sync();
        // e window: rows ul = RX xg + n of the tile, dword dg
        const unsigned char *erow = eT + (RX * xg) * Se + 4 * dg;
        AswRow ew[RX];
#pragma unroll
        for (int n = 0; n < RX - 1; ++n) {
            asw_row_unpack(ew[n], *reinterpret_cast<const uint32_t *>(erow));
            erow += Se;
        }
        const float *const wlp = wS + RX * xg;
        const float *const wrp = wS + g.SLw + (RX * xg - ASW_RD * dg + Dc - ASW_RD);

        for (int j0 = 0; j0 < win; j0 += RX) {
#define SSAMD_WSTEP(JJ)                                                                             \
    if (j0 + (JJ) < win) {                                                                          \
        const int j = j0 + (JJ);                                                                    \
        /* 1. even j: the support weights of tap columns j, j + 1 for the strip's centres (_passive.cpp:47-50, 71-74) */ \
        if (((JJ) & 1) == 0) {                                                                      \
            asw_wave_order();                                                                       \
            build(j, __builtin_bit_cast(float, __builtin_amdgcn_readlane(proxv, j)),                \
                  __builtin_bit_cast(float, __builtin_amdgcn_readlane(proxv, j + 1)));              \
            asw_wave_order();                                                                       \
        }                                                                                           \
        const float *const wl_ = wlp + ((JJ) & 1) * wrow, *const wr_ = wrp + ((JJ) & 1) * wrow;     \
        /* 2. the taps of column j (lanes past the last column group read inside the slice and are ignored) */ \
        {                                                                                           \
            const uint32_t epk = *reinterpret_cast<const uint32_t *>(erow);                         \
            erow += Se;                                                                             \
            float wl[RX], wr[NWR];                                                                  \
            {                                                                                       \
                const float4 v0 = *reinterpret_cast<const float4 *>(wl_);                          \
                wl[0] = v0.x; wl[1] = v0.y; wl[2] = v0.z; wl[3] = v0.w;                             \
                if constexpr (RX == 8) {                                                            \
                    const float4 v1 = *reinterpret_cast<const float4 *>(wl_ + 4);                  \
                    wl[RX - 4] = v1.x; wl[RX - 3] = v1.y; wl[RX - 2] = v1.z; wl[RX - 1] = v1.w;     \
                }                                                                                   \
                const float4 r0 = *reinterpret_cast<const float4 *>(wr_);                          \
                const float4 r1 = *reinterpret_cast<const float4 *>(wr_ + 4);                      \
                asm volatile("" ::"v"(r1.w));                                                       \
                wr[0] = r0.x; wr[1] = r0.y; wr[2] = r0.z; wr[3] = r0.w;                             \
                wr[4] = r1.x; wr[5] = r1.y; wr[6] = r1.z; wr[7] = r1.w;                             \
                if constexpr (RX == 8) {                                                            \
                    const float4 r2 = *reinterpret_cast<const float4 *>(wr_ + 8);                  \
                    asm volatile("" ::"v"(r2.w));                                                   \
                    wr[NWR - 4] = r2.x; wr[NWR - 3] = r2.y; wr[NWR - 2] = r2.z; wr[NWR - 1] = r2.w; \
                }                                                                                   \
            }                                                                                       \
            _Pragma("unroll") for (int xi = 0; xi < RX; xi += 2) {                                  \
                /* the products of two columns; (xi, di) and (xi + 1, di + 1) share the right weight.  (As v_pk_mul_f32 pairs */ \
                /* with a broadcast operand -- same IEEE products, 5 instead of 8 instructions -- measured 1.5-4 % slower.) */ \
                float w_[2][ASW_RD];                                                                \
                _Pragma("unroll") for (int di = 0; di + 1 < ASW_RD; ++di) {                         \
                    const float s_ = wr[xi - di + ASW_RD - 1];                                      \
                    w_[0][di] = wl[xi] * s_; w_[1][di + 1] = wl[xi + 1] * s_;                       \
                }                                                                                   \
                w_[0][ASW_RD - 1] = wl[xi] * wr[xi];                                                \
                w_[1][0] = wl[xi + 1] * wr[xi + ASW_RD];                                            \
                _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                     \
                    if (xi + u == RX - 1) asw_row_unpack(ew[((JJ) + RX - 1) % RX], epk);            \
                    const AswRow &row_ = ew[((JJ) + xi + u) % RX];                                  \
                    _Pragma("unroll") for (int di = 0; di < ASW_RD; ++di) {                         \
                        accN[xi + u][di] = fmaf(w_[u][di], row_.e[di], accN[xi + u][di]);           \
                        accS[xi + u][di] = fmaf(w_[u][di], row_.c[di], accS[xi + u][di]);           \
                    }                                                                               \
                }                                                                                   \
            }                                                                                       \
        }                                                                                           \
    }
            SSAMD_WSTEP(0) SSAMD_WSTEP(1) SSAMD_WSTEP(2) SSAMD_WSTEP(3)
            if constexpr (RX == 8) { SSAMD_WSTEP(4) SSAMD_WSTEP(5) SSAMD_WSTEP(6) SSAMD_WSTEP(7) }
#undef SSAMD_WSTEP
        }
    }

    // ---- weighted average (_passive.cpp:88), the two winner-take-all reductions (inside the wave), near-tie selection, outputs:
    //      asw_epilogue.inc, after bestL / bestR are cleared
    asw_wave_sync();
    for (int k = lane; k < Txw; k += 64) bestL[k] = KEY_NONE;        // (these share the pixel rows' space)
    for (int k = lane; k <= nRcw; k += 64) bestR[k] = KEY_NONE;
    asw_wave_sync();
#define ASW_EPI_RD ASW_RD
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
