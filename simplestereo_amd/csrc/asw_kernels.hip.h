// K1: ASW cost aggregation + winner-take-all keys, fused (gfx950).
//
// Replaces the reference hot loop _passive.cpp:34-100 (left-referenced) and, by
// the symmetry of the aggregated cost, also the right-referenced loop
// _passive.cpp:191-253:
//     C(y, xl, xr) = sum_t wL[y,xl,t] wR[y,xr,t] TAD(L[t+xl], R[t+xr]) / sum_t wL wR
// is ONE number used by both passes, so a single evaluation feeds two argmins
// (left: over xr for fixed xl; right: over xl for fixed xr).
//
// Work decomposition
//   workgroup  = (image row y, tile of Tx left columns, chunk of Dc disparities)
//   thread     = register tile of RX=8 columns x RD=4 disparities, 2 fp32 accumulators
//                (N, S' -- see below) per (x,d) pair (RX=4 instantiation for small disparity ranges)
//   outer loop = the window rows i (tap row r = y - pad + i).  Per window row the
//                workgroup stages the pixels it needs in LDS (prefetched one row ahead) and
//                builds, in LDS,
//                  wL[j][x]   left support weights  (x in tile, tap column j)
//                  wR[j][xr]  right support weights (xr = x - d over the tile: they
//                             do not depend on x, the reference re-evaluates them
//                             for every (x,d), _passive.cpp:71-74)
//                  e[u][d]    truncated absolute difference of L[r][u], R[r][u-d]
//                             as bytes: it depends on the tap column u = x+j-pad
//                             only, so each value serves up to `win` taps
//   inner loop = tap columns j; per step a thread reads 8 wL + 12 wR values (five
//                ds_read_b128, 16-byte lane stride thanks to the parity-split rows) and
//                ONE new dword of e (the other seven rows of its window slide in
//                registers), then does 32 taps x {v_mul, 2 v_fma} + 4 x {cvt_ubyte, sub}.
// HBM traffic is the pixel records only (16 B/pixel/image, re-read from L2 by
// neighbouring tiles) plus 8-byte WTA keys; everything else lives in LDS/VGPRs.
// Measured (1080p, D 0..192, win 35): 45.6-46.4 ms, 3.5e10 VALU wave-instructions at ~83 % of the
// plain fp32 issue rate, no scratch, LDS ~50 % busy (profiles/).
#pragma once
#include "asw_shared.hip.h"

namespace ssamd {

// wL / wR rows are stored with their even and odd 16-byte blocks in two halves ("parity split"):
// element c lives at  ((c >> 2) & 1) * half + ((c >> 3) << 2) + (c & 3).  A thread reads RX = 8
// consecutive columns = one even + one odd block, so for each ds_read_b128 the lanes of a wave
// (consecutive column groups) are 16 bytes apart instead of 32: no 2-way bank conflicts.
__device__ __forceinline__ int asw_split_pos(int c, int half)
{
    return ((c >> 2) & 1) * half + ((c >> 3) << 2) + (c & 3);
}

// e tile addressing: rows of Se bytes (Se = 4 * power of two >= DG), one dword (RD = 4 disparities)
// per disparity group; the dword slot of group dg in row ul is XOR-swizzled with (ul / RX) so that
// the lanes of a wave (consecutive xg, rows RX apart) read distinct banks.
template <int RX>
__device__ __forceinline__ int asw_e_offset(int ul, int slot, int Se, int emask)
{
    return ul * Se + ((slot ^ ((ul / RX) & emask)) << 2);
}

// CHUNKED: the tap columns of a window row are staged g.JC at a time (see the loop over jc below).
// RX: columns per thread.  8 is the throughput tile (168 VGPRs, 3 waves per SIMD).  4 halves the columns and
// the accumulators per thread: twice the threads per tile column and 4 waves per SIMD, for small disparity
// ranges where few threads share a weight row and LDS capacity, not VGPRs, limits the resident waves.
template <bool WITH_COSTS, bool CHUNKED, int RX = ASW_RX>
__global__ __launch_bounds__(ASW_MAX_THREADS, RX == 8 ? 3 : 4) void asw_aggregate_kernel(const AswArgs A)
{
    constexpr int NWR = asw_nwr(RX);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const AswGeom &g = A.g;
    float *const wL = reinterpret_cast<float *>(smem + g.off_wL);
    float *const wR = reinterpret_cast<float *>(smem + g.off_wR);
    unsigned char *const eT0 = reinterpret_cast<unsigned char *>(smem + g.off_e);
    float4 *const labL = reinterpret_cast<float4 *>(smem + g.off_labL);
    float4 *const labR = reinterpret_cast<float4 *>(smem + g.off_labR);
    uint32_t *const bgrL = reinterpret_cast<uint32_t *>(smem + g.off_bgrL);
    uint32_t *const bgrR = reinterpret_cast<uint32_t *>(smem + g.off_bgrR);
    u64 *const bestL = reinterpret_cast<u64 *>(smem + g.off_bestL);
    u64 *const bestR = reinterpret_cast<u64 *>(smem + g.off_bestR);
    float4 *const cenLab = reinterpret_cast<float4 *>(smem + g.off_cen);
    float *const proxS = reinterpret_cast<float *>(smem + g.off_prox);

    const int tid = threadIdx.x, nthr = blockDim.x;
    const int W = A.W, win = A.win, p = A.pad;
    const int Tx = g.Tx, Dc = g.Dc, nL = g.nL, nR = g.nR, nRc = g.nRc, SR = g.SR, Se = g.Se, emask = g.emask;
    // XCD-aware tile order: workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8, a
    // speed assumption only).  When the row has a multiple of 8 x tiles, tile slot b of every row lands on
    // XCD b % 8; give each XCD a run of ADJACENT tiles (slots b, b+8, ... -> tiles m*(b%8) + b/8, m = tiles/8)
    // so that the halo columns neighbouring tiles share are served by one L2 instead of two.
    int bx = blockIdx.x;
    if ((gridDim.x & 7) == 0) bx = (bx & 7) * (gridDim.x >> 3) + (bx >> 3);
    const int x0 = bx * Tx;
    const int y = asw_out_row(A, blockIdx.y);
    const int dlo = A.minD + blockIdx.z * Dc;
    const int dhi = dlo + Dc - 1;
    // no (x,d) pair of this tile has x-d >= 0 (left image border): nothing to aggregate; the empty candidate
    // loop of the reference leaves dBest = 0, i.e. the output x (_passive.cpp:54,98)
    if (min(x0 + Tx - 1, W - 1) - dlo < 0) {
        if (A.disp)
            for (int k = threadIdx.x; k < Tx && x0 + k < W; k += blockDim.x)
                A.disp[(size_t)(y - A.row0) * W + x0 + k] = (int16_t)(x0 + k);
        return;
    }

    const int segL_lo = x0 - p;        // first tap column staged from the left image
    const int xrc_lo = x0 - dhi;       // first right-image window centre of the tile
    const int segR_lo = xrc_lo - p;    // first tap column staged from the right image

    // lanes of a wave run along x (xg fastest): their wL / wR reads are consecutive 16-byte
    // slots (conflict-free ds_read_b128 for any lane grouping)

    float accN[RX][ASW_RD], accS[RX][ASW_RD];
#pragma unroll
    for (int a = 0; a < RX; ++a)
#pragma unroll
        for (int b = 0; b < ASW_RD; ++b) { accN[a][b] = 0.f; accS[a][b] = 0.f; }

    for (int k = tid; k < Tx; k += nthr) bestL[k] = KEY_NONE;
    for (int k = tid; k <= nRc; k += nthr) bestR[k] = KEY_NONE;

    // window centres (row y) of the tile: left columns x0.., then right columns xrc_lo..
    for (int c = tid; c < Tx + nRc; c += nthr) {
        const bool isL = c < Tx;
        const int ccol = isL ? x0 + c : xrc_lo + (c - Tx);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)ccol < (unsigned)W) {
            const PixRec q = (isL ? A.recL : A.recR)[(size_t)y * W + ccol];
            v = make_float4(q.L, q.a, q.b, 1.f);
        }
        cenLab[c] = v;
    }
    // e-build task walk: task t -> (ul = t % nL, dq = t / nL), advanced incrementally

    const int i_lo = max(0, p - y), i_hi = min(win, A.H + p - y);
    // stage the pixels of image row r this tile touches into staging buffer `buf`
    // (coalesced 16 B loads; columns outside the image become zero records)
    auto stage_row = [&](int r, int buf) {
        int tids = threadIdx.x;          // opaque copy: keeps the staging indices from being hoisted out of the
        asm volatile("" : "+v"(tids));   // row loop and held (or spilled) across the aggregation
        for (int k = tids; k < win; k += nthr) proxS[buf * win + k] = A.prox[(r - (y - p)) * win + k];
        const PixRec *const rowL = A.recL + (size_t)r * W;
        const PixRec *const rowR = A.recR + (size_t)r * W;
        for (int k = tids; k < nL + nR; k += nthr) {
            const bool isL = k < nL;
            const int idx = isL ? k : k - nL;
            const int col = (isL ? segL_lo : segR_lo) + idx;
            PixRec v;
            v.L = v.a = v.b = 0.f;
            v.bgrx = 0u;
            if ((unsigned)col < (unsigned)W) v = (isL ? rowL : rowR)[col];
            (isL ? labL + buf * nL : labR + buf * nR)[idx] = make_float4(v.L, v.a, v.b, 0.f);
            (isL ? bgrL + buf * nL : bgrR + buf * nR)[idx] = v.bgrx;
        }
    };
    // Tap columns are staged JC at a time when the whole window row of weights does not leave room for
    // enough resident waves (small disparity ranges: few threads share a weight row); chunk buffers
    // alternate so that one barrier per chunk suffices.  JC == win: a single chunk, rows used in place.
    const int JC = CHUNKED ? g.JC : win;
    int cb = 0;
    for (int i = i_lo; i < i_hi; ++i) {
        const int r = y - p + i;

        // per-phase thread indices are re-derived from an opaque copy of the thread id so that
        // they are not kept live across the aggregation loop (168-VGPR budget, no scratch spills)
        int tidb = threadIdx.x;
        asm volatile("" : "+v"(tidb));
        // ---- pixels of image row r were staged into buffer (i & 1) during the previous
        //      iteration's aggregation (prologue for the first row): global latency is hidden
        float4 *const labLc = labL + (i & 1) * nL, *const labRc = labR + (i & 1) * nR;
        uint32_t *const bgrLc = bgrL + (i & 1) * nL, *const bgrRc = bgrR + (i & 1) * nR;
        if (i == i_lo) stage_row(r, i & 1);
        // staged pixels visible; every thread is done with main(i-1).  With two e tiles the barrier is only needed
        // for the first row: the pixels of later rows were staged before an earlier chunk barrier of the previous row,
        // this row's e tile and first weight chunk go to the buffers the previous row's last chunk does not read,
        // and stragglers of that chunk are waited for at this row's first chunk barrier.
        if (!(CHUNKED && g.e2) || i == i_lo) __syncthreads();
        unsigned char *const eT = eT0 + ((CHUNKED && g.e2) ? (i & 1) * g.e_bytes : 0);

        // ---- truncated absolute differences e[ul][d] = min(40, |dB|+|dG|+|dR|) (_passive.cpp:77-79);
        //      pixel bytes are B,G,R,0 so v_sad_u8 sums the 3 channels.  Task = (tap column ul,
        //      pair of disparity groups = 8 disparities); consecutive lanes = consecutive ul.
        {
            const int nsp = (g.DG + 1) >> 1, e_q = nthr / nL, e_r = nthr - e_q * nL;
            int sp = tidb / nL, ul = tidb - sp * nL;
            while (sp < nsp) {
                const uint32_t lp = bgrLc[ul];
                const uint32_t *const rp = bgrRc + (ul + (Dc - 1) - 8 * sp);   // R[u-d] for d = dlo + 8*sp
                uint32_t lo, hi;
                asw_tad8(lp, rp, lo, hi);
                *reinterpret_cast<uint32_t *>(eT + asw_e_offset<RX>(ul, 2 * sp, Se, emask)) = lo;
                if (2 * sp + 1 < g.DG) *reinterpret_cast<uint32_t *>(eT + asw_e_offset<RX>(ul, 2 * sp + 1, Se, emask)) = hi;
                ul += e_r; sp += e_q;
                if (ul >= nL) { ul -= nL; ++sp; }
            }
        }

        // ---- per-row aggregation state (register window of e rows, running e pointer)
        int tidm = threadIdx.x;
        asm volatile("" : "+v"(tidm));
        // a register tile contributes only if some (x,d) of it is a candidate the reference evaluates
        // (x - d >= 0, d <= maxDisparity, x < W); waves whose lanes are all outside (left image border,
        // padded disparities) skip the aggregation -- wave-uniform, decided once per window row
        bool run;
        {
            const int xg = tidm % g.XG, dg = tidm / g.XG;
            const bool tile_live = tidm < g.XG * g.DG && x0 + RX * xg < W && dlo + ASW_RD * dg <= A.maxD &&
                                   x0 + RX * xg + RX - 1 - (dlo + ASW_RD * dg) >= 0;
            run = __builtin_amdgcn_ballot_w64(tile_live) != 0 && tidm < g.XG * g.DG;
        }
        AswRow ew[RX];      // the only per-row state (besides the accumulators) that lives across the chunks' build phases

        for (int jc = 0; jc < win; jc += JC) {
            const int jend = min(win, jc + JC);
            const int rb = CHUNKED ? cb * JC : 0;          // first buffer row of this chunk
            // ---- support weights of window row i, tap columns [jc, jend) (_passive.cpp:47-50 and 71-74;
            //      exp(-dist/gammaC) = exp2(dist*kC)).  Task = (window centre c, segment of the tap
            //      columns); consecutive lanes take consecutive centres: conflict-free ds_read_b128 of the
            //      staged pixels and coalesced LDS writes.  Branch-free: taps or centres outside the image
            //      get weight 0 through a bit mask.
            {
                int tidw = threadIdx.x;
                asm volatile("" : "+v"(tidw));
                const float *const prow = proxS + (i & 1) * win;    // proximity weights of window row i, staged in LDS
                const int ncen = Tx + nRc;
                for (int t = tidw; t < ncen * g.wseg; t += nthr) {
                    const int sgm = t / ncen, c = t - sgm * ncen;
                    const bool isL = c < Tx;
                    const int cc = isL ? c : c - Tx;
                    const float4 cen = cenLab[c];                      // centre pixel (row y); .w = inside image
                    const float4 *const seg = (isL ? labLc : labRc) + cc;
                    const int stride = isL ? g.SL : SR;
                    float *const wout = (isL ? wL : wR) + asw_split_pos(cc, isL ? g.hL : g.hR) + (rb - jc) * stride;
                    const int col0 = (isL ? x0 : xrc_lo) + cc - p;
                    const int j1 = min(jend, jc + (sgm + 1) * g.wlen);
                    const uint32_t cmask = cen.w != 0.f ? 0xffffffffu : 0u;
                    // batches of ASW_WB independent evaluations: all LDS reads first, then the dependent
                    // chains (sub, fma, v_sqrt, v_exp, mul) side by side -- a single chain is ~150 cycles of
                    // latency, and during this phase every wave of the group is in the same loop.  ONE batch body:
                    // entry u is tap at(u) past the column that sp, pp, wp and col stand for.  Whole batches walk
                    // running pointers (staged pixels, proximity row, output column) and take the taps 0, 1, ..;
                    // only the last, partial batch of a segment pays for indices clamped to the segment's end, where
                    // the clamped tap is simply rewritten (straight-line batches of 1 - 3 instead, as the phase-shifted
                    // kernel has them, measured 1.6 - 2.5 % slower here: profiles/fp32_steps_fold.txt).
                    auto batch = [&](const float4 *sp, const float *pp, float *wp, int col, auto at) {
                        float4 tp[ASW_WB];
                        float pr[ASW_WB], wv[ASW_WB];
#pragma unroll
                        for (int u = 0; u < ASW_WB; ++u) { tp[u] = sp[at(u)]; pr[u] = pp[at(u)]; }
#pragma unroll
                        for (int u = 0; u < ASW_WB; ++u) wv[u] = asw_lab_dist2(tp[u], cen);
                        asw_support_weights(wv, A.kC, pr);
#pragma unroll
                        for (int u = 0; u < ASW_WB; ++u) {
                            const uint32_t m = (unsigned)(col + at(u)) < (unsigned)W ? cmask : 0u;
                            wp[at(u) * stride] = __uint_as_float(__float_as_uint(wv[u]) & m);
                        }
                    };
                    int j = jc + sgm * g.wlen;
                    const float4 *sp = seg + j;
                    const float *pp = prow + j;
                    float *wp = wout + j * stride;
                    int col = col0 + j;
                    const int stride4 = ASW_WB * stride;
                    for (; j + ASW_WB <= j1; j += ASW_WB, sp += ASW_WB, pp += ASW_WB, wp += stride4, col += ASW_WB)
                        batch(sp, pp, wp, col, [](int u) { return u; });
                    if (j < j1) batch(seg, prow, wout, col0, [&](int u) { return min(j + u, j1 - 1); });
                }
            }
            __syncthreads();   // e tile and this chunk of wL, wR ready; every thread is done with the previous chunk
            if (jc == 0 && i + 1 < i_hi) stage_row(r + 1, (i + 1) & 1);   // prefetch: overlaps with the aggregation below

            // ---- aggregation over the tap columns of this chunk
            if (run) {
                // thread coordinates, e-row pointer and swizzle state are re-derived per chunk from an opaque thread
                // id: nothing but the e window and the accumulators stays live across a weight-build phase
                int tida = threadIdx.x;
                asm volatile("" : "+v"(tida));
                const int xg = tida % g.XG, dg = tida / g.XG;
                // the next e row to load is ul0 + RX - 1 + jc (ul0 + 0 before the priming of the first chunk); the
                // swizzled dword slot of the thread's disparity group depends on row / RX only, i.e. it changes
                // once per RX tap columns
                const unsigned char *erow = eT + (RX * xg + (jc == 0 ? 0 : RX - 1 + jc)) * Se;
                int q = xg + jc / RX;
                int slotA = (dg ^ (q & emask)) << 2;
                if (jc == 0) {
#pragma unroll
                    for (int n = 0; n < RX - 1; ++n) {
                        asw_row_unpack(ew[n], *reinterpret_cast<const uint32_t *>(erow + slotA));
                        erow += Se;
                    }
                }
                // running LDS pointers (advanced by one tap column per step) keep the address arithmetic at
                // ~4 VALU ops per step and nothing step-specific live across the loop
                // RX = 8: even block of the thread's columns, odd block at + hL;  RX = 4: the thread's single block
                const float *wlp = wL + rb * g.SL + (RX == 8 ? RX / 2 * xg : (xg & 1) * g.hL + ((xg >> 1) << 2));
                // right weights: NWR/4 consecutive 4-float blocks starting at block b0 (parity-split rows)
                const int b0 = (RX * xg - ASW_RD * dg + Dc - ASW_RD) >> 2;
                const float *wrp0 = wR + rb * SR + (b0 & 1) * g.hR + ((b0 >> 1) << 2);
                const float *wrp1 = wR + rb * SR + ((b0 + 1) & 1) * g.hR + (((b0 + 1) >> 1) << 2);
                const float *wrp2 = wR + rb * SR + (b0 & 1) * g.hR + (((b0 + 2) >> 1) << 2);
                for (int j0 = jc; j0 < jend; j0 += RX) {
                    const int slotB = (dg ^ ((q + 1) & emask)) << 2;
#define SSAMD_STEP(JJ, SLOT)                                                                        \
    if (j0 + (JJ) < jend) {                                                                         \
        asw_row_unpack(ew[((JJ) + RX - 1) % RX], *reinterpret_cast<const uint32_t *>(erow + (SLOT))); \
        erow += Se;                                                                                 \
        float wl[RX], wr[NWR];                                                              \
        {                                                                                           \
            const float4 v0 = *reinterpret_cast<const float4 *>(wlp);                              \
            wl[0] = v0.x; wl[1] = v0.y; wl[2] = v0.z; wl[3] = v0.w;                                 \
            if constexpr (RX == 8) {                                                                \
                const float4 v1 = *reinterpret_cast<const float4 *>(wlp + g.hL);                   \
                wl[RX - 4] = v1.x; wl[RX - 3] = v1.y; wl[RX - 2] = v1.z; wl[RX - 1] = v1.w;         \
            }                                                                                       \
            const float4 r0 = *reinterpret_cast<const float4 *>(wrp0);                             \
            const float4 r1 = *reinterpret_cast<const float4 *>(wrp1);                             \
            wr[0] = r0.x; wr[1] = r0.y; wr[2] = r0.z; wr[3] = r0.w;                                 \
            wr[4] = r1.x; wr[5] = r1.y; wr[6] = r1.z; wr[7] = r1.w;                                 \
            if constexpr (RX == 8) {                                                                \
                const float4 r2 = *reinterpret_cast<const float4 *>(wrp2);                         \
                wr[NWR - 4] = r2.x; wr[NWR - 3] = r2.y; wr[NWR - 2] = r2.z; wr[NWR - 1] = r2.w;     \
            }                                                                                       \
        }                                                                                           \
        wlp += g.SL; wrp0 += SR; wrp1 += SR; wrp2 += SR;                                            \
        asw_taps<RX, (JJ)>(accN, accS, wl, wr, ew);                                                 \
    }
                    // the row loaded at step JJ is row j + RX - 1: (row / RX) == q for JJ = 0, q + 1 afterwards
                    SSAMD_STEP(0, slotA) SSAMD_STEP(1, slotB) SSAMD_STEP(2, slotB) SSAMD_STEP(3, slotB)
                    if constexpr (RX == 8) {
                        SSAMD_STEP(RX - 4, slotB) SSAMD_STEP(RX - 3, slotB) SSAMD_STEP(RX - 2, slotB) SSAMD_STEP(RX - 1, slotB)
                    }
#undef SSAMD_STEP
                    slotA = slotB;
                    ++q;
                }
            }
            if (CHUNKED) cb ^= 1;
        }
    }

    // ---- weighted average (_passive.cpp:88), the two WTA reductions, near-tie selection, outputs: asw_epilogue.inc
    int tidf = threadIdx.x;
    asm volatile("" : "+v"(tidf));
#define ASW_EPI_RD ASW_RD
#define ASW_EPI_LIVE (tidf < g.XG * g.DG)
#define ASW_EPI_XG(live) ((live) ? tidf % g.XG : 0)
#define ASW_EPI_DG(live) ((live) ? tidf / g.XG : 0)
#define ASW_EPI_TX Tx
#define ASW_EPI_NRC nRc
#define ASW_EPI_TID tid
#define ASW_EPI_NTHR nthr
#define ASW_EPI_SYNC() __syncthreads()
#define ASW_EPI_ROW (size_t)(y - A.row0) * W
#include "asw_epilogue.inc"
}

}  // namespace ssamd
