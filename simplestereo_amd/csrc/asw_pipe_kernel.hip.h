// K1p: the phase-shifted ("pipelined") form of the ASW aggregation kernel (gfx950).
//
// Same algebra, same per-thread 8 x 4 register tile, same tap order and therefore bit-identical sums as
// asw_aggregate_kernel (asw_kernels.hip.h); what changes is WHEN each wave does its build work.
//
// asw_aggregate_kernel<CHUNKED> runs every wave in lockstep:  build(c) | barrier | aggregate(c) | build(c+1) | barrier ...
// The build work (support weights: LDS read -> 3 sub, 3 fma -> v_sqrt -> v_exp -> LDS write; e tiles; pixel staging)
// is a dependent chain of ~200 cycles with little to overlap it when all twelve waves of the CU are in it at the same
// time: measured, the build phases alone cost 13.8 ms of the 44.5 ms of a 1080p / D 0..192 / win 35 frame although
// their VALU work is worth ~4 ms.
//
// Here the build for the NEXT chunk only touches buffers the current chunk does not read (second weight buffer,
// second e tile, other pixel-staging buffer), so a wave may do it at any point between the chunk's two barriers.
// The twelve waves of a workgroup sit three per SIMD (waves w, w+4, w+8 share a SIMD) and are given three different
// orders, one per SIMD-mate:
//     waves 0-3  : build(next) , aggregate(chunk)
//     waves 4-11 : aggregate(chunk) , build(next)
// so that on every SIMD the first wave's latency-bound build chains are covered by the FMA streams of its two
// mates, and theirs by the first wave's (it starts aggregating later and is still at it when they build).
// One barrier per chunk, as before.
//
// Chunks: tap columns [c*JC, (c+1)*JC) with JC = 8 or 16 and a tail shorter than 8 merged into the last chunk
// (win 35, JC 8: 8, 8, 8, 11), so that the work hidden under a chunk and the chunk itself stay comparable.
// build(next) of chunk c of window row i is
//     c == 0        : stage the pixels of image row i+1 (global -> LDS) + weights of chunk 1
//     0 < c < NC-1  : weights of chunk c+1                              + a share of the e tile of row i+1
//     c == NC-1     : weights of chunk 0 of row i+1                     + the last share of that e tile
// Needs NC >= 2 chunks (the pixels staged under chunk 0 are first read under chunk 1) and two e tiles.
//
// LDS layout ("plain rows", AswGeom::pipe): the lanes of a wave run along the DISPARITY groups of one column group
// (thread = xg * DG + dg), not along x as in asw_aggregate_kernel.  The right-weight blocks a thread reads start at
// float 8 xg - 4 dg + Dc - 4 of a weight row, so consecutive lanes read consecutive 16-byte blocks of a PLAIN row
// (the hardware serves a ds_read_b128 in groups of 16 lanes whose 16-byte slots must differ mod 16: any run of 32
// consecutive blocks does); the left-weight blocks are the same for all lanes of a column group (broadcast); the e
// dwords of a lane group are consecutive in a plain e row.  rocprofv3 on the x-fastest layout with its 15-wide
// thread rows: 21 bank-conflict cycles per 26-cycle aggregation step (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE =
// 0.37, LDS 55 % busy); see profiles/r02_*.  It also needs one running pointer per operand instead of three for
// wR and no swizzle arithmetic.
#pragma once
#include "asw_shared.hip.h"

namespace ssamd {

// (A 6-column register tile -- 48 accumulators, 128 VGPRs, FOUR waves per SIMD in 1024-thread groups, right weights
// read as 8-byte pairs -- was built and measured in round 2: bit-identical maps, 43.6 ms against 38.2 ms for this
// kernel on 1080p / 193 / 35.  A third more LDS traffic per tap outweighs the fourth wave; code removed.)
// SLC, SRC, SEC (round 3): the strides of the left / right weight rows (floats) and of the e rows (bytes) as
// compile-time constants for the launch geometries of the headline configurations (0: read from the geometry at run
// time).  The eight steps of a trip then address their operands with immediate offsets from one pointer per array,
// advanced once per trip: 3 address instructions per 8 steps instead of 24 (107 -> 104.4 VALU instructions per step).
// (Round 6 also built instantiations with the WHOLE tile geometry and the window as constants: 1.7 ... 3.9 % slower,
// profiles/r06_static_geometry_ab.txt; code removed.)
// AswArgs must stay the kernel's ONLY parameter: the item loop reads it at offset 0 of the kernel-argument segment
// (__builtin_amdgcn_kernarg_segment_ptr, see the loop at the end of the body).
template <bool WITH_COSTS, int SLC = 0, int SRC = 0, int SEC = 0>
__global__ __launch_bounds__(ASW_MAX_THREADS, 3) void asw_aggregate_pipe_kernel(const AswArgs A0)
{
    constexpr bool STATIC = SLC > 0;
    constexpr int RX = ASW_RX;
    constexpr int NWR = asw_nwr(RX);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // a static stride triple is one the plain-row layout (asw_layout_e) produces: whole 8-column and 4-disparity groups, e rows of 16-byte blocks
    static_assert(!STATIC || (SLC % 8 == 0 && (SRC - SLC) % 4 == 0 && SEC == 16 * (((SRC - SLC) / 4 + 3) / 4)),
                  "the strides name a tile of the plain-row layout");
    // Persistent form (A.pq != nullptr, see the loop behind this lambda): the ticket of the workgroup's NEXT item, drawn from queue
    // pq_q under the current item and left in a dword of LDS the kernel has no other use for (AswGeom::off_prox)
    uint32_t *const pq_next = reinterpret_cast<uint32_t *>(smem + A0.g.off_prox);
    int pq_q = 0;
    // One work item: the tile (ibx, iby, ibz) of a grid of inx tiles per row -- blockIdx and gridDim.x of the plain launch.  A `return`
    // in here (and in asw_epilogue.inc) ends the item, not the kernel.  A: the kernel's arguments as the item reads them (see the loop).
    auto run_item = [&](const AswArgs &A, const int ibx, const int iby, const int ibz, const int inx) __attribute__((always_inline)) {
    const bool persist = A.pq != nullptr;
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

    const int tid = threadIdx.x, nthr = blockDim.x;
    const int W = A.W, win = A.win, p = A.pad;
    const int Tx = g.Tx, Dc = g.Dc, nL = g.nL, nR = g.nR, nRc = g.nRc, SR = g.SR, Se = g.Se;
    const int JC = g.JC, NC = g.NC;
    // (the row stride as 64 bits, made here as a scalar pair: extended where a lane loop first needs it, inside the item loop the
    //  product became a value of divergent control flow and took two vector registers through the taps)
    size_t Wz = (size_t)W;
    asm volatile("" : "+s"(Wz));
    int bx = ibx;                                 // XCD-aware tile order, see asw_aggregate_kernel
    if ((inx & 7) == 0) bx = (bx & 7) * (inx >> 3) + (bx >> 3);
    const int x0 = bx * Tx;
    const int y = asw_out_row(A, iby);
    const int dlo = A.minD + ibz * Dc;
    const int dhi = dlo + Dc - 1;
    if (min(x0 + Tx - 1, W - 1) - dlo < 0) {      // no candidate the reference evaluates in this tile
        if (A.disp)
            for (int k = threadIdx.x; k < Tx && x0 + k < W; k += blockDim.x)
                A.disp[(size_t)(y - A.row0) * Wz + x0 + k] = (int16_t)(x0 + k);
        if (persist) {
            if (threadIdx.x == 0) *pq_next = atomicAdd(A.pq + pq_q * ASW_PQ_LINE, 1u);
            __syncthreads();
        }
        return;
    }
    // the next ticket: asked for here, waited for behind the first staged row's loads (which are waited for anyway)
    uint32_t pq_ticket = 0;
    if (persist && threadIdx.x == 0) pq_ticket = atomicAdd(A.pq + pq_q * ASW_PQ_LINE, 1u);
    const int segL_lo = x0 - p, xrc_lo = x0 - dhi, segR_lo = xrc_lo - p;
    // which of the two orders this wave follows (0: build first): wave-uniform, kept in a scalar register
    const int phase = g.dephase ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 1;

    float accN[RX][ASW_RD], accS[RX][ASW_RD];
#pragma unroll
    for (int a = 0; a < RX; ++a)
#pragma unroll
        for (int b = 0; b < ASW_RD; ++b) { accN[a][b] = 0.f; accS[a][b] = 0.f; }

    for (int k = tid; k < Tx; k += nthr) bestL[k] = KEY_NONE;
    for (int k = tid; k <= nRc; k += nthr) bestR[k] = KEY_NONE;
    for (int c = tid; c < Tx + nRc; c += nthr) {   // window centres (row y): left columns x0.., right columns xrc_lo..
        const bool isL = c < Tx;
        const int ccol = isL ? x0 + c : xrc_lo + (c - Tx);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)ccol < (unsigned)W) {
            const PixRec q = (isL ? A.recL : A.recR)[(size_t)y * Wz + ccol];
            v = make_float4(q.L, q.a, q.b, 1.f);
        }
        cenLab[c] = v;
    }

    const int i_lo = max(0, p - y), i_hi = min(win, A.H + p - y);

    // ---- build pieces.  Every thread index they use is re-derived from an opaque copy of threadIdx.x so that
    //      nothing of a build stays live across the aggregation (168-VGPR budget, no scratch).
    // pixels of window row i -> staging buffer i & 1  (the proximity row is not staged: build_weights reads A.prox with scalar
    // loads; AswGeom::off_prox stays planned for the kernels that share the layout)
    auto stage_row = [&](int i) {
        int tids = threadIdx.x;
        asm volatile("" : "+v"(tids));
        const int buf = i & 1, r = y - p + i;
        const PixRec *const rowL = A.recL + (size_t)r * Wz;
        const PixRec *const rowR = A.recR + (size_t)r * Wz;
        for (int k = tids; k < nL + nR; k += nthr) {
            const bool isL = k < nL;
            const int idx = isL ? k : k - nL;
            const int col = (isL ? segL_lo : segR_lo) + idx;
            // a tap column outside the image gets L = +inf: colour distance +inf, exp2(-inf) = +0 -- the weight 0 the
            // reference's bounds test gives (_passive.cpp:60-62), exactly and without a mask in the weight build
            PixRec v;
            v.L = __builtin_inff();
            v.a = v.b = 0.f;
            v.bgrx = 0u;
            if ((unsigned)col < (unsigned)W) v = (isL ? rowL : rowR)[col];
            (isL ? labL + buf * nL : labR + buf * nR)[idx] = make_float4(v.L, v.a, v.b, 0.f);
            if (!A.evol) (isL ? bgrL + buf * nL : bgrR + buf * nR)[idx] = v.bgrx;      // (only the in-kernel e tiles read them; not allocated otherwise)
        }
    };
    // tasks [t_lo, t_hi) of the e tile of window row i (task = tap column ul x pair of disparity groups, flat index
    // sp * nL + ul): e[ul][d] = min(40, |dB|+|dG|+|dR|) (_passive.cpp:77-79) from the staged bytes
    auto build_e = [&](int i, int t_lo, int t_hi) {
        int tidb = threadIdx.x;
        asm volatile("" : "+v"(tidb));
        unsigned char *const eT = eT0 + (i & 1) * g.e_bytes;
        const uint32_t *const bgrLc = bgrL + (i & 1) * nL, *const bgrRc = bgrR + (i & 1) * nR;
        const int e_q = nthr / nL, e_r = nthr - e_q * nL;
        int t = t_lo + tidb;
        int sp = t / nL, ul = t - sp * nL;
        while (t < t_hi) {
            const uint32_t lp = bgrLc[ul];
            const uint32_t *const rp = bgrRc + (ul + (Dc - 1) - 8 * sp);   // R[u-d] for d = dlo + 8*sp
            uint32_t lo, hi;
            asw_tad8(lp, rp, lo, hi);
            uint32_t *const dst = reinterpret_cast<uint32_t *>(eT + ul * Se) + 2 * sp;
            dst[0] = lo;
            if (2 * sp + 1 < g.DG) dst[1] = hi;
            t += nthr; ul += e_r; sp += e_q;
            if (ul >= nL) { ul -= nL; ++sp; }
        }
    };
    // the e tile of window row i fetched from the pre-computed volume (A.evol) by LDS-DMA: the tile is ONE contiguous
    // block of nL columns x Se bytes there; every wave moves 1 KiB pieces (64 lanes x 16 B) straight into LDS
    auto load_e = [&](int i) {
        int tidd = threadIdx.x;
        asm volatile("" : "+v"(tidd));
        const int r = y - p + i;
        const unsigned char *const src = A.evol + (((size_t)ibz * A.erows + (r - A.erow0)) * (size_t)A.evolW + x0) * Se;
        unsigned char *const dst = eT0 + (i & 1) * g.e_bytes;
        const int bytes = nL * Se, lane16 = (tidd & 63) * 16;
        for (int k = __builtin_amdgcn_readfirstlane(tidd >> 6) * 1024; k < bytes; k += (nthr >> 6) * 1024)
            if (k + lane16 < bytes)
                __builtin_amdgcn_global_load_lds((const void *)(src + k + lane16),
                                                 (__attribute__((address_space(3))) void *)(dst + k), 16, 0, 0);
    };
    // support weights of window row i, tap columns [jb, je), into weight buffer rows rb.. (_passive.cpp:47-50, 71-74;
    // exp(-dist/gammaC) = exp2(dist*kC)); tap columns outside the image are staged with L = +inf and get weight +0 (centres
    // outside the image only feed candidates the winner-take-all never looks at).
    // The centres are dealt in CENTRE-WAVES of 64, left ones first, and a wave builds whole centre-waves: it never mixes left
    // and right centres, so the staged pixel row, the weight row and its stride are scalars (compile-time strides in the
    // static instantiations: the ASW_WB stores of a batch take immediate offsets from one address), every lane has the same
    // [jb, je) and the trip state lives in scalar registers, and the proximity weight of a tap column is a scalar load from
    // A.prox.  Batches of ASW_WB independent chains, then a straight-line remainder of exactly (je - jb) % ASW_WB weights
    // picked by a scalar branch: no clamped index, no weight computed twice.
    auto build_weights = [&](int i, int jb, int je, int rb) {
        static_assert(ASW_WB == 4, "the remainder below is written out for batches of four");
        typedef const __attribute__((address_space(4))) float cfloat;      // read-only for the whole launch: scalar loads
        int tidw = threadIdx.x;
        asm volatile("" : "+v"(tidw));
        const int wave = __builtin_amdgcn_readfirstlane(tidw >> 6), lane = tidw & 63;
        // (Tx == SL and nRc == SR - 1 are identities of the plain-row layout in asw_layout_e: the strides name the centres and the threads)
        constexpr int NTHR = STATIC ? round_up((SLC / ASW_RX) * ((SRC - SLC) / ASW_RD), 64) : 0;
        const int TxB = STATIC ? SLC : Tx, nRcB = STATIC ? SRC - 1 : nRc, nw = (STATIC ? NTHR : nthr) >> 6;
        const int nLw = (TxB + 63) >> 6, ncw = nLw + ((nRcB + 63) >> 6);
        const float4 *const labLc = labL + (i & 1) * nL, *const labRc = labR + (i & 1) * nR;
        cfloat *const prow = reinterpret_cast<cfloat *>(reinterpret_cast<uintptr_t>(A.prox)) + i * win;
        // N weights of one centre: tap columns sp[0..N), proximity weights pp[0..N), into wp[0], wp[stride], ...
        auto batch = [&](auto n_, const float4 &cen, const float4 *sp, cfloat *pp, float *wp, int stride) {
            constexpr int N = decltype(n_)::value;
            float4 tp[N];
            float pr[N], wv[N];
#pragma unroll
            for (int u = 0; u < N; ++u) { tp[u] = sp[u]; pr[u] = pp[u]; }
#pragma unroll
            for (int u = 0; u < N; ++u) {
                asm volatile("" ::"v"(tp[u].w));     // keeps the read a ds_read_b128 (4 LDS cycles; the 12-byte form takes 8)
                wv[u] = asw_lab_dist2(tp[u], cen);
            }
            asw_support_weights(wv, A.kC, pr);
#pragma unroll
            for (int u = 0; u < N; ++u) wp[u * stride] = wv[u];
        };
        // centre cc (this lane's) of the left / right centres, tap columns [jb_t, je_t)
        auto build_side = [&](auto left_, int cc, int jb_t, int je_t) {
            constexpr bool LEFT = decltype(left_)::value;
            const int stride = LEFT ? (STATIC ? SLC : g.SL) : (STATIC ? SRC : SR);
            if (cc >= (LEFT ? TxB : nRcB)) return;      // lanes past the last centre of the side
            const float4 cen = cenLab[(LEFT ? 0 : TxB) + cc];
            asm volatile("" ::"v"(cen.w));
            const float4 *sp = (LEFT ? labLc : labRc) + cc + jb_t;
            cfloat *pp = prow + jb_t;
            float *wp = (LEFT ? wL : wR) + cc + (rb + jb_t - jb) * stride;
            int j = jb_t;
#pragma nounroll
            for (; j + ASW_WB <= je_t; j += ASW_WB, sp += ASW_WB, pp += ASW_WB, wp += ASW_WB * stride)
                batch(std::integral_constant<int, ASW_WB>{}, cen, sp, pp, wp, stride);
            const int rem = je_t - j;
            if (rem == 1) batch(std::integral_constant<int, 1>{}, cen, sp, pp, wp, stride);
            else if (rem == 2) batch(std::integral_constant<int, 2>{}, cen, sp, pp, wp, stride);
            else if (rem == 3) batch(std::integral_constant<int, 3>{}, cen, sp, pp, wp, stride);
        };
        // tasks: a wave takes whole centre-waves with all columns of the chunk while whole rounds of nw centre-waves last; the
        // centre-waves left over are cut into column segments (multiples of ASW_WB) so that the last round is spread over the
        // waves instead of leaving most of them idle behind a few (tiles with more centres than threads).  All of it is scalar
        // arithmetic on a handful of small numbers: counted out, no division.
        // (Headline tile: 7 centre-waves on 12 waves, so SIMD 3 builds one where the others build two.  Handing batches of centre-waves
        // 4-6 to wave 7, and eight building waves of 60 / 53 lanes, were both measured slower: profiles/r07_pipe_build_uniform.txt.)
        int full = 0;
        while (full + nw <= ncw) full += nw;
        const int rest = ncw - full;
        int slen = je - jb, nseg = 1;
        if (rest > 0 && full > 0) {
            int per = 0;                                   // waves per left-over centre-wave
            for (int a = rest; a <= nw; a += rest) ++per;
            for (slen = ASW_WB; slen * per < je - jb;) slen += ASW_WB;
            while (nseg * slen < je - jb) ++nseg;
        }
        for (int t = wave; t < full + rest * nseg; t += nw) {
            int cw = t, jb_t = jb, je_t = je;
            if (t >= full && nseg > 1) {
                int q = t - full, sgm = 0;
                while (q >= rest) { q -= rest; ++sgm; }
                cw = full + q;
                jb_t = jb + sgm * slen;
                je_t = min(je, jb_t + slen);
            }
            if (cw < nLw) build_side(std::true_type{}, 64 * cw + lane, jb_t, je_t);
            else build_side(std::false_type{}, 64 * (cw - nLw) + lane, jb_t, je_t);
        }
    };
    auto chunk_end = [&](int c) { return c == NC - 1 ? win : (c + 1) * JC; };
    const int nE = nL * ((g.DG + 1) >> 1);             // tasks of one e tile
    // everything chunk c of window row i can hide: see the file header.  cb = weight buffer chunk c reads.
    auto build_next = [&](int i, int c, int cb) {
        const bool more_rows = i + 1 < i_hi;
        if (c == 0 && more_rows) stage_row(i + 1);
        // issued after the staged pixels are in LDS (their global loads are waited for with vmcnt(0), which would
        // also wait for these); lands under the chunk's taps, complete at the next barrier
        if (c == 0 && more_rows && A.evol) load_e(i + 1);
        if (c + 1 < NC || more_rows) {                 // (one call: one copy of the build per wave order)
            const int cn = c + 1 < NC ? c + 1 : 0;
            build_weights(c + 1 < NC ? i : i + 1, cn * JC, chunk_end(cn), (cb ^ 1) * g.JCmax);
        }
        if (c >= 1 && more_rows && !A.evol) build_e(i + 1, (int)((long long)nE * (c - 1) / (NC - 1)), (int)((long long)nE * c / (NC - 1)));
    };

    // ---- prologue: first window row staged, its e tile and its first weight chunk built (not overlapped: 1 / win of the work)
    stage_row(i_lo);
    if (persist && threadIdx.x == 0) *pq_next = pq_ticket;
    if (A.evol) load_e(i_lo);
    __syncthreads();
    if (!A.evol) build_e(i_lo, 0, nE);
    build_weights(i_lo, 0, chunk_end(0), 0);

    // Thread -> (column group xg, disparity group dg), lanes along the disparity groups.  Round 3: a tile at the left
    // image border only has candidates up to d = x (x - d >= 0, _passive.cpp:56), so its threads are dealt over the
    // DGe <= DG disparity groups that hold any: the waves beyond XG * DGe threads skip the tap loops altogether (x tile 0
    // of a 1080p / D 0..192 frame: 30 of 49 groups, 8 of 12 waves; the round-2 mapping kept every wave busy with dead
    // candidates there).  The LDS layout does not depend on the mapping.  (xg, dg) are worked out ONCE and carried in one
    // register: two integer divisions per window row were 1.3 % of the kernel's instructions.
    const int DGe = max(1, min(g.DG, (min(min(x0 + Tx, W) - 1, x0 + Tx - 1) - dlo) / ASW_RD + 1));
    const int nact = g.XG * DGe;
    int pk_xd;
    bool run;          // does this wave hold any candidate the reference evaluates?  (wave-uniform, see asw_aggregate_kernel)
    {
        const int tidm = threadIdx.x;
        int xg, dg;
        // Lane order (round 3).  The LDS serves a ds_read_b128 in groups of 16 lanes and a ds_read_b32 in groups of 32;
        // with thread = xg * DGe + dg and DGe no multiple of 16 (49 at 1080p / D 0..192) a third of the 16-lane groups
        // straddle two column groups, whose right-weight blocks and e dwords then collide (rocprofv3: 23 % of the LDS
        // cycles were bank conflicts).  Here every 16-lane group holds 16 consecutive disparity groups of ONE column
        // group (F = DGe / 16 such groups per column group, in reversed order for odd column groups: the e rows of
        // neighbouring column groups are half the banks apart, so pairs of 16-lane groups stay on disjoint banks);
        // the DGe % 16 left-over disparity groups of all column groups follow at the end.
        const int F = DGe >> 4, Lo = DGe & 15, nfull = g.XG * F;
        const int grp16 = tidm >> 4, r16 = tidm & 15;
        if (grp16 < nfull) {
            xg = grp16 / F;
            int gi = grp16 - xg * F;
            if (xg & 1) gi = F - 1 - gi;
            dg = 16 * gi + r16;
        } else {
            const int q = tidm - 16 * nfull;
            xg = Lo ? q / Lo : g.XG;                 // (q >= XG * Lo: beyond the active threads)
            dg = 16 * F + (Lo ? q - xg * Lo : 0);
        }
        pk_xd = xg | (dg << 16);
        const bool tile_live = tidm < nact && x0 + RX * xg < W && dlo + ASW_RD * dg <= A.maxD &&
                               x0 + RX * xg + RX - 1 - (dlo + ASW_RD * dg) >= 0;
        run = __builtin_amdgcn_ballot_w64(tile_live) != 0 && tidm < nact;
    }

    int cb = 0;
#pragma nounroll
    for (int i = i_lo; i < i_hi; ++i) {
        const unsigned char *const eT = eT0 + (i & 1) * g.e_bytes;
        AswRow ew[RX];

#pragma nounroll                      // (a tap loop per chunk costs VGPRs -> scratch: seen when round 6's whole-geometry form made NC a compile-time 2)
        for (int c = 0; c < NC; ++c) {
            __syncthreads();       // buffers of chunk (i, c) complete; every wave is done with chunk (i, c) - 1
            const int jc = c * JC, jend = chunk_end(c);
            const int rb = cb * g.JCmax;
            // waves 0-3 (one per SIMD) build first, their two SIMD-mates aggregate first and build afterwards
            if (phase == 0) build_next(i, c, cb);
            if (run) {
                // e-row and weight pointers are derived per chunk from the packed thread coordinates: nothing but those,
                // the e window and the accumulators stays live across a build
                const int xg = pk_xd & 0xffff, dg = pk_xd >> 16;
                // the next e row to load is ul0 + RX - 1 + jc (ul0 + 0 before the priming of the window row)
                const unsigned char *erow = eT + (RX * xg + (jc == 0 ? 0 : RX - 1 + jc)) * Se + 4 * dg;
                if (jc == 0) {
#pragma unroll
                    for (int n = 0; n < RX - 1; ++n) {
                        asw_row_unpack(ew[n], *reinterpret_cast<const uint32_t *>(erow));
                        erow += Se;
                    }
                }
                const float *wlp = wL + rb * g.SL + 8 * xg;
                const float *wrp = wR + rb * SR + (RX * xg - ASW_RD * dg + Dc - ASW_RD);
                for (int j0 = jc; j0 < jend; j0 += RX) {
#define SSAMD_PSTEP(JJ)                                                                             \
    if (j0 + (JJ) < jend) {                                                                         \
        const uint32_t epk = *reinterpret_cast<const uint32_t *>(erow + (STATIC ? (JJ) * SEC : 0)); \
        if constexpr (!STATIC) erow += Se;                                                          \
        float wl[RX], wr[NWR];                                                                      \
        {                                                                                           \
            const float *const wl_ = wlp + (STATIC ? (JJ) * SLC : 0);                              \
            const float *const wr_ = wrp + (STATIC ? (JJ) * SRC : 0);                              \
            const float4 v0 = *reinterpret_cast<const float4 *>(wl_);                              \
            wl[0] = v0.x; wl[1] = v0.y; wl[2] = v0.z; wl[3] = v0.w;                                 \
            const float4 v1 = *reinterpret_cast<const float4 *>(wl_ + 4);                          \
            wl[4] = v1.x; wl[5] = v1.y; wl[6] = v1.z; wl[7] = v1.w;                                 \
            const float4 r0 = *reinterpret_cast<const float4 *>(wr_);                              \
            const float4 r1 = *reinterpret_cast<const float4 *>(wr_ + 4);                          \
            const float4 r2 = *reinterpret_cast<const float4 *>(wr_ + 8);                          \
            asm volatile("" ::"v"(r2.w));      /* unused 12th weight: keeps the read a ds_read_b128 */ \
            wr[0] = r0.x; wr[1] = r0.y; wr[2] = r0.z; wr[3] = r0.w;                                 \
            wr[4] = r1.x; wr[5] = r1.y; wr[6] = r1.z; wr[7] = r1.w;                                 \
            wr[8] = r2.x; wr[9] = r2.y; wr[10] = r2.z; wr[11] = r2.w;                               \
        }                                                                                           \
        if constexpr (!STATIC) { wlp += g.SL; wrp += SR; }                                         \
        /* columns 0 .. RX-2 first: the newest e row (tap row j + RX - 1) is only used by the last column and is \
           unpacked into the registers of the oldest row once column 0 is done with that one */       \
        _Pragma("unroll") for (int xi = 0; xi < RX; ++xi) {                                         \
            if (xi == RX - 1) asw_row_unpack(ew[((JJ) + RX - 1) % RX], epk);                        \
            const AswRow &row_ = ew[((JJ) + xi) % RX];                                              \
            _Pragma("unroll") for (int di = 0; di < ASW_RD; ++di) {                                 \
                const float w_ = wl[xi] * wr[xi - di + ASW_RD - 1];                                 \
                accN[xi][di] = fmaf(w_, row_.e[di], accN[xi][di]);                                  \
                accS[xi][di] = fmaf(w_, row_.c[di], accS[xi][di]);                                  \
            }                                                                                       \
        }                                                                                           \
    }
                    SSAMD_PSTEP(0) SSAMD_PSTEP(1) SSAMD_PSTEP(2) SSAMD_PSTEP(3)
                    SSAMD_PSTEP(4) SSAMD_PSTEP(5) SSAMD_PSTEP(6) SSAMD_PSTEP(7)
#undef SSAMD_PSTEP
                    if constexpr (STATIC) { erow += RX * SEC; wlp += RX * SLC; wrp += RX * SRC; }
                }
            }
            if (phase != 0) build_next(i, c, cb);
            cb ^= 1;
        }
    }

    // ---- weighted average (_passive.cpp:88), the two WTA reductions, near-tie selection, outputs: asw_epilogue.inc
    int tidf = threadIdx.x;
    asm volatile("" : "+v"(tidf));
#define ASW_EPI_RD ASW_RD
#define ASW_EPI_LIVE (tidf < nact)
#define ASW_EPI_XG(live) (pk_xd & 0xffff)
#define ASW_EPI_DG(live) (pk_xd >> 16)
#define ASW_EPI_TX Tx
#define ASW_EPI_NRC nRc
#define ASW_EPI_TID tid
#define ASW_EPI_NTHR nthr
#define ASW_EPI_SYNC() __syncthreads()
#define ASW_EPI_ROW (size_t)(y - A.row0) * Wz
#include "asw_epilogue.inc"
    };

    // Plain launch: the grid is the work, one trip.  Persistent launch (round 8): fewer workgroups than items; item id stands for the
    // block (id % nx, id / nx % ny, id / (nx ny)) of the plain grid and goes through the same mapping, so every tile is computed by
    // the same instructions as before.  Queue q holds the ids q, q + 8, ...: a workgroup draws tickets (one lane's atomicAdd, handed
    // round through LDS) from the queue of its XCD, moves on to the next queue when one is exhausted -- a queue never refills, so it
    // never looks back -- and ends behind the eighth.  Nobody waits for anybody: at most items + 8 tickets are drawn per workgroup.
    int dead = 0;
    if (A0.pq) {
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        pq_q = (int)(xcc & (ASW_PQ_QUEUES - 1));
        if (threadIdx.x == 0) *pq_next = atomicAdd(A0.pq + pq_q * ASW_PQ_LINE, 1u);
        __syncthreads();
    }
    for (;;) {
        // Every item reads the arguments from the kernel-argument segment through a pointer the optimiser cannot see through: what
        // an item keeps in scalar registers is then what the one-trip kernel kept, and nothing is carried round the loop for it
        // (with the arguments hoisted out of the loop the kernel spilled scalars into the tap loop and vector registers to scratch).
        typedef const __attribute__((address_space(4))) AswArgs *KernArgs;
        uintptr_t ka = reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr());
        asm volatile("" : "+s"(ka));
        const AswArgs &A = *(const AswArgs *)reinterpret_cast<KernArgs>(ka);
        const bool persist = A.pq != nullptr;
        int ibx = blockIdx.x, iby = blockIdx.y, ibz = blockIdx.z, inx = gridDim.x;
        if (persist) {
            int item = pq_q + ASW_PQ_QUEUES * __builtin_amdgcn_readfirstlane((int)*pq_next);
            while ((unsigned)item >= (unsigned)A.pq_items) {
                if (++dead == ASW_PQ_QUEUES) return;
                pq_q = (pq_q + 1) & (ASW_PQ_QUEUES - 1);
                __syncthreads();       // every thread has read the ticket that is replaced now
                if (threadIdx.x == 0) *pq_next = atomicAdd(A.pq + pq_q * ASW_PQ_LINE, 1u);
                __syncthreads();
                item = pq_q + ASW_PQ_QUEUES * __builtin_amdgcn_readfirstlane((int)*pq_next);
            }
            __syncthreads();           // the last item's reads of bestL / bestR and of the ticket come before this item's writes
            inx = A.pq_nx;
            const int row = item / inx;
            ibx = item - row * inx;
            ibz = row / A.pq_ny;
            iby = row - ibz * A.pq_ny;
        }
        run_item(A, ibx, iby, ibz, inx);
        if (!persist) return;
        if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(A.pq + ASW_PQ_QUEUES * ASW_PQ_LINE), 1ull);      // items finished (ssamd_counter "pipe_persist_items")
    }
}

}  // namespace ssamd
