// Launch planner of the ASW kernels: tile layouts in LDS, the cost model that picks a tile and a kernel form, the wave kernel's
// strip.  Pure integer / double arithmetic: a function of its arguments (shape, window, PlanOptions) -- no HIP call, no global,
// no tune(): the options come in with the caller.  The per-shape caches and the autotuner live with the operators (host_geometry.h, host_asw.h); host_context.h, a host section of ssamd_api.hip, is the only file that includes this
// (behind asw_shared.hip.h and asw_wave_kernel.hip.h: AswGeom, AswWaveGeom, the register-tile constants and round_up are theirs).
#pragma once

enum PlanResult { PLAN_OK = 0, PLAN_FORCED_UNUSABLE, PLAN_NO_FIT };     // (the operators turn these into error codes and messages)

// What the planner reads besides the shape: the caller's snapshot of the tuning options (ssamd_options.h) and one condition of the call.
struct PlanOptions {
    const Tuning &t;
    bool no_volume;           // the call cannot have the TAD volume: a phase-shifted tile must fit LDS with its staged colour bytes
};

// ------------------------------------------------------------ ASW geometry
bool asw_layout_e(AswGeom &g, const PlanOptions &po, int win, int XG, int DG, size_t limit, int JC, int Rx, bool e2, bool odd_pitch = false,
                  bool pipe = false)
{
    g.Rx = Rx;
    g.JC = JC >= win ? win : JC;                 // tap columns staged per chunk; win = the whole row at once
    g.pipe = 0; g.NC = 1; g.JCmax = g.JC; g.dephase = 0; g.wave_rx = 0;
    if (pipe) {
        // phase-shifted kernel (asw_pipe_kernel.hip.h): chunks start at multiples of JC (8 or 16), a tail shorter than
        // the 8-column register tile is merged into the last chunk; needs >= 2 chunks, two e tiles, the 8-column tile
        // chunk starts are multiples of JC (itself a multiple of the register tile's columns); the chunk count is
        // win / JC rounded, the last chunk takes what is left (win 35: JC 16 -> 16, 19; JC 8 -> 8, 8, 8, 11; JC 12 -> 12, 12, 11)
        if (Rx != 8 || JC % Rx || !e2) return false;
        g.NC = (win + JC / 2) / JC;
        if (g.NC < 2 || (g.NC - 1) * JC >= win) return false;
        g.pipe = 1;
        // waves 0-3 build before they aggregate (see the kernel): pays with three or four waves per SIMD (12-wave
        // groups: 1080p/193 41.8 -> 41.0 ms), costs with two (640x480/65, 8 waves: 3.11 -> 3.26 ms)
        g.dephase = po.t.asw_dephase >= 0 ? po.t.asw_dephase : (round_up(XG * DG, 64) / 64 >= 12 ? 1 : 0);
        g.JCmax = std::max(JC, win - (g.NC - 1) * JC);
    }
    const int wrows = g.pipe ? 2 * g.JCmax : (g.JC < win ? 2 * g.JC : win);   // chunk buffers alternate
    const int wcols = g.JC;                      // tap columns a weight-build pass covers

    const int p = win / 2;
    g.XG = XG; g.DG = DG;
    g.Tx = Rx * XG; g.Dc = ASW_RD * DG;
    g.threads = round_up(XG * DG, 64);
    g.nL = g.Tx + 2 * p;
    g.nRc = g.Tx + g.Dc - 1;
    g.nR = g.nRc + 2 * p;
    // parity-split rows (asw_split_pos): two halves of ceil(n/8)*4 floats; +1 block so that the halves
    // start on different banks phases and reads one block past the end stay inside the row
    g.hL = ((g.Tx + 7) / 8) * 4 + 4;
    g.SL = 2 * g.hL;
    g.hR = ((g.nRc + 4 + 7) / 8) * 4 + 4;
    g.SR = 2 * g.hR;
    int P = 8;                                  // dword slots per e row: closed under XOR with emask
    while (P < DG && P < 32) P <<= 1;           //   power of two up to 32, then multiples of 32
    if (P < DG) P = round_up(DG, 32);
    g.Se = 4 * P;
    g.emask = std::min(P, 32) - 1;
    if (odd_pitch) {                            // plain rows with an odd dword pitch instead of the XOR swizzle
        g.Se = 4 * (DG | 1);
        g.emask = 0;
    }
    if (g.pipe) {
        // plain rows, lanes along the disparity groups (asw_pipe_kernel.hip.h): a thread reads floats
        // [8 xg, 8 xg + 8) of a wL row and [8 xg - 4 dg + Dc - 4, + 12) of a wR row (the last one is index nRc, unused)
        g.hL = g.hR = 0;
        g.SL = round_up(g.Tx, 4);
        g.SR = round_up(g.nRc + 1, 4);
        // e rows: one dword per disparity group, pitch a multiple of 16 bytes so that a tile is an aligned contiguous
        // block of the pre-computed volume (LDS-DMA moves 16 bytes per lane)
        g.Se = 16 * ((DG + 3) / 4);
        g.emask = 0;
    }
    // weight build balance: (centres x segments) tasks over the workgroup's threads (asw_aggregate_kernel; the phase-shifted
    // kernel deals whole waves of 64 centres itself and reads neither field)
    {
        const int ncen = g.Tx + g.nRc;
        int best_cost = 1 << 30;
        for (int ns = 1; ns <= wcols && ns <= 8; ++ns) {
            const int len = (wcols + ns - 1) / ns, rounds = (ncen * ns + g.threads - 1) / g.threads;
            const int cost = rounds * (round_up(len, ASW_WB) + 2);       // evaluated in batches of ASW_WB
            if (cost < best_cost) { best_cost = cost; g.wseg = ns; g.wlen = len; }
        }
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return (int)o; };
    g.off_wL = take((size_t)wrows * g.SL * 4);
    g.off_wR = take((size_t)wrows * g.SR * 4);
    g.e_bytes = (int)(((size_t)g.nL * g.Se + 15) & ~(size_t)15);
    g.e2 = (e2 && g.JC < win && (win + g.JC - 1) / g.JC >= 2) ? 1 : 0;
    if (g.pipe && !g.e2) return false;
    g.off_e = take((size_t)g.e_bytes * (g.e2 ? 2 : 1));
    g.off_labL = take((size_t)g.nL * 16 * 2);    // staging is double-buffered (prefetch of the next row)
    g.off_labR = take((size_t)g.nR * 16 * 2);
    if (!g.pipe) {
        g.off_bgrL = take((size_t)g.nL * 4 * 2);
        g.off_bgrR = take((size_t)g.nR * 4 * 2);
    }
    g.off_bestL = take((size_t)g.Tx * 8);
    g.off_bestR = take((size_t)(g.nRc + 1) * 8);
    g.off_cen = take((size_t)(g.Tx + g.nRc) * 16);
    g.off_prox = take((size_t)win * 4 * 2);      // one window row of proximity weights, double-buffered (asw_aggregate_kernel stages it; the
                                                 // phase-shifted kernel reads A.prox with scalar loads and leaves the slot unused)
    g.lds_bytes_evol = (int)off;
    if (g.pipe) {
        // the staged colour bytes only feed the in-kernel e tiles: LAST in the layout, so that a launch that has the pre-computed
        // TAD volume asks for lds_bytes_evol and leaves them out (round 4: LDS is what bounds the resident workgroups of mid-size tiles)
        g.off_bgrL = take((size_t)g.nL * 4 * 2);
        g.off_bgrR = take((size_t)g.nR * 4 * 2);
    }
    g.lds_bytes = (int)off;
    // the phase-shifted kernel normally runs with the TAD volume and then does not allocate the staged colour bytes: a tile is
    // planned on that (round 4, profiles/r04_lds_relax_ab.txt) unless SSAMD_ASW_EVOL=0 says there will be no volume; a call that
    // cannot have the volume after all re-plans with PlanOptions::no_volume set (asw_final_volume)
    if (g.pipe && po.t.asw_evol != 0 && !po.no_volume) return (size_t)g.lds_bytes_evol <= limit;
    return off <= limit;
}

// Chunked geometries first try two e tiles (no row-start barrier, asw_kernels.hip.h); when that does not fit the
// LDS budget they fall back to one.
bool asw_layout(AswGeom &g, const PlanOptions &po, int win, int XG, int DG, size_t limit, int JC = 1 << 20, int Rx = ASW_RX, bool odd_pitch = false)
{
    if (!po.t.no_e2 && asw_layout_e(g, po, win, XG, DG, limit, JC, Rx, true, odd_pitch) && g.e2) return true;
    return asw_layout_e(g, po, win, XG, DG, limit, JC, Rx, false, odd_pitch);
}

// Average number of LDS passes of the aggregation loop's e-row read (one dword per lane; a wave is served in two
// halves of 32 lanes, a pass per distinct address that shares a bank) for an e layout: lanes = consecutive thread
// ids, thread (xg, dg) reads dword dg (XOR-swizzled with row / Rx & emask) of row Rx*xg + n.
double asw_e_read_passes(const AswGeom &g)
{
    const int P = g.Se / 4, T = g.XG * g.DG;
    long long tot = 0, cnt = 0;
    for (int n = 0; n < g.Rx; ++n)
        for (int base = 0; base < T; base += 32) {
            int hits[64] = {0}, worst = 0;
            for (int l = 0; l < 32 && base + l < T; ++l) {
                const int tid = base + l, xg = tid % g.XG, dg = tid / g.XG, ul = g.Rx * xg + n;
                worst = std::max(worst, ++hits[(ul * P + (dg ^ ((ul / g.Rx) & g.emask))) & 63]);
            }
            tot += worst; ++cnt;
        }
    return cnt ? (double)tot / cnt : 1.0;
}

// The e-tile scheme is decided for the chosen tile only (the search prices LDS with the swizzled form): rows with an
// odd dword pitch are smaller (DG|1 instead of a power of two / multiple of 32 dwords) and often conflict less for
// narrow thread grids; the XOR swizzle wins for wide ones.  Take the odd pitch when it makes room for a second e
// tile, or when it does not read slower.
void asw_pick_e_scheme(AswGeom &g, const PlanOptions &po, int win)
{
    if (po.t.xor_only) return;
    AswGeom alt;
    if (!asw_layout(alt, po, win, g.XG, g.DG, 160 * 1024, g.JC >= win ? (1 << 20) : g.JC, g.Rx, true)) return;
    // two e tiles (one barrier less per window row: 1080p/193 45.96 -> 44.7 ms) outweigh a few bank conflicts of a
    // one-dword read; among equals the layout with fewer passes wins
    const bool take = alt.e2 != g.e2 ? alt.e2 > g.e2 : asw_e_read_passes(alt) <= asw_e_read_passes(g) + 1e-9;
    if (take) {
        alt.nchunks = g.nchunks;
        g = alt;
    }
}

// Phase-shifted kernel for a chosen tile (asw_pipe_kernel.hip.h): same XG x DG thread grid and register tile, tap
// columns in chunks of 8 (or 16) with the tail merged, two e tiles.  Taken whenever it fits (8-column tile, window of
// at least two chunks, LDS); the sums and their order are those of asw_aggregate_kernel, so maps do not change.
// SSAMD_ASW_PIPE=0 disables it, =8 / =16 force the chunk length (experiments and tests).
void asw_try_pipe(AswGeom &g, const PlanOptions &po, int win)
{
    const int want = po.t.asw_pipe;
    if (want == 0 || g.Rx != 8) return;
    for (int JC : {16, 8}) {
        if (want > 0 && JC != want) continue;
        // chunks of 8 double the barriers per window row: measured to pay only with three waves per SIMD
        // (4096x2160/257: 265 -> 245 ms, 1080p/129/win 21: 12.7 -> 11.3 ms; 8-wave tiles lose 5-15 %)
        if (want < 0 && JC == 8 && round_up(g.XG * g.DG, 64) / 64 < 12) continue;
        AswGeom alt;
        if (!asw_layout_e(alt, po, win, g.XG, g.DG, 160 * 1024, JC, 8, true, false, true)) continue;
        alt.nchunks = g.nchunks;
        g = alt;
        return;
    }
}

// Wave-autonomous kernel for small disparity ranges (asw_wave_kernel.hip.h): geometry of one wave's strip and its
// slice of LDS.  false: the range does not fit one chunk of at most ASW_WAVE_MAX_DG disparity groups.
static constexpr int ASW_WAVE_MAX_DG = 16;
// One candidate strip: nxg column groups, left / right centres in separate build rounds or merged into one list.
bool asw_wave_layout_one(AswWaveGeom &g, const PlanOptions &po, int win, int DG, int rx, int nxg, bool merged, int rd = ASW_RD, bool creg = false)
{
    g.RX = rx;
    g.RD = rd;
    g.creg = 0;
    const int p = win / 2;
    g.DG = DG;
    g.NXG = nxg;
    g.Txw = rx * g.NXG;
    g.Dc = rd * g.DG;
    g.lanes = g.NXG * g.DG;
    g.nLw = g.Txw + 2 * p;
    g.nRcw = g.Txw + g.Dc - 1;
    g.nRw = g.nRcw + 2 * p;
    g.merged = merged ? 1 : 0;
    if (merged) {
        // one list of Txw + nRcw centres: the right weights follow the left ones directly, the row is padded to whole rounds
        g.K = (g.Txw + g.nRcw + 63) / 64;
        g.SLw = g.Txw;
        g.SRw = round_up(g.Txw + g.nRcw + 1, 64) - g.Txw;
    } else {
        g.K = (g.Txw + 63) / 64 + (g.nRcw + 63) / 64;
        g.SLw = round_up(g.Txw, 64);                   // weight rows padded to whole 64-lane build rounds
        g.SRw = round_up(g.nRcw + 1, 64);
    }
    // bytes per e column: an odd number of dwords, so that the e dwords the lanes of a wave read in one step (column
    // group stride rx * Se) spread over the LDS banks -- with Se = 32 the 12 column groups of D 0..16 all hit the same
    // five banks (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.21)
    g.Se = rd == 6 ? 8 * ((g.DG + 1) | 1) : 4 * (g.DG | 1);        // (six per lane: 8-byte slots, an odd number of them and one to spare)
    g.waves = po.t.wave_wg ? po.t.wave_wg : 1;
    // order matters: the build's last round reads up to 127 entries past the end of the centres and of each pixel
    // row (asw_wave_kernel.hip.h) -- into the array that follows, never past the e tile -- and the merged build
    // relies on pixR starting right behind pixL
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return (int)o; };
    g.off_w = take((size_t)(g.SLw + g.SRw) * 4 * 2);        // two rows: tap columns j and j + 1
    // centres in registers (CREG, asw_wave_front.inc): 4-column tile, merged build of two to four rounds (to three: six per lane)
    g.creg = creg && merged && rx == 4 && g.K >= 2 && (rd == 6 ? g.K <= 3 : g.K <= 4) ? 1 : 0;      // (the instantiations that exist)
    g.off_cen = take(g.creg ? 0 : (size_t)(g.Txw + g.nRcw) * 16);
    g.off_pixL = take((size_t)g.nLw * 16);
    g.off_pixR = take((size_t)g.nRw * 16);
    // (+ rx e columns of slack: the lanes past the last column group read inside the slice.  The six-per-lane kernel clamps
    //  their column group instead, round 4: LDS is granted in 512-byte granules, and at win 35 those 160 bytes decide whether
    //  11 or 12 of its waves are resident per CU -- 13 424 -> 13 264 bytes, 6.06 -> 5.8 ms at 1080p / D 0..16)
    g.off_e = take(std::max((size_t)g.nLw * g.Se, (size_t)(129 + 2 * p) * 16) + (rd == 6 ? 0 : (size_t)rx * g.Se));
    // the winner arrays are only used after the last window row: they share the pixel rows' space
    g.off_bestL = g.off_pixL;
    g.off_bestR = g.off_pixL + (int)(((size_t)g.Txw * 8 + 15) & ~(size_t)15);
    if ((size_t)g.off_bestR + (size_t)(g.nRcw + 1) * 8 > off) off = (size_t)g.off_bestR + (size_t)(g.nRcw + 1) * 8;
    g.wave_lds = (int)((off + 15) & ~(size_t)15);
    return g.off_pixR == g.off_pixL + g.nLw * 16 && (size_t)g.wave_lds * g.waves <= 160 * 1024;
}

// The strip of a wave: DG disparity groups x NXG <= 64 / DG column groups.  Round 3: the number of column groups and
// whether the left and right centres are built as one list are chosen by the cost per column of a tap column's work,
// K build rounds (~17 issue slots each: one weight per lane) + the taps (~59 slots with the 4-column tile, ~110 with
// the 8-column one).  SSAMD_ASW_WAVE_MERGE=0 restores the round-2 form (all column groups, separate rounds).
// rx: 8 or 4 columns per lane; 4 | 16 (= 20, an autotuning candidate, AswGeom::wave_rx): 4 columns and never six disparities per lane
bool asw_wave_layout(AswWaveGeom &g, const PlanOptions &po, int win, int nD, int rx, bool creg = false)
{
    const bool never6 = (rx & 16) != 0;
    rx &= 15;
    const int DG = (nD + ASW_RD - 1) / ASW_RD;
    if (DG < 1 || DG > ASW_WAVE_MAX_DG) return false;
    const int nxg_max = 64 / DG;
    if (po.t.wave_merge == 0) return asw_wave_layout_one(g, po, win, DG, rx, nxg_max, false);
    const double c_round = 17.0, c_taps = rx == 8 ? 110.0 : 59.0;
    double best = 1e30;
    bool found = false;
    // (separate rounds first: on a tie they win -- measured 1.5 % faster at D 0..32, where both forms take three rounds;
    //  the merged form only where its straight-line instantiations exist, K <= 4: the counted loop with its per-round
    //  select lost 7 % at D 0..3, eight rounds instead of nine)
    for (int nxg = nxg_max; nxg >= std::max(1, nxg_max - 4); --nxg)
        for (int merged = 0; merged <= 1; ++merged) {
            AswWaveGeom c;
            if (!asw_wave_layout_one(c, po, win, DG, rx, nxg, merged != 0, ASW_RD, creg)) continue;
            if (merged && c.K > 4) continue;
            if (!merged && nxg != nxg_max) continue;     // fewer column groups only pay through a saved merged round
            const double cost = (c.K * c_round + c_taps) / (double)c.Txw;
            if (cost < best - 1e-9) { best = cost; g = c; found = true; }
        }
    // Six disparities per lane (asw_wave6_kernel.hip.h, 4-column tile, merged rounds only): where the range pads badly to groups of
    // four -- 17 and 18 disparities, the class default among them: three groups of six, 21 column groups, three build rounds
    // for 84 columns -- it must beat the four-per-lane strip by 5 % of the modelled cost to be taken
    if (found && rx == 4 && !never6 && po.t.wave_rd != 4 && po.t.wave_merge != 0) {
        const int DG6 = (nD + 5) / 6;
        if (DG6 >= 1 && DG6 <= 10) {
            const int nxg6 = 64 / DG6;
            for (int nxg = nxg6; nxg >= std::max(1, nxg6 - 4); --nxg) {
                AswWaveGeom c;
                if (!asw_wave_layout_one(c, po, win, DG6, 4, nxg, true, 6, creg) || c.K > 4) continue;
                const double cost = (c.K * c_round + 87.0) / (double)c.Txw;
                if (cost < 0.95 * best) { best = cost / 0.95; g = c; }
            }
        }
    }
    return found;
}

// Which wave kernel (0: none) serves a window / disparity range.  Measured on 1080p and VGA frames, windows 11..35
// (profiles/r02_wave_sweep.txt): the wave kernel beats the workgroup kernels up to 48 disparities; the 4-column tile
// (more waves per SIMD, half the LDS per wave) wins up to 16 disparities, the 8-column tile above.
// Round 3: with the merged build rounds (two rounds for the 32 + 83..95 centres of a four-column-group strip) the wave
// kernel also wins for 49..64 disparities -- 14.0-14.1 ms against 15.9-16.6 ms at 1080p / win 35, 2.64 vs 3.09 ms at VGA
// (profiles/r03_wave_range_49_64_ab.txt); from 65 disparities (three column groups per wave) the phase-shifted kernel is ahead
// again (17.2 vs 18.7 ms at D 0..64), so the limit is 16 disparity groups.
// SSAMD_ASW_WAVE=0 disables it, SSAMD_ASW_WAVE_RX=8|4 forces a tile (experiments / tests); SSAMD_ASW_EVOL=0 (in-kernel e
// tiles) also disables it, the wave kernel needs the TAD volume.
static constexpr int ASW_WAVE_MAX_ND = 64;
int asw_wave_pick(const PlanOptions &po, int win, int nD)
{
    if (po.t.asw_wave == 0 || po.t.asw_evol == 0) return 0;
    if (nD < 1 || nD > ASW_WAVE_MAX_ND || win > 63) return 0;
    AswWaveGeom wg;
    if (const int rx = po.t.wave_rx) {
        return (rx == 8 || rx == 4) && asw_wave_layout(wg, po, win, nD, rx) ? rx : 0;
    }
    // (round 3, merged build rounds: five disparity groups -- 17..20 disparities, the class default among them -- build
    //  48 + 67 centres in two rounds with the 4-column tile: 6.10 vs 6.27 ms at 1080p / D 0..16; from six groups on the
    //  8-column tile wins, 6.69 vs 7.63 ms at D 0..20)
    const int first = nD <= 20 ? 4 : 8, second = 12 - first;
    if (asw_wave_layout(wg, po, win, nD, first)) return first;
    return asw_wave_layout(wg, po, win, nD, second) ? second : 0;
}

// Pick the workgroup tile (XG column groups x DG disparity groups, nchunks disparity chunks)
// with an occupancy-aware cost model calibrated on MI355X (profiles/r01_*):
//   - the kernel needs 168 VGPRs -> 3 waves per SIMD; a workgroup of w waves puts ceil(w/4)
//     on each SIMD, so k = min(floor(3 / ceil(w/4)), floor(160 KiB / LDS)) workgroups are
//     resident per CU.  Measured: 2 x 6-wave groups do NOT co-reside (87 ms), one 12-wave
//     group does (55 ms) on the 1080p/193/35 workload.
//   - per window row a thread spends M cycles aggregating and B cycles building weights / e
//     tiles; B shrinks with the tile (fewer window centres per (x,d) pair).
//   - padding of the disparity range, idle lanes, partial x tiles and the last partial wave of
//     workgroups over the 256 CUs are charged as lost throughput.
// shortlist (autotuning): the best-scoring geometry of every structurally different class of candidates
// (register tile, tap-column chunking, disparity chunks, waves per group), best classes first
PlanResult asw_search_geometry(AswGeom &best, const PlanOptions &po, int W, int rows, int win, int nD, std::vector<AswGeom> *shortlist = nullptr)
{
    std::map<std::array<int, 4>, std::pair<double, AswGeom>> classes;
    // tuning hook: SSAMD_ASW_GEOM="XG,DG[,JC[,RX]]" forces the tile shape (experiments and tests only)
    if (!po.t.asw_geom.empty()) {
        int XG = 0, DG = 0, JCe = 1 << 20, Rx = ASW_RX;
        if (sscanf(po.t.asw_geom.c_str(), "%d,%d,%d,%d", &XG, &DG, &JCe, &Rx) >= 2 && XG > 0 && DG > 0 && XG * DG <= ASW_MAX_THREADS &&
            (Rx == 8 || Rx == 4)) {
            if (JCe <= 0 || JCe % Rx) JCe = 1 << 20;
            if (!asw_layout(best, po, win, XG, DG, 160 * 1024, JCe, Rx)) return PLAN_FORCED_UNUSABLE;
            best.nchunks = (nD + best.Dc - 1) / best.Dc;
            asw_pick_e_scheme(best, po, win);
            asw_try_pipe(best, po, win);
            return PLAN_OK;
        }
    }
    const double c_tap = 10.9, c_w = 70.0, c_e = 60.0, c_stage = 40.0;   // cycles (one SIMD lane-slot)
    double best_score = -1.0;
    bool found = false;
    for (int nch = 1; nch <= nD; ++nch) {
        const int per = (nD + nch - 1) / nch;
        const int DG = round_up(per, ASW_RD) / ASW_RD;
        if (DG > 128) continue;
        if ((nD + DG * ASW_RD - 1) / (DG * ASW_RD) != nch) continue;
        // register tile 8x4 (168 VGPRs: 3 waves per SIMD), or 4x4 (<= 128 VGPRs: 4 waves per SIMD, twice the
        // threads per tile column) for small disparity ranges, where LDS capacity bounds the resident waves
        // (measured, 1080p / win 35: D 0..16 16.7 -> 10.5 ms, D 0..32 14.3 -> 13.2 ms, D 0..47 17.2 -> 14.7 ms,
        //  D 0..64 no gain)
        for (int Rx : {8, 4}) {
        if (Rx == 4 && nD > 56) continue;
        const int max_wps = Rx == 8 ? 3 : 4;
        const int xg_cap = std::min(ASW_MAX_THREADS / DG, (W + Rx - 1) / Rx);
        const int pipe_env = po.t.asw_pipe;
        for (int XG = xg_cap; XG >= 1; --XG)
        for (int cand = 0; cand < 6; ++cand) {
            // candidates 0-3: asw_aggregate_kernel with whole window rows or tap-column chunks of 16 / 8 / 4;
            // candidates 4-5: the phase-shifted kernel (8-column tile) with chunks of 16 / 8
            static const int jcs[6] = {1 << 20, 16, 8, 4, 16, 8};
            const int JC = jcs[cand];
            const bool piped = cand >= 4;
            AswGeom g;
            if (piped) {
                if (Rx != 8 || pipe_env == 0 || (pipe_env > 0 && pipe_env != JC)) continue;
                if (pipe_env < 0 && JC == 8 && round_up(XG * DG, 64) / 64 < 12) continue;      // see asw_try_pipe
                if (!asw_layout_e(g, po, win, XG, DG, 160 * 1024, JC, 8, true, false, true)) continue;
            } else {
                if (JC < (1 << 20) && (JC >= win || JC % Rx)) continue;
                if (!asw_layout(g, po, win, XG, DG, 160 * 1024, JC, Rx)) continue;
            }
            g.nchunks = nch;
            const int waves = g.threads / 64, per_simd = (waves + 3) / 4;
            // (the phase-shifted kernel normally runs with the TAD volume and then leaves the staged colour bytes out of its LDS)
            const int k = std::min(max_wps / per_simd, (160 * 1024) / (piped && po.t.asw_evol != 0 ? g.lds_bytes_evol : g.lds_bytes));
            if (k < 1) continue;
            // per-thread aggregation cycles of one window row; the 4-column tile spends the same address and
            // e-row work on half the taps; the phase-shifted kernel's step is 107 instead of 111 instructions
            // with a third of the bank conflicts
            const double M = (double)win * Rx * ASW_RD * (Rx == 8 ? (piped ? 0.93 * c_tap : c_tap) : c_tap * 1.15);
            const int ncen = g.Tx + g.nRc;
            const int njc = piped ? g.NC : (win + g.JC - 1) / g.JC;     // weight-build passes (= barriers) per window row
            double B;
            if (piped)      // no e tiles (TAD volume), one centre per thread, the build partly under other waves' taps
                B = (double)ncen * win / g.threads * 28.0 + njc * 350.0 + c_stage;
            else
                B = (double)njc * ((ncen * g.wseg + g.threads - 1) / g.threads) * (round_up(g.wlen, ASW_WB) + 2) * c_w +
                    (njc > 1 ? njc * 400.0 : 0.0) +               // extra barriers of the chunked form
                    (double)((g.nL * (g.Dc / 4) + g.threads - 1) / g.threads) * c_e +
                    (double)((g.nL + g.nR + g.threads - 1) / g.threads) * c_stage;
            const double d_util = (double)nD / ((double)nch * g.Dc);
            const int xt = (W + g.Tx - 1) / g.Tx;
            const double x_util = (double)W / ((double)xt * g.Tx);
            const double nwg = (double)xt * std::max(rows, 1) * nch, slots = 256.0 * k;
            const double tail = nwg / (std::ceil(nwg / slots) * slots);
            const double overlap = k > 1 ? 1.05 : 1.0;             // independent groups hide each other's build phase
            // the busiest SIMD carries k*per_simd waves: a group's time scales with per_simd, and fewer
            // resident waves hide less latency (measured: 2 waves/SIMD ~0.85x, 1 wave/SIMD ~0.6x of 3)
            const int wps = k * per_simd;
            const double occ = wps >= 3 ? 1.0 : (wps == 2 ? 0.85 : 0.6);
            const double useful = (double)win * Rx * ASW_RD * c_tap;        // = M for the 8-column tile
            const double score = (double)XG * DG / per_simd * occ * (useful / (M + B)) * d_util * x_util * tail * overlap;
            if (score > best_score) { best_score = score; best = g; found = true; }
            if (shortlist) {
                auto &slot = classes[{piped ? 80 : Rx, std::min(g.JC, 64), nch, waves}];
                if (score > slot.first) slot = {score, g};
            }
        }
        }
        if (DG <= 2) break;
    }
    // Measured exception to the cost model: with the 8-column tile and many disparity groups (DG >= 33, i.e. narrow
    // x tiles under long weight rows) staging the tap columns in chunks of 16 is 1-1.5 % FASTER than whole rows --
    // build and aggregation phases of different waves interleave (1080p/193: 46.9 -> 46.2 ms, 4K/257: 271.9 -> 269.2 ms,
    // 1080p/129: 32.4 -> 32.0 ms) -- while for DG <= 25 it is 4-6 % slower, as the model says.
    if (found && !best.pipe && best.Rx == 8 && best.JC >= win && best.DG >= 33 && win > 16) {
        AswGeom g;
        if (asw_layout(g, po, win, best.XG, best.DG, 160 * 1024, 16, 8)) {
            g.nchunks = best.nchunks;
            best = g;
        }
    }
    if (found && !best.pipe) asw_pick_e_scheme(best, po, win);      // (the phase-shifted form competed in the search above)
    // small disparity ranges: the wave kernel takes over (the workgroup geometry stays as its fallback)
    const int wave_rx = found ? asw_wave_pick(po, win, nD) : 0;
    if (wave_rx) best.wave_rx = wave_rx;
    if (shortlist && found) {
        std::vector<std::pair<double, AswGeom>> v;
        for (auto &kv : classes) v.push_back(kv.second);
        std::sort(v.begin(), v.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
        shortlist->clear();
        if (wave_rx) {          // the model's choice first, then the other tile of the wave kernel, then workgroup geometries
            shortlist->push_back(best);
            AswWaveGeom wg;
            if (!po.t.wave_rx && asw_wave_layout(wg, po, win, nD, 12 - wave_rx)) {
                AswGeom other = best;
                other.wave_rx = 12 - wave_rx;
                shortlist->push_back(other);
            }
            if (wave_rx == 4 && asw_wave_layout(wg, po, win, nD, 4) && wg.RD == 6) {      // ... and the four-per-lane strip next to the six-per-lane one
                AswGeom other = best;
                other.wave_rx = 4 | 16;
                shortlist->push_back(other);
            }
        }
        // every class enters in its phase-shifted form where that exists AND in the plain form: which of the two is
        // faster depends on the tile (waves per SIMD, centres per thread), and the trials measure it
        // (next to the wave kernel only the three best workgroup classes: they have not won a trial for such ranges)
        for (size_t i = 0; i < v.size() && i < (wave_rx ? 3u : 12u) && v[i].first > 0.6 * best_score; ++i) {
            if (!v[i].second.pipe) asw_pick_e_scheme(v[i].second, po, win);
            v[i].second.wave_rx = 0;
            shortlist->push_back(v[i].second);
        }
    }
    return found ? PLAN_OK : PLAN_NO_FIT;
}
