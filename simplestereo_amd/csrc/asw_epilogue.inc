// The epilogue of the four ASW aggregation kernels (asw_aggregate_kernel, _pipe_kernel, _wave_kernel, _wave6_kernel): weighted
// average (_passive.cpp:88) as cost images, the two tile-local winner-take-all reductions, exact mode's near-tie selection, and
// either the disparity map or the merge of the tile's winners into the key images.  Included as the LAST statements of the kernel
// body, after the kernel has cleared bestL / bestR.  Text, not a function: as a __forceinline__ template the same statements moved
// the instruction stream of the tap loops of every instance (DESIGN 4.7); tools/isa_compare.py holds an edit here to its intent.
//
// Kernel locals read by name:  A (AswArgs / AswWaveArgs), RX, accN, accS, bestL, bestR, x0, xrc_lo, dlo, Dc, W, win,
//                              WITH_COSTS (template parameter).
// Macros the kernel defines before the #include (all are #undef'd at the end of this file):
//   ASW_EPI_RD             disparities per thread (second extent of accN / accS)
//   ASW_EPI_LIVE           does this thread hold a register tile?
//   ASW_EPI_XG(live), ASW_EPI_DG(live)
//                          its column / disparity group; `live` is what the place of use knows of ASW_EPI_LIVE (true, or the flag
//                          itself where dead lanes evaluate it too and must get an in-range value)
//   ASW_EPI_TX, ASW_EPI_NRC
//                          columns of the tile, right-image window centres of the tile
//   ASW_EPI_TID, ASW_EPI_NTHR
//                          index and stride of the loops over the tile's columns (thread of the workgroup / lane of the wave)
//   ASW_EPI_SYNC()         barrier among the threads that share bestL / bestR
//   ASW_EPI_ROW            (output row - row0) * W as size_t: an expression, evaluated where it is used
{
    constexpr int RD = ASW_EPI_RD;
    AswKeyTile<RX, RD> kt;                      // cost images of the register tile (exact mode re-reads them after the barrier)
    if (ASW_EPI_LIVE) {
        const int txg = ASW_EPI_XG(true), tdg = ASW_EPI_DG(true);
        u64 diag[RX + RD - 1];
#pragma unroll
        for (int k = 0; k < RX + RD - 1; ++k) diag[k] = KEY_NONE;
#pragma unroll
        for (int xi = 0; xi < RX; ++xi) {
            const int x = x0 + RX * txg + xi;
            u64 bl = KEY_NONE;
#pragma unroll
            for (int di = 0; di < RD; ++di) {
                const int d = dlo + RD * tdg + di;
                const bool valid = (x < W) && (d <= A.maxD) && (x - d >= 0);
                kt.v[xi][di] = 0xffffffffu;
                if (valid) {
                    float c;
                    const u64 hi = (u64)asw_cost_key(accN[xi][di], accS[xi][di], c) << 32;
                    kt.v[xi][di] = (uint32_t)(hi >> 32);
                    bl = min(bl, hi | (u64)(uint32_t)d);
                    diag[xi - di + RD - 1] = min(diag[xi - di + RD - 1], hi | (u64)(uint32_t)x);
                    if (WITH_COSTS)
                        A.costs[((ASW_EPI_ROW) + x) * (A.maxD - A.minD + 1) + (d - A.minD)] = A.cost_keys ? __uint_as_float((uint32_t)(hi >> 32)) : c;
                }
            }
            if (bl != KEY_NONE) atomicMin(&bestL[RX * txg + xi], bl);
        }
        if (A.keyR) {
            const int base = RX * txg - RD * tdg + Dc - RD;
#pragma unroll
            for (int k = 0; k < RX + RD - 1; ++k)
                if (diag[k] != KEY_NONE) atomicMin(&bestR[base + k], diag[k]);
        }
    }
    ASW_EPI_SYNC();
    const size_t rowoff = ASW_EPI_ROW;
    const bool xq = !WITH_COSTS && A.xq.entries != nullptr;          // exact mode: near-ties of the winners go to the fp64 pass's queue
    if (xq) {
        const bool live = ASW_EPI_LIVE;
        const int txg = ASW_EPI_XG(live), tdg = ASW_EPI_DG(live);
        asw_exact_select<RX, RD>(A.xq, live, kt, bestL + RX * txg, A.keyR ? bestR + (RX * txg - RD * tdg + Dc - RD) : nullptr,
                                 x0 + RX * txg, dlo + RD * tdg, (uint32_t)rowoff, exact_zkey(win));
    }
    if (A.disp) {
        for (int k = ASW_EPI_TID; k < ASW_EPI_TX; k += ASW_EPI_NTHR) {
            const int x = x0 + k;
            if (x < W) A.disp[rowoff + x] = bestL[k] == KEY_NONE ? (int16_t)x : (int16_t)(uint32_t)bestL[k];
        }
        return;
    }
    if (xq) {
        // tile-local winners meet the pixels' running minima: the loser of each meeting is queued if it is a near-tie (uniform trip counts)
        for (int k0 = 0; k0 < ASW_EPI_TX; k0 += ASW_EPI_NTHR) {
            const int k = k0 + ASW_EPI_TID, x = x0 + k;
            const bool have = k < ASW_EPI_TX && x < W && bestL[k < ASW_EPI_TX ? k : 0] != KEY_NONE;
            const u64 mine = have ? bestL[k] : KEY_NONE;
            const u64 old = have ? atomicMin(&A.keyL[rowoff + x], mine) : KEY_NONE;
            asw_exact_merge<false>(A.xq, have, mine, old, (uint32_t)rowoff, x, exact_zkey(win));
        }
        if (A.keyR)
            for (int k0 = 0; k0 < ASW_EPI_NRC; k0 += ASW_EPI_NTHR) {
                const int k = k0 + ASW_EPI_TID, xr = xrc_lo + k;
                const bool have = k < ASW_EPI_NRC && (unsigned)xr < (unsigned)W && bestR[k < ASW_EPI_NRC ? k : 0] != KEY_NONE;
                const u64 mine = have ? bestR[k] : KEY_NONE;
                const u64 old = have ? atomicMin(&A.keyR[rowoff + xr], mine) : KEY_NONE;
                asw_exact_merge<true>(A.xq, have, mine, old, (uint32_t)rowoff, xr, exact_zkey(win));
            }
        return;
    }
    for (int k = ASW_EPI_TID; k < ASW_EPI_TX; k += ASW_EPI_NTHR) {
        const int x = x0 + k;
        if (x < W && bestL[k] != KEY_NONE) atomicMin(&A.keyL[rowoff + x], bestL[k]);
    }
    if (A.keyR) {
        for (int k = ASW_EPI_TID; k < ASW_EPI_NRC; k += ASW_EPI_NTHR) {
            const int xr = xrc_lo + k;
            if ((unsigned)xr < (unsigned)W && bestR[k] != KEY_NONE) atomicMin(&A.keyR[rowoff + xr], bestR[k]);
        }
    }
}
#undef ASW_EPI_RD
#undef ASW_EPI_LIVE
#undef ASW_EPI_XG
#undef ASW_EPI_DG
#undef ASW_EPI_TX
#undef ASW_EPI_NRC
#undef ASW_EPI_TID
#undef ASW_EPI_NTHR
#undef ASW_EPI_SYNC
#undef ASW_EPI_ROW
