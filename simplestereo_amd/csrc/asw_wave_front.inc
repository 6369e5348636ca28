// The front half of the two wave kernels (asw_aggregate_wave_kernel, asw_aggregate_wave6_kernel): the wave's LDS slice and strip,
// the early exits, the cleared accumulators, the window centres (in registers or in LDS), the LDS address helpers and the merged
// support-weight build of two tap columns.  Included ONCE, as the first statements of the kernel body after the kernel's own
// constants; asw_wave_row.inc (inside the loop over window rows) and asw_epilogue.inc (last) use the names it defines.
// Text, not functions: with the staging block and the best-row clear as lambdas the same statements changed every instance of
// the two kernels (24 then, DESIGN 4.7); tools/isa_compare.py holds an edit here to its intent.
//
// Read by name:      A (AswWaveArgs), threadIdx, blockIdx; template parameter KM; the constant CREG each kernel derives from its
//                    template parameters (4-column tile and KM > 0: the straight-line merged build has its centres in registers;
//                    without them a straight-line merged build is the 8-column tile's); RX and RD (columns and disparities per
//                    lane: the second extent of accN / accS), which the wave kernel has as template parameter / constant and the
//                    six-per-lane kernel as constants.
// Defined, used by the kernels, asw_wave_row.inc and asw_epilogue.inc:
//   g, lane, wave, smem; the slice's arrays wS, cenLab, pixL, pixR, eT, bestL, bestR
//   W, win, p, Txw, Dc, nLw, nRcw, nRw, Se, x0, y, dlo, dhi, orow, segL_lo, xrc_lo, segR_lo, ncen, xg, dg, active
//   accN, accS (zero), cenx / ceny / cenz (CREG)
//   v4f, lds_v4, lds_f1, ld4, sbase, lane16, lane4, weight, wrow -- the wave kernel's separate-rounds build uses these too
//   tapoff, build_merged(tap_b, cen_b, dst_b, pj0, pj1)
// May return from the kernel: a strip right of the image, or one without a candidate the reference evaluates.
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const AswWaveGeom &g = A.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    char *const smem = smem_all + wave * g.wave_lds;
    float *const wS = reinterpret_cast<float *>(smem + g.off_w);            // [SLw + SRw]: left weights, then right weights
    float4 *const cenLab = reinterpret_cast<float4 *>(smem + g.off_cen);    // [Txw + nRcw]
    float4 *const pixL = reinterpret_cast<float4 *>(smem + g.off_pixL);     // [nLw] Lab of the current image row
    float4 *const pixR = reinterpret_cast<float4 *>(smem + g.off_pixR);     // [nRw]
    unsigned char *const eT = reinterpret_cast<unsigned char *>(smem + g.off_e);   // [nLw][Se]
    u64 *const bestL = reinterpret_cast<u64 *>(smem + g.off_bestL);
    u64 *const bestR = reinterpret_cast<u64 *>(smem + g.off_bestR);

    const int W = A.W, win = A.win, p = A.pad;
    const int Txw = g.Txw, Dc = g.Dc, nLw = g.nLw, nRcw = g.nRcw, nRw = g.nRw, Se = g.Se;
    const int x0 = (blockIdx.x * g.waves + wave) * Txw;
    if (x0 >= W) return;                                         // (no workgroup barrier anywhere: waves are independent)
    const int y = asw_out_row(A, blockIdx.y);
    const int dlo = A.minD, dhi = dlo + Dc - 1;
    const size_t orow = (size_t)(y - A.row0) * W;
    if (min(x0 + Txw - 1, W - 1) - dlo < 0) {                   // no candidate the reference evaluates in this strip
        if (A.disp)
            for (int k = lane; k < Txw && x0 + k < W; k += 64) A.disp[orow + x0 + k] = (int16_t)(x0 + k);
        return;
    }
    const int segL_lo = x0 - p, xrc_lo = x0 - dhi, segR_lo = xrc_lo - p;
    const int ncen = Txw + nRcw;
    const int xg = lane / g.DG, dg = lane - xg * g.DG;
    const bool active = lane < g.lanes;

    float accN[RX][RD], accS[RX][RD];
#pragma unroll
    for (int a = 0; a < RX; ++a)
#pragma unroll
        for (int b = 0; b < RD; ++b) { accN[a][b] = 0.f; accS[a][b] = 0.f; }
    float cenx[CREG ? KM : 1], ceny[CREG ? KM : 1], cenz[CREG ? KM : 1];      // CREG: Lab of the centres lane, lane + 64, ... (row y)
    if constexpr (CREG) {
#pragma unroll
        for (int r = 0; r < KM; ++r) {
            const int c = 64 * r + lane;
            const bool isL = c < Txw;
            const int ccol = isL ? x0 + c : xrc_lo + (c - Txw);
            cenx[r] = ceny[r] = cenz[r] = 0.f;
            if (c < ncen && (unsigned)ccol < (unsigned)W) {
                const PixRec q = (isL ? A.recL : A.recR)[(size_t)y * W + ccol];
                cenx[r] = q.L; ceny[r] = q.a; cenz[r] = q.b;
            }
        }
    } else {
        for (int c = lane; c < ncen; c += 64) {                  // window centres (row y)
            const bool isL = c < Txw;
            const int ccol = isL ? x0 + c : xrc_lo + (c - Txw);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)ccol < (unsigned)W) {
                const PixRec q = (isL ? A.recL : A.recR)[(size_t)y * W + ccol];
                v = make_float4(q.L, q.a, q.b, 1.f);
            }
            cenLab[c] = v;
        }
    }
    // Support weights of one tap column: lane l evaluates the centres l, l + 64, ... of the left and of the right part.
    // A tap column outside the image has L = +inf and so a zero weight; centres outside the image only feed candidates
    // the winner-take-all never looks at.
    // Addresses are LDS byte offsets = a wave-uniform base (SGPR) + the lane's 16 * lane or 4 * lane: the only vector
    // registers the build keeps between steps are those two (pointers per array would not fit next to the accumulators).
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const v4f *lds_v4;
    typedef __attribute__((address_space(3))) float *lds_f1;
    auto ld4 = [](uint32_t a) { const v4f v = *(lds_v4)a; return make_float4(v.x, v.y, v.z, v.w); };
    const uint32_t sbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    const uint32_t lane16 = lane * 16, lane4 = lane * 4;
    // (no lane guards: reads up to 127 entries past a part's end stay inside the wave's LDS slice and the weight rows
    // are padded to whole rounds, so the surplus lanes of the last round write weights nobody reads)
    auto weight = [&](const float4 &ce, const float4 &tp, float pj) {
        return asw_support_weight(tp, ce, A.kC, pj);
    };
    // Two tap columns (j, j + 1) per build: a centre is read once for both, and the wave pays the LDS round trip of a
    // build once per two aggregation steps.  Weight row q = column parity, at wS + q * wrow.
    const int wrow = g.SLw + g.SRw;
    // KM (round 3): rounds of the MERGED build -- the strip's Txw left and nRcw right centres as one list of Txw + nRcw
    // entries dealt to the lanes 64 at a time, instead of ceil(Txw / 64) + ceil(nRcw / 64) rounds with two part-filled
    // last rounds (class default D 0..16, 4-column tile: 48 + 67 centres = 2 rounds instead of 1 + 2); 0: counted at run time.
    // The two parts read different pixel rows; pixR follows pixL in LDS, so the tap address of list entry c is
    // pixL + 16 (c + j) + (c < Txw ? 0 : 32 pad): one per-lane constant per round (tapoff), set up once per wave.
    // CREG (round 4; 4-column tile, KM > 0): the centres a lane evaluates are the SAME in every build of the kernel (list entries lane,
    // lane + 64, ...), so their Lab values are loaded once from the records into 3 KM registers (cenx/y/z above) instead of being
    // kept in an LDS array and re-read twice per tap-column pair: a third fewer LDS reads per weight, and the wave's LDS slice
    // loses 16 bytes per centre -- at D 0..7 / win 35 (124-column strips, 255 centres) that is 13.9 -> 9.9 KB, 11 -> 16 resident
    // waves per CU.
    uint32_t tapoff[KM > 0 ? KM : 1];
#pragma unroll
    for (int r = 0; r < (KM > 0 ? KM : 1); ++r) {
        const int c = 64 * r + lane;
        tapoff[r] = 16u * (uint32_t)c + (c < Txw ? 0u : 32u * (uint32_t)p);
    }
    auto build_merged = [&](uint32_t tap_b, uint32_t cen_b, uint32_t dst_b, float pj0, float pj1) {
        asm volatile("" : "+s"(tap_b), "+s"(cen_b), "+s"(dst_b));        // opaque: base + lane sums are formed here, per build
        const uint32_t row1 = (uint32_t)wrow * 4;
        if constexpr (CREG) {                            // centres in registers: two tap reads per weight pair, all in flight together
            const uint32_t da = dst_b + lane4, db_ = da + row1;
            float4 ta_[KM], tb[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                const uint32_t ta = tap_b + tapoff[r];
                ta_[r] = ld4(ta); tb[r] = ld4(ta + 16);
            }
#pragma unroll
            for (int r = 0; r < KM; ++r) asm volatile("" ::"v"(ta_[r].w), "v"(tb[r].w) : "memory");
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                const float4 ce = make_float4(cenx[r], ceny[r], cenz[r], 0.f);
                *(lds_f1)(da + 256 * r) = weight(ce, ta_[r], pj0);
                *(lds_f1)(db_ + 256 * r) = weight(ce, tb[r], pj1);
            }
            return;
        }
        if constexpr (KM > 0) {                          // centres in LDS, round by round: the 8-column tile (no registers for more)
            const uint32_t ca = cen_b + lane16, da = dst_b + lane4, db_ = da + row1;
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                const uint32_t ta = tap_b + tapoff[r];
                const float4 ce0 = ld4(ca + 1024 * r), ta0 = ld4(ta), tb0 = ld4(ta + 16);
                asm volatile("" ::"v"(ce0.w), "v"(ta0.w), "v"(tb0.w));   // keeps the reads ds_read_b128
                *(lds_f1)(da + 256 * r) = weight(ce0, ta0, pj0);
                *(lds_f1)(db_ + 256 * r) = weight(ce0, tb0, pj1);
            }
            return;
        }
        for (int k = 0; k < ncen; k += 64) {              // rounds counted at run time
            const int c = k + lane;
            const uint32_t ca = cen_b + lane16 + k * 16, ta = tap_b + lane16 + k * 16 + (c < Txw ? 0u : 32u * (uint32_t)p),
                           da = dst_b + lane4 + k * 4;
            const float4 ce0 = ld4(ca), ta0 = ld4(ta), tb0 = ld4(ta + 16);
            asm volatile("" ::"v"(ce0.w), "v"(ta0.w), "v"(tb0.w) : "memory");
            *(lds_f1)da = weight(ce0, ta0, pj0);
            *(lds_f1)(da + row1) = weight(ce0, tb0, pj1);
        }
    };
