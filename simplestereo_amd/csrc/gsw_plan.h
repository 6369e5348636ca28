// Launch planner of the GSW kernel: tile layout, cost model, autotuning candidates.  Pure arithmetic, like asw_plan.h (which it
// follows in host_context.h, a host section of ssamd_api.hip and the only file that includes it).
#pragma once

bool gsw_layout(GswGeom &g, int win, int XG, int DG, int Ty, size_t limit, int Hy = 1)
{
    const int p = win / 2;
    g.XG = XG; g.DG = DG; g.Ty = Ty; g.Rd = Ty == 2 ? 4 : 8; g.Hy = Hy;
    g.Tx = GSW_RX * XG; g.Dc = g.Rd * DG;
    g.threads = round_up(XG * DG, 64);
    g.nL = g.Tx + 2 * p;
    g.nT = g.nL + g.Dc - 1;
    int P = 1;
    while (8 * P < g.Dc) P <<= 1;
    g.Se = 8 * P;                                  // floats per e row (slots of 8 disparities)
    g.Ses = 3;
    while ((1 << g.Ses) < g.Se) ++g.Ses;
    g.emask = std::min(P, 32) - 1;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return (int)o; };
    g.off_w = take((size_t)Ty * Hy * win * g.Tx * 4);
    const int nL4 = round_up(g.nL, 4);                 // the e tasks cover 4 columns
    g.off_e = take((size_t)nL4 * g.Se * 4);
    g.off_ref = take((size_t)nL4 * 16 * 2);            // pixel staging is double-buffered (prefetch of the next image row)
    g.off_tgt = take((size_t)(g.nT + nL4 - g.nL) * 16 * 2);
    g.off_best = take((size_t)Ty * Hy * g.Tx * 8);
    g.off_cen = take((size_t)Ty * Hy * g.Tx * 4);
    g.lds_bytes = (int)off;
    return off <= limit && g.threads * Hy <= GSW_MAX_THREADS;
}

// Autotuning candidates (round 4).  The cost model above is calibrated on config 4 (193 disparities) and is up to 38 % off for
// small ranges -- the class default of StereoGSW is maxDisparity = 16 -- where narrow tiles with ONE wave per thread group and
// four-row strips win (1080p / win 11: D 0..16 2.09 -> 1.40 ms with "10,5,2,2", D 0..7 1.91 -> 1.18 ms with "16,2,2,2", D 0..32
// 2.55 -> 1.97 ms with "14,9,2,2"; profiles/r04_gsw_geometry_small_ranges.txt).  Candidates: the model's choice first, then for
// strips of 2 / 4 / 8 rows the tiles whose thread groups fill whole waves (XG x DG just below 64, 128, ... 512 lanes).
void gsw_candidates(std::vector<GswGeom> &out, const GswGeom &model, int W, int rows, int win, int nD)
{
    out.clear();
    out.push_back(model);
    const int Ty = 2, Rd = 4;
    if (rows < 2) return;
    for (int nch = model.nchunks; nch <= model.nchunks + 1 && nch <= nD; ++nch) {
        const int per = (nD + nch - 1) / nch, DG = round_up(per, Rd) / Rd;
        if (DG > 64 || (nD + DG * Rd - 1) / (DG * Rd) != nch) continue;
        for (int Hy : {1, 2, 4}) {
            if (Ty * Hy > std::max(rows, 2)) break;
            for (int T : {32, 64, 128, 192, 256, 384, 512}) {
                if (T * Hy > GSW_MAX_THREADS) break;
                for (int trim = 0; trim < 2; ++trim) {          // ... and a sixth narrower (smaller LDS slice: one more resident workgroup)
                    const int XG = std::min((T / DG) * (6 - trim) / 6, (W + GSW_RX - 1) / GSW_RX);
                    if (XG < 2) continue;
                    GswGeom g;
                    if (!gsw_layout(g, win, XG, DG, Ty, 160 * 1024, Hy)) continue;
                    g.nchunks = nch;
                    bool dup = false;
                    for (const GswGeom &o : out) dup = dup || (o.XG == g.XG && o.DG == g.DG && o.Ty == g.Ty && o.Hy == g.Hy && o.nchunks == g.nchunks);
                    if (!dup && out.size() < 36) out.push_back(g);
                }
            }
        }
    }
}

// Launch geometry of the GSW kernel: strip height Ty, XG x DG thread grid.  Relative cost model of one
// strip, per thread: every image row of the strip pays the e tile once (c_e per element), every
// (output row, window row) pair pays its weights (c_w per element) and its taps (c_tap per cell).
PlanResult gsw_search_geometry(GswGeom &best, const std::string &forced, int W, int rows, int win, int nD)
{
    if (!forced.empty()) {                             // experiment hook: "XG,DG,Ty"
        int XG = 0, DG = 0, Ty = 1, Hy = 1;                       // "XG,DG[,Ty[,Hy]]"
        if (sscanf(forced.c_str(), "%d,%d,%d,%d", &XG, &DG, &Ty, &Hy) >= 2 && XG >= 1 && DG >= 1 && (Ty == 1 || Ty == 2) && Hy >= 1 && Hy <= 8 &&
            XG * DG <= GSW_MAX_THREADS && gsw_layout(best, win, XG, DG, Ty, 160 * 1024, Hy)) {
            best.nchunks = (nD + best.Dc - 1) / best.Dc;
            return PLAN_OK;
        }
        return PLAN_FORCED_UNUSABLE;
    }
    const double c_tap = 5.3, c_w = 60.0, c_e = 70.0;
    double best_score = -1.0;
    bool found = false;
    for (int Ty = 1; Ty <= 2; ++Ty) {
        if (Ty > std::max(rows, 1)) break;
        const int Rd = Ty == 2 ? 4 : 8;
        for (int nch = 1; nch <= nD; ++nch) {
            const int per = (nD + nch - 1) / nch;
            const int DG = round_up(per, Rd) / Rd;
            if (DG > 64) continue;
            if ((nD + DG * Rd - 1) / (DG * Rd) != nch) continue;
            const int xg_cap = std::min(GSW_MAX_THREADS / DG, (W + GSW_RX - 1) / GSW_RX);
            // Hy thread groups share the e tile and the staged pixels of an image row (round 3): strips of Ty * Hy rows.
            // Built, bit-exact (SSAMD_GSW_GEOM="XG,DG,Ty,Hy", tests/test_gpu_gsw.py) and MEASURED at 1080p / D 0..192:
            // 10,25,2,2 (40-column tiles, four-row strips) 9.24 ms against 9.16 ms for 20,25,2,1 -- the third fewer e
            // elements are paid back by the narrower tile (profiles/r03_gsw_*.txt), so the search keeps Hy = 1.
            for (int Hy = 1; Hy <= 1; Hy *= 2)
            for (int XG = xg_cap; XG >= 1; --XG) {
                GswGeom g;
                if (!gsw_layout(g, win, XG, DG, Ty, 160 * 1024, Hy)) continue;
                g.nchunks = nch;
                const int tot = g.threads * Hy, TyS = Ty * Hy;
                const int waves = tot / 64, per_simd = (waves + 3) / 4;
                const int k = std::min({4 / per_simd, (160 * 1024) / g.lds_bytes, 8});   // <= 128 VGPRs: 4 waves per SIMD
                if (k < 1) continue;
                const double M = (double)win * GSW_RX * Rd * c_tap;                       // a thread aggregates its group's Ty rows only
                const double Bw = (double)((g.Tx * win + tot - 1) / tot) * c_w;           // weights and e tiles are built by all threads
                const double Be = (double)((g.nL * g.Dc + tot - 1) / tot) * c_e;
                const double strip = (double)(win + TyS - 1) * Be + (double)TyS * win * Bw + (double)Ty * win * M;
                const double eff = (double)Ty * win * M / strip;
                const double d_util = (double)nD / ((double)nch * g.Dc);
                const int xt = (W + g.Tx - 1) / g.Tx, yt = (std::max(rows, 1) + TyS - 1) / TyS;
                const double x_util = (double)W / ((double)xt * g.Tx);
                const double y_util = (double)std::max(rows, 1) / ((double)yt * TyS);
                const double nwg = (double)xt * yt * nch, slots = 256.0 * k;
                const double tail = nwg / (std::ceil(nwg / slots) * slots);
                const double score = (double)k * XG * DG * Hy * eff * d_util * x_util * y_util * tail;
                if (score > best_score) { best_score = score; best = g; found = true; }
            }
            if (DG <= 1) break;
        }
    }
    return found ? PLAN_OK : PLAN_NO_FIT;
}
