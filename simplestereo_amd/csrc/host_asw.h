// Host section of ssamd_api.hip: ASW -- tables, key buffers and their decode (GSW's too), kernel variants, AswCall / AswRun and the steps of a call.
namespace {
// Proximity weights exp(-|t|/gammaP) of the window taps, cached per (winSize, gammaP): the reference's expression (_passive.cpp:360-364:
// exp(-sqrt(pow(i-padding,2) + pow(j-padding,2))/gammaP)) rounded to float for the kernels, and as it is for the fp64 tie-break pass.
template <class T> int get_prox_table(TableCache &tc, const char *what, int win, double gammaP, hipStream_t s, const T **out)
{
    return get_table(tc, win, gammaP, (size_t)win * win, what, s, out, [&](T *host) {
        const int p = win / 2;
        for (int i = 0; i < win; ++i)
            for (int j = 0; j < win; ++j) {
                // exp: glibc's algorithm restated (glibc_math.hip.h), not the host's libm (round 6: rounds 1-5 called it here, which made the exact
                // mode's bit-identity a property of the host) -- bit-identical to glibc's on every argument oracle/libm_check.c tries, and the
                // same on a host that runs another libm.  pow(int, 2) is exact, sqrt and the division are IEEE operations
                const double di = i - p, dj = j - p;
                host[(size_t)i * win + j] = (T)glibc_exp(-std::sqrt(di * di + dj * dj) / gammaP);
            }
    });
}
int get_prox(Ctx &c, int win, double gammaP, hipStream_t s, const float **out) { return get_prox_table(c.proxTabs, "proximity table", win, gammaP, s, out); }
int get_prox64(Ctx &c, int win, double gammaP, hipStream_t s, const double **out) { return get_prox_table(c.proxTabs64, "fp64 proximity table", win, gammaP, s, out); }

// WTA keys of a call start as all ones: any (cost, disparity) key is smaller
int reset_keys(DevBuf &keys, size_t nout, hipStream_t s)
{
    if (int rc = keys.reserve(nout * 8)) return rc;
    HIP_TRY(hipMemsetAsync(keys.ptr, 0xFF, nout * 8, s));
    return SSAMD_OK;
}

// Decode / left-right check of rows [b0, b0 + nb) of a call's key buffers into the same rows of d_disp (row-local:
// _passive.cpp:251-285).  d_raw_right: verification dump, both raw argmins instead of the left-right check and filling.
int launch_finalize(Ctx &c, int slot, bool lrcheck, int b0, int nb, int W, int16_t *d_disp, hipStream_t s,
                    int16_t *d_raw_right = nullptr)
{
    if (nb <= 0) return SSAMD_OK;
    const size_t off = (size_t)b0 * W;
    const long long n = (long long)nb * W;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 256 * 8);
    Timed t(c, s, slot);
    if (d_raw_right) {
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyL.ptr + off, d_disp + off, nb, W, 0);
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyR.ptr + off, d_raw_right + off, nb, W, 1);
    } else if (lrcheck) {
        const size_t lds = (((size_t)W * 2 + 15) & ~(size_t)15) + W;      // up to 96 KiB at the 32767-column limit
        int rc = grant_dyn_lds(c, (const void *)lr_check_fill_kernel, (int)lds);
        if (rc) return rc;
        hipLaunchKernelGGL(lr_check_fill_kernel, dim3(nb), dim3(256), lds, s, (const u64 *)c.keyL.ptr + off,
                           (const u64 *)c.keyR.ptr + off, d_disp + off, nb, W);
    } else {
        hipLaunchKernelGGL(wta_decode_kernel, dim3(blocks), dim3(256), 0, s, (const u64 *)c.keyL.ptr + off, d_disp + off, nb, W, 0);
    }
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// ------------------------------------------------------------ ASW: kernel variants, picked from tables generated from asw_instances.inc
// (the list of what the other two translation units compile): what is selected here and what is compiled there cannot disagree
using AswKernel = void (*)(const AswArgs);
using AswWaveKernel = void (*)(const AswWaveArgs);
struct AswPipeVariant { bool costs; int SL, SR, Se; AswKernel kernel; };
const AswPipeVariant kPipeVariants[] = {
#define SSAMD_PIPE_INSTANCE(C, SL, SR, SE) {C, SL, SR, SE, asw_aggregate_pipe_kernel<C, SL, SR, SE>},
#include "asw_instances.inc"
#undef SSAMD_PIPE_INSTANCE
};
// Wave kernels: RD disparities per lane (6: asw_instances.inc; 4: instantiated here), RX columns, and the build rounds known at
// compile time (straight-line build) for the common combinations; KM > 0: merged build of KM rounds, else KL + KR separate rounds
// (a straight-line merged build of the 4-column tile keeps the window centres in registers, AswWaveGeom::creg: the kernels derive that)
// Row comments: the disparity counts nD at which the default plan of a plain call selects the row, and those at which only one
// of the autotuner's other candidates does (the other tile, never six per lane); enumerated from asw_plan.h over nD 1..64,
// profiles/wave_variants_retired.txt.  The six-per-lane rows (asw_instances.inc): KM 3 default 17..18, tuner 21..24; KM 2 tuner
// only, 29..30 and 33..60.  Every other strip -- SSAMD_ASW_WAVE_MERGE=0 with the 4-column tile among them -- runs the generic kernel.
struct AswWaveVariant { int RD; bool costs; int RX, KL, KR, KM; AswWaveKernel kernel; };
#define SSAMD_WAVE_VARIANT(RX, KL, KR, KM) {4, false, RX, KL, KR, KM, asw_aggregate_wave_kernel<false, RX, KL, KR, KM>}
const AswWaveVariant kWaveVariants[] = {
#define SSAMD_WAVE6_INSTANCE(C, K) {6, C, 4, 0, 0, K, asw_aggregate_wave6_kernel<C, K>},
#include "asw_instances.inc"
#undef SSAMD_WAVE6_INSTANCE
    SSAMD_WAVE_VARIANT(4, 0, 0, 2),      // default 13..16, 19..20 (class default D 0..16 four per lane: 48 + 67 centres); tuner 17..18, 61..64
    SSAMD_WAVE_VARIANT(4, 0, 0, 3),      // default 9..12
    SSAMD_WAVE_VARIANT(4, 0, 0, 4),      // default 5..8
    SSAMD_WAVE_VARIANT(8, 0, 0, 2),      // default 41..64
    SSAMD_WAVE_VARIANT(8, 0, 0, 3),      // default 21..28
    SSAMD_WAVE_VARIANT(8, 0, 0, 4),      // tuner only, 13..16
    SSAMD_WAVE_VARIANT(8, 2, 2, 0),      // tuner only, 17..20 (SSAMD_ASW_WAVE_MERGE=0: 17..28)
    SSAMD_WAVE_VARIANT(8, 1, 2, 0),      // default 29..40 (SSAMD_ASW_WAVE_MERGE=0: 29..64)
};
#undef SSAMD_WAVE_VARIANT

// Strides known at compile time for the tiles of the headline configurations (immediate offsets in the
// tap steps): 120 x 196 (1080p / D 0..192) and 88 x 260 (4096 x 2160 / D 0..256), 216 x 68 (D 0..64)
// (with the cost / cost-image dump too: exact=True on the headline tiles ran the run-time-stride form, + 0.9 ms at 1080p / 193)
AswKernel asw_pick_pipe_kernel(const AswGeom &g, bool costs, int asw_static)
{
    AswKernel pk = nullptr;
    for (const AswPipeVariant &v : kPipeVariants) {
        if (v.costs != costs) continue;
        if (v.SL == 0 && !pk) pk = v.kernel;                                  // (the generic instantiation, unless a static one matched)
        if (asw_static != 0 && v.SL == g.SL && v.SR == g.SR && v.Se == g.Se) pk = v.kernel;
    }
    return pk;
}

// A miss runs the generic instantiation of the family (no straight-line build, centres in LDS) -- also a variant whose centres are
// not where the strip's LDS layout (g.creg) has them.
AswWaveKernel asw_pick_wave_kernel(const AswWaveGeom &g, bool costs, bool unrolled)
{
    const bool straight = unrolled && !costs;
    const int kl = g.merged ? 0 : (g.Txw + 63) / 64, kr = g.merged ? 0 : (g.nRcw + 63) / 64, km = g.merged ? g.K : 0;
    for (const AswWaveVariant &v : kWaveVariants)
        if (straight && v.RD == g.RD && !v.costs && v.RX == g.RX && v.KL == kl && v.KR == kr && v.KM == km &&
            (v.RX == 4 && v.KM > 0) == (g.creg != 0)) return v.kernel;
    if (g.RD == 6) return costs ? asw_aggregate_wave6_kernel<true, 0> : asw_aggregate_wave6_kernel<false, 0>;
    return g.RX == 8 ? (costs ? asw_aggregate_wave_kernel<true, 8> : asw_aggregate_wave_kernel<false, 8>)
                     : (costs ? asw_aggregate_wave_kernel<true, 4> : asw_aggregate_wave_kernel<false, 4>);
}

// ------------------------------------------------------------ ASW: one call
// What an entry point asks for.  Images: dL / dR (rectified BGR bytes on the device), or rm: the RAW frames through the rig's maps
// (remap_lab_records_pair_kernel: rectification + Lab in one launch).
// skip > 0: rows [row0 + skip_at, row0 + skip_at + skip) of the range are NOT matched (ssamd_asw_device_rows2: the two border
// bands of a row strip in one launch); buffers stay laid out for the whole range [row0, row0 + rows)
struct MatchCall {                // (what AswCall and GswCall, host_gsw.h, share: the part host_rows rebases to a row strip)
    const uint8_t *dL = nullptr, *dR = nullptr;
    const RemapSrc *rm = nullptr;
    int H = 0, W = 0, row0 = 0, rows = 0;
    int win = 0, maxD = 0, minD = 0;
    int16_t *d_disp = nullptr;
    hipStream_t s = nullptr;
};
struct AswCall : MatchCall {
    int skip_at = 0, skip = 0;
    double gammaC = 0, gammaP = 0;
    bool consistent = false, alternate = false, exact = false;
    float *d_costs = nullptr;
    int16_t *d_raw_right = nullptr;
};

// The call the C parameters every ASW entry point shares describe, in its mode; the rest (rm, skip, the dumps) by field name.
AswCall asw_call(const uint8_t *dL, const uint8_t *dR, int H, int W, int row0, int rows, int win, int maxD, int minD, double gammaC,
                 double gammaP, int consistent, int16_t *d_disp, void *stream, bool alternate = false, bool exact = false)
{
    AswCall q;
    q.dL = dL; q.dR = dR; q.H = H; q.W = W; q.row0 = row0; q.rows = rows;
    q.win = win; q.maxD = maxD; q.minD = minD; q.gammaC = gammaC; q.gammaP = gammaP; q.consistent = consistent != 0;
    q.d_disp = d_disp; q.s = (hipStream_t)stream; q.alternate = alternate; q.exact = exact;
    return q;
}

struct AswRun : AswCall {
    Ctx &c;
    const Tuning &t;                  // (state of a call in flight: the call, the thread's option snapshot, what the steps hand on)
    PlanOptions po;
    int p, nD, grows, r0, r1, lab_blocks;
    size_t nout;
    long long np2;
    ShapeKey shape;           // W, workgroup rows, winSize, nD
    AswGeom geom;                     // the geometry of the (last) launch
    std::vector<AswGeom> trial;       // autotuning candidates, the model's choice first; empty: no trial launches
    bool need_keys = false, lab_pending = false;
    size_t evol_cap_max = 0, evol_limit = 0;      // (evol_limit 0: free memory not asked for yet)
    const float *d_prox = nullptr;
    const unsigned char *evol = nullptr;      // TAD volume of the geometry prepared last (nullptr: none)
    int evolW = 0;
    AswWaveGeom wave;                 // strip of the wave kernel, filled by asw_prepare_volume
    AswExactQueue xq_final{}, xq_raw{}, xq_kernel{};      // exact mode: the final near-tie queue, for merging calls the raw one, and the one the kernels append to
};
// exact mode, before and after the aggregation (host_asw_exact.h, the section behind this one: it works on the AswRun)
int asw_exact_prepare(AswRun &r, bool direct);
int asw_exact_pass(AswRun &r, bool direct);

// One disparity chunk and no right-referenced pass: each pixel is decided by exactly one workgroup, which then
// writes the disparity itself -- no key buffer, atomics or decode kernel (34 instead of 48+ bytes of HBM per pixel).
bool asw_is_direct(const AswRun &r, const AswGeom &g) { return r.nD >= 1 && (g.nchunks == 1 || g.wave_rx) && !r.consistent; }

// 1: nothing to compute
int asw_check_call(const AswCall &q)
{
    int rc = check_common(q.H, q.W, q.win, q.minD, q.maxD, q.row0, q.rows);
    if (rc) return rc;
    if (q.skip < 0 || q.skip_at < 0 || q.skip_at + q.skip > q.rows) return fail(SSAMD_EINVAL, "bad row gap [%d,%d) in a range of %d rows", q.skip_at, q.skip_at + q.skip, q.rows);
    if (q.skip > 0 && (q.alternate || q.d_costs || q.d_raw_right)) return fail(SSAMD_EINVAL, "two row ranges: plain, consistent and exact matching only");
    if (q.skip == q.rows) return 1;
    if (!(q.gammaC > 0) || !(q.gammaP > 0)) return fail(SSAMD_EINVAL, "gammaC and gammaP must be positive");
    if (q.exact && (q.alternate || q.d_costs)) return fail(SSAMD_EINVAL, "the exact (fp64 tie-break) mode has no alternate-rows form and no cost dump");
    // alternate-rows mode: row0 is matched exactly, then every second row; the range must end with an exact row or with
    // the image (asw_alternate_rows arranges that for strips)
    if (q.alternate && q.d_costs) return fail(SSAMD_EINVAL, "the alternate-rows mode has no cost dump");
    return q.rows == 0 ? 1 : SSAMD_OK;
}

// The TAD volume is scratch of THIS library next to the caller's own allocations (torch's caching allocator on the
// same GPU): never more than 24 GiB and never more than half of what is free right now (plus what the buffer already
// holds).  The phase-shifted kernel builds its e tiles itself when there is no volume; the wave kernel cannot, so
// a range it would serve falls back to the workgroup geometry stored next to it.
// Free memory is only asked for (a driver query, tens of microseconds next to a 0.1 ms Tsukuba call) when a volume
// would have to GROW: what fits the buffer the context already holds fits.
bool asw_volume_fits(AswRun &r, size_t bytes)
{
    if (bytes > r.evol_cap_max) return false;
    if (bytes <= r.c.evol.cap) return true;
    if (!r.evol_limit) {
        size_t free_b = 0, total_b = 0;
        r.evol_limit = r.evol_cap_max;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) r.evol_limit = std::min(r.evol_cap_max, r.c.evol.cap + free_b / 2);
        else (void)hipGetLastError();
    }
    return bytes <= r.evol_limit;
}

bool asw_wave_volume_fits(AswRun &r, const AswGeom &g)
{
    AswWaveGeom wg;
    if (!g.wave_rx || !asw_wave_layout(wg, r.po, r.win, r.nD, g.wave_rx)) return !g.wave_rx;
    const int xt = (r.W + wg.Txw - 1) / wg.Txw, erows = std::min(r.H, r.row0 + r.rows + r.win / 2) - std::max(0, r.row0 - r.win / 2);
    return asw_volume_fits(r, (size_t)erows * (size_t)round_up(xt * wg.Txw + 2 * (r.win / 2), 4) * (size_t)wg.Se + 4096);
}

// Planning: the geometry (cached per shape), the autotuner's trial list, and what of both survives without room for a volume.
int asw_plan_call(AswRun &r)
{
    if (r.nD >= 1)
        if (int rc = asw_choose_geometry(r.geom, r.po, r.W, r.grows, r.win, r.nD)) return rc;
    // Autotuning (ssamd_autotune): the first call for a problem shape times the best geometry of every class of
    // candidates on the real buffers and keeps the fastest.  Every geometry accumulates the same taps in the same
    // order, so the result does not depend on the choice (and the trial launches are idempotent).
    const double call_taps = (double)r.W * r.grows * r.nD * r.win * r.win;
    if (autotune_due(g_asw_geom, r.shape, call_taps) && r.nD >= 1 && !asw_geometry_forced(r.t)) {
        AswGeom tmp;
        if (asw_search(tmp, r.po, r.W, r.grows, r.win, r.nD, &r.trial) != SSAMD_OK || r.trial.size() < 2) r.trial.clear();
    }
    r.evol_cap_max = r.t.evol_max_mb ? std::min((size_t)24 << 30, (size_t)r.t.evol_max_mb << 20) : (size_t)24 << 30;
    if (r.nD >= 1 && r.geom.wave_rx && !asw_wave_volume_fits(r, r.geom)) ++r.c.evol_fallbacks;
    if (r.nD >= 1 && !asw_wave_volume_fits(r, r.geom)) r.geom.wave_rx = 0;
    r.trial.erase(std::remove_if(r.trial.begin(), r.trial.end(), [&](const AswGeom &g) { return !asw_wave_volume_fits(r, g); }), r.trial.end());
    if (r.trial.size() < 2) r.trial.clear();
    r.need_keys = !asw_is_direct(r, r.geom) || r.alternate;  // the alternate mode merges its odd-row jobs through the left keys
    for (const AswGeom &g : r.trial) r.need_keys = r.need_keys || !asw_is_direct(r, g);
    return SSAMD_OK;
}

// Lab records of both images, one launch
int asw_lab_records(AswRun &r)
{
    Ctx &c = r.c;
    Timed t(c, r.s, SSAMD_K_LAB);
    if (r.rm)
        hipLaunchKernelGGL(remap_lab_records_pair_kernel, dim3(r.lab_blocks), dim3(256), 0, r.s, *r.rm, (PixRec *)c.recL.ptr, (PixRec *)c.recR.ptr,
                           (long long)r.r0 * r.W, r.np2);
    else
        hipLaunchKernelGGL(bgr2lab_records_pair_kernel, dim3(r.lab_blocks), dim3(256), 0, r.s, r.dL + (size_t)r.r0 * r.W * 3, r.dR + (size_t)r.r0 * r.W * 3,
                           (PixRec *)c.recL.ptr + (size_t)r.r0 * r.W, (PixRec *)c.recR.ptr + (size_t)r.r0 * r.W, r.np2);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// pre-computed truncated-absolute-difference volume for the phase-shifted and wave kernels (asw_tad_volume_kernel), or -- when the
// Lab records are still pending -- records and volume in one launch (asw_prepass_kernel);
// SSAMD_ASW_EVOL=0 keeps the in-kernel e tiles (experiments / tests)
int asw_prepare_volume(AswRun &r, const AswGeom &g)
{
    Ctx &c = r.c;
    hipStream_t s = r.s;
    r.evol = nullptr;
    int chunks = g.nchunks, Tx = g.Tx, Dc = g.Dc, Se = g.Se;
    if (g.wave_rx) {
        if (!asw_wave_layout(r.wave, r.po, r.win, r.nD, g.wave_rx, !r.d_costs && r.t.wave_unroll != 0))
            return fail(SSAMD_ELIMIT, "wave kernel geometry does not fit LDS");
        chunks = 1; Tx = r.wave.Txw; Dc = r.wave.Dc; Se = r.wave.Se;
    } else if (!g.pipe || r.t.asw_evol == 0) {
        return SSAMD_OK;
    }
    const int xt = (r.W + Tx - 1) / Tx, erows = r.r1 - r.r0;
    // rows stay 16-byte aligned for any Se; the phase-shifted kernel's half-width tail tiles (see asw_launch_pipe) may reach
    // up to half a tile + 4 columns further than the last full tile
    const int evolW = round_up(xt * Tx + 2 * r.p + (g.wave_rx ? 0 : Tx / 2 + 8), 4);
    const size_t bytes = (size_t)chunks * (size_t)erows * (size_t)evolW * (size_t)Se;
    // A buffer four times larger than the calls need is given back -- but only after eight such calls in a row
    // and never between the trial launches of the autotuner: a workload alternating a large and a small shape
    // (or the tuner's round-robin over wave and workgroup candidates) must not pay a device synchronisation,
    // a hipFree and a hipMalloc per switch.
    if (c.evol.cap > ((size_t)256 << 20) && (bytes + 4096) * 4 < c.evol.cap) {
        if (r.trial.empty() && ++c.evol_small_calls >= 8) {
            (void)hipStreamSynchronize(s);                    // (earlier launches of this call may still read it)
            c.evol.release();
            c.evol_small_calls = 0;
        }
    } else {
        c.evol_small_calls = 0;
    }
    int erc = SSAMD_ENOMEM;
    if (r.t.evol_fail) {                                      // test hook: a hipMalloc that really fails
        void *none = nullptr;
        size_t free_b = 0, total_b = (size_t)512 << 30;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (hipMalloc(&none, 2 * total_b) == hipSuccess) (void)hipFree(none);     // twice the device's memory
        // (deliberately NOT drained here: the fallback below has to cope with the sticky error itself)
    } else if (asw_volume_fits(r, bytes + 4096)) {
        erc = c.evol.reserve(bytes + 4096);                   // + one DMA piece of slack behind the last tile
    }
    if (erc) {
        (void)hipGetLastError();      // a failed hipMalloc stays the thread's last HIP error on ROCm 7: drop it before the launches' checks
        // the phase-shifted kernel builds its e tiles itself when there is no volume (evol == nullptr);
        // only the wave kernel cannot run without one
        if (g.wave_rx) return fail(erc == SSAMD_ENOMEM ? SSAMD_ENOMEM : erc, "TAD volume of %zu bytes does not fit the device memory left", bytes);
        ++c.evol_fallbacks;
        g_err.clear();
        return SSAMD_OK;
    }
    r.evol = (const unsigned char *)c.evol.ptr;
    r.evolW = evolW;
    const int rd = g.wave_rx ? r.wave.RD : 4;
    Timed t(c, s, SSAMD_K_LAB);
    const dim3 egrid((unsigned)((evolW + TADV_COLS - 1) / TADV_COLS), (unsigned)erows, (unsigned)chunks);
    const size_t elds = (size_t)(2 * TADV_COLS + Dc) * 4;
    const long long tiles = (long long)egrid.x * egrid.y * egrid.z;
    if (r.lab_pending && tiles + r.lab_blocks < (1ll << 31)) {
        AswPrepassArgs pa;
        pa.bgrL = r.dL; pa.bgrR = r.dR; pa.recL = (PixRec *)c.recL.ptr; pa.recR = (PixRec *)c.recR.ptr;
        pa.evol = (unsigned char *)c.evol.ptr; pa.npix_total = (long long)r.H * r.W;
        pa.W = r.W; pa.pad = r.p; pa.minD = r.minD; pa.Dc = Dc; pa.Se = Se; pa.erow0 = r.r0; pa.erows = erows; pa.evolW = evolW;
        pa.rd = rd;
        pa.lab_blocks = r.lab_blocks; pa.ex = (int)egrid.x; pa.ey = (int)egrid.y;
        if (int grc = grant_dyn_lds(c, (const void *)asw_prepass_kernel, (int)elds)) return grc;
        hipLaunchKernelGGL(asw_prepass_kernel, dim3((unsigned)(tiles + r.lab_blocks)), dim3(256), elds, s, pa);
        HIP_TRY(hipGetLastError());
        r.lab_pending = false;
        return SSAMD_OK;
    }
    if (r.lab_pending) {                   // (cannot share a launch: records first, as in rounds 2-4)
        r.lab_pending = false;
        if (int lrc = asw_lab_records(r)) return lrc;
    }
    if (int grc = grant_dyn_lds(c, (const void *)asw_tad_volume_kernel, (int)elds)) return grc;
    hipLaunchKernelGGL(asw_tad_volume_kernel, egrid, dim3(256), elds, s, (const PixRec *)c.recL.ptr, (const PixRec *)c.recR.ptr,
                       (unsigned char *)c.evol.ptr, r.W, r.p, r.minD, Dc, Se, r.r0, erows, evolW, rd);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// Every member AswArgs and AswWaveArgs share (all but the geometry), for a launch of geometry g.
template <class Args> void asw_fill_args(Args &x, const AswRun &r, const AswGeom &g)
{
    const bool direct = asw_is_direct(r, g);
    x.recL = (const PixRec *)r.c.recL.ptr; x.recR = (const PixRec *)r.c.recR.ptr;
    x.prox = r.d_prox;
    x.keyL = direct ? nullptr : (u64 *)r.c.keyL.ptr;
    x.keyR = r.consistent ? (u64 *)r.c.keyR.ptr : nullptr;
    x.disp = direct ? r.d_disp : nullptr;
    x.costs = r.d_costs;
    x.cost_keys = r.t.asw_cost_keys != 0;                             // (test hook: the dump holds the cost images)
    x.xq = r.xq_kernel;                                               // (the autotuner's trial launches run without the queue)
    x.evol = r.evol; x.erow0 = r.r0; x.erows = r.r1 - r.r0; x.evolW = r.evolW;
    x.H = r.H; x.W = r.W; x.win = r.win; x.pad = r.p; x.minD = r.minD; x.maxD = r.maxD; x.row0 = r.row0; x.rows = r.rows;
    x.kC = (float)(-1.4426950408889634 / r.gammaC);
    x.ystep = r.alternate ? 2 : 1;
    x.yb0 = 0;
    x.yskip_at = r.skip > 0 ? r.skip_at : 0x7fffffff; x.yskip = r.skip;
}

int asw_launch_pipe(AswRun &r, const AswArgs &a, const dim3 &grid)
{
    Ctx &c = r.c;
    const AswGeom &g = a.g;
    const AswKernel pk = asw_pick_pipe_kernel(g, r.d_costs != nullptr, r.t.asw_static);
    const int pipe_lds = a.evol ? g.lds_bytes_evol : g.lds_bytes;          // (no staged colour bytes when the e tiles come from the volume)
    if (pipe_lds > 160 * 1024) return fail(SSAMD_ELIMIT, "this tile needs the TAD volume (LDS %d bytes without it)", pipe_lds);
    if (int grc = grant_dyn_lds(c, (const void *)pk, pipe_lds)) return grc;
    // The last PARTIAL round of workgroups (round 4).  The kernel keeps one 12-wave workgroup per CU, so a launch
    // of n workgroups takes ceil(n / 256) rounds: a row strip of an 8-GPU run (135 rows x 16 tiles = 8.44 rounds)
    // pays nine.  When the last round is at most half full, the rows that fill whole rounds keep the tile and the
    // remaining rows are launched with tiles of half the columns (twice the workgroups, half the taps each: the
    // round ends after about half its time).  Same taps in the same order per (x, d): maps cannot change
    // (tests/test_gpu_asw.py).  Worth ~4 % at 8.44 rounds, nothing beyond a few dozen; SSAMD_ASW_TAIL=0 / 1 forces.
    int rows_main = r.grows;
    AswGeom tail_g;
    // workgroups in flight at a time: the device's CUs x the tile's residency (168 VGPRs -> three waves per SIMD;
    // the tile's LDS).  One per CU for the 9- to 12-wave tiles of the headline configurations.
    const int per_simd = (g.threads / 64 + 3) / 4;
    const long long resident = std::max(1, std::min(3 / std::max(1, per_simd), (160 * 1024) / std::max(1, pipe_lds)));
    const long long per_row = (long long)grid.x * g.nchunks, slots = (long long)c.cus * resident;
    if (!r.alternate && r.t.asw_tail != 0 && g.XG >= 4) {
        const long long n = per_row * r.grows;
        const long long full = n / slots, rem = n - full * slots;
        if (full >= 1 && rem > 0 && 2 * rem <= slots && (full < 32 || r.t.asw_tail > 0)) {
            const int rm = (int)(full * slots / per_row);
            if (rm >= 1 && rm < r.grows &&
                asw_layout_e(tail_g, r.po, r.win, (g.XG + 1) / 2, g.DG, 160 * 1024, g.JC, 8, true, false, true) && tail_g.pipe &&
                tail_g.Se == g.Se && tail_g.Dc == g.Dc &&
                (a.evol == nullptr || round_up(((r.W + tail_g.Tx - 1) / tail_g.Tx) * tail_g.Tx + 2 * r.p, 4) <= a.evolW)) {
                tail_g.nchunks = g.nchunks;
                rows_main = rm;
            }
        }
    }
    // The persistent form (round 8, asw_pipe_kernel.hip.h): as many workgroups as are resident at a time, each drawing the launch's
    // tiles as items from eight queues.  What it recovers is the XCD whose tiles include the light left-border ones running dry
    // about 12 % of the launch early (the dispatcher deals blocks to XCDs by id % 8 whatever their load: profiles/r08_xcd_dispatch.txt)
    // and the round quantisation; what it costs is fixed (the memset, one exposed ticket).  Measured on the 120 x 196 tile
    // (profiles/r08_pipe_persistent.txt): + 0.6 % at 8 full rounds, + 0.3 % at 16, nothing either way at 33.75, - 0.8 ... - 1.2 % at 67.5
    // (1080p), - 1.5 % at 4096 x 2160.  The host picks it from 64 full rounds on: where it is measured to gain.  Between 34 and 64
    // rounds nothing is measured and the launch stays the plain grid.  SSAMD_ASW_PERSIST=0 / n forces the plain grid /
    // min(n, slots) workgroups.  Same tiles, same instructions.
    const long long items = per_row * rows_main;
    long long workers = r.t.asw_persist > 0 ? std::min<long long>(r.t.asw_persist, slots) : (r.t.asw_persist < 0 && items >= 64 * slots ? slots : 0);
    workers = std::min(workers, items);
    if (workers > 0 && items < (1ll << 30)) {
        const size_t pq_bytes = (size_t)(ASW_PQ_QUEUES + 1) * ASW_PQ_LINE * 4;
        if (!c.pq.ptr) {
            if (int prc = c.pq.reserve(pq_bytes)) return prc;
            HIP_TRY(hipMemsetAsync(c.pq.ptr, 0, pq_bytes, r.s));       // (the counter of finished items behind the queues' is never zeroed again)
        }
        HIP_TRY(hipMemsetAsync(c.pq.ptr, 0, (size_t)ASW_PQ_QUEUES * ASW_PQ_LINE * 4, r.s));
        AswArgs pa = a;
        pa.pq = (unsigned int *)c.pq.ptr;
        pa.pq_nx = (int)grid.x; pa.pq_ny = rows_main; pa.pq_items = (int)items;
        ++c.persist_launches;
        hipLaunchKernelGGL(pk, dim3((unsigned)workers), dim3(g.threads), pipe_lds, r.s, pa);
    } else {
        hipLaunchKernelGGL(pk, dim3(grid.x, rows_main, grid.z), dim3(g.threads), pipe_lds, r.s, a);
    }
    HIP_TRY(hipGetLastError());
    if (rows_main < r.grows) {
        ++c.tail_splits;
        AswArgs t = a;
        t.g = tail_g;
        t.yb0 = rows_main;              // (workgroup rows continue; outputs are addressed by image row, so the buffers stay put)
        const AswKernel tk = asw_pick_pipe_kernel(tail_g, r.d_costs != nullptr, 0);
        const int tail_lds = a.evol ? tail_g.lds_bytes_evol : tail_g.lds_bytes;
        if (int grc = grant_dyn_lds(c, (const void *)tk, tail_lds)) return grc;
        hipLaunchKernelGGL(tk, dim3((r.W + tail_g.Tx - 1) / tail_g.Tx, r.grows - rows_main, tail_g.nchunks), dim3(tail_g.threads),
                           tail_lds, r.s, t);
        HIP_TRY(hipGetLastError());
    }
    return SSAMD_OK;
}

// The aggregation launch of geometry g (after asw_prepare_volume(r, g)); r.geom = g afterwards.
int asw_launch(AswRun &r, const AswGeom &g)
{
    r.geom = g;
    if (g.wave_rx) {                  // (asw_prepare_volume(r, g) filled r.wave and built the volume)
        AswWaveArgs wa;
        asw_fill_args(wa, r, g);
        wa.g = r.wave;
        const AswWaveKernel wk = asw_pick_wave_kernel(wa.g, r.d_costs != nullptr, r.t.wave_unroll != 0);
        const int lds = wa.g.wave_lds * wa.g.waves, xt = (r.W + wa.g.Txw - 1) / wa.g.Txw;
        if (int grc = grant_dyn_lds(r.c, (const void *)wk, lds)) return grc;
        hipLaunchKernelGGL(wk, dim3((xt + wa.g.waves - 1) / wa.g.waves, r.grows, 1), dim3(64 * wa.g.waves), lds, r.s, wa);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    }
    AswArgs a{};
    asw_fill_args(a, r, g);
    a.g = g;
    const dim3 grid((r.W + g.Tx - 1) / g.Tx, r.grows, g.nchunks);
    if (g.pipe) return asw_launch_pipe(r, a, grid);
    const bool chunked = g.JC < r.win;
    AswKernel kern = chunked ? (r.d_costs ? asw_aggregate_kernel<true, true> : asw_aggregate_kernel<false, true>)
                             : (r.d_costs ? asw_aggregate_kernel<true, false> : asw_aggregate_kernel<false, false>);
    if (g.Rx == 4)
        kern = chunked ? (r.d_costs ? asw_aggregate_kernel<true, true, 4> : asw_aggregate_kernel<false, true, 4>)
                       : (r.d_costs ? asw_aggregate_kernel<true, false, 4> : asw_aggregate_kernel<false, false, 4>);
    if (int grc = grant_dyn_lds(r.c, (const void *)kern, g.lds_bytes)) return grc;
    hipLaunchKernelGGL(kern, grid, dim3(g.threads), g.lds_bytes, r.s, a);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// The autotuner's trial launches: times r.trial on the call's own buffers, caches the fastest for the shape, leaves it in r.geom.
int asw_autotune(AswRun &r)
{
    hipStream_t s = r.s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    bool all_prepared = true;     // a candidate whose volume cannot be had right now is never launched, and the verdict of such a round is not cached
    // (a phase-shifted tile whose volume cannot be had is timed with in-kernel e tiles, or fails its launch when it was
    //  planned on the volume's LDS saving: that round says nothing about the tile, so its verdict is not kept either)
    const bool want_evol = r.t.asw_evol != 0;
    for (const AswGeom &g : r.trial) {                                             // code load, clocks, scratch
        if (asw_prepare_volume(r, g) != SSAMD_OK) { all_prepared = false; continue; }
        if (g.pipe && !g.wave_rx && want_evol && !r.evol) all_prepared = false;
        if (asw_launch(r, g) != SSAMD_OK) all_prepared = false;
    }
    const int fastest = autotune_rounds(r.trial.size(), 4, false, e0, e1, s, &all_prepared, [&](size_t ci) {
        const AswGeom &g = r.trial[ci];
        const bool launched = asw_prepare_volume(r, g) == SSAMD_OK && asw_launch(r, g) == SSAMD_OK;
        if (g.pipe && !g.wave_rx && want_evol && !r.evol) all_prepared = false;
        return launched;
    });
    if (fastest >= 0) r.geom = r.trial[fastest];      // (none timed: the geometry launched last)
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (all_prepared) autotune_keep(g_asw_geom, r.shape, r.geom);
    else g_err.clear();
    return SSAMD_OK;
}

// The final geometry's volume, with the two ways out when it cannot be had.  final_geom may change; r.need_keys follows.
int asw_final_volume(AswRun &r, AswGeom &final_geom)
{
    int rc = asw_prepare_volume(r, final_geom);
    if (rc == SSAMD_ENOMEM && final_geom.wave_rx) {
        // the volume's hipMalloc failed although the pre-check said it fits (fragmentation, another allocator on the
        // same GPU): the wave kernel cannot run without it, the workgroup geometry stored next to it can (in-kernel
        // e tiles, or a smaller volume if that one can be had)
        ++r.c.evol_fallbacks;
        g_err.clear();
        final_geom.wave_rx = 0;
        r.geom = final_geom;
        if (!asw_is_direct(r, final_geom) && !r.need_keys) {
            if ((rc = reset_keys(r.c.keyL, r.nout, r.s))) return rc;
            r.need_keys = true;
        }
        rc = asw_prepare_volume(r, final_geom);
    }
    if (rc) return rc;
    if (final_geom.pipe && !final_geom.wave_rx && !r.evol && final_geom.lds_bytes > 160 * 1024) {
        // the tile was planned on the TAD volume (no staged colour bytes in LDS) and the volume cannot be had: plan
        // again for the in-kernel e tiles (PlanOptions::no_volume)
        AswGeom g2;
        if ((rc = asw_search(g2, PlanOptions{r.t, true}, r.W, r.grows, r.win, r.nD))) return rc;
        g2.wave_rx = 0;
        if (!asw_is_direct(r, g2) && !r.need_keys && (rc = reset_keys(r.c.keyL, r.nout, r.s))) return rc;
        final_geom = g2;
        if ((rc = asw_prepare_volume(r, final_geom))) return rc;
    }
    return SSAMD_OK;
}

// odd rows of the alternate-rows mode: candidates bounded by the exact rows above and below (asw_alt_kernels.hip.h).  With an
// empty disparity range the decode already wrote x everywhere and the fill reproduces it.
int asw_alternate_fill(AswRun &r)
{
    Ctx &c = r.c;
    hipStream_t s = r.s;
    int rc;
    AswAltArgs f;
    const size_t nodd = (size_t)(r.rows / 2) * r.W;
    if ((double)nodd * ((r.nD + 7) / 8 + 1) >= 4.0e9)
        return fail(SSAMD_ELIMIT, "alternate-rows mode: image x disparity range too large for the 32-bit job counter");
    f.cap = (unsigned int)std::min<size_t>(std::max<size_t>(nodd, 1 << 16), 1u << 28);   // jobs of 8 candidates
    if (r.t.alt_queue_cap)                                      // test hook: a tiny queue forces the in-place path
        f.cap = (unsigned int)r.t.alt_queue_cap;
    if ((rc = c.altq.reserve((size_t)f.cap * 8 + 16))) return rc;
    f.ctr = (unsigned int *)c.altq.ptr; f.queue = (u64 *)((char *)c.altq.ptr + 16);
    HIP_TRY(hipMemsetAsync(f.ctr, 0, 16, s));
    f.recL = (const PixRec *)c.recL.ptr; f.recR = (const PixRec *)c.recR.ptr; f.prox = r.d_prox;
    f.disp = r.d_disp; f.key = (u64 *)c.keyL.ptr;
    f.H = r.H; f.W = r.W; f.win = r.win; f.pad = r.p; f.minD = r.minD; f.maxD = r.maxD; f.row0 = r.row0; f.rows = r.rows;
    f.kC = (float)(-1.4426950408889634 / r.gammaC);
    const dim3 pix_grid((r.W + 255) / 256, r.rows / 2);
    Timed t(c, s, SSAMD_K_ASW_ALT);
    hipLaunchKernelGGL(asw_alt_scan_kernel, pix_grid, dim3(256), 0, s, f);
    hipLaunchKernelGGL(asw_alt_jobs_kernel, dim3(256 * 8), dim3(256), 0, s, f);
    hipLaunchKernelGGL(asw_alt_decode_kernel, pix_grid, dim3(256), 0, s, f);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int asw_device_impl(Ctx &c, const AswCall &q)
{
    int rc = asw_check_call(q);
    if (rc) return rc > 0 ? SSAMD_OK : rc;
    hipStream_t s = q.s;
    ScratchOrder order(c, s);
    const Tuning &t = tune();
    AswRun r{q, c, t, PlanOptions{t, false}};
    r.exact = q.exact && q.maxD >= q.minD;                            // empty candidate loops: nothing to break ties between
    r.p = q.win / 2; r.nD = q.maxD - q.minD + 1;
    r.nout = (size_t)q.rows * q.W;
    r.grows = q.alternate ? (q.rows + 1) / 2 : q.rows - q.skip;       // workgroup rows: every row (of both ranges), or the even ones
    r.shape = {q.W, r.grows, q.win, r.nD};
    r.r0 = std::max(0, q.row0 - r.p); r.r1 = std::min(q.H, q.row0 + q.rows + r.p);
    r.np2 = (long long)(r.r1 - r.r0) * q.W;
    r.lab_blocks = (int)std::min<long long>((2 * r.np2 + 255) / 256, 256 * 8);
    if ((rc = asw_plan_call(r))) return rc;
    if (r.need_keys && (rc = reset_keys(c.keyL, r.nout, s))) return rc;
    if (q.consistent && (rc = reset_keys(c.keyR, r.nout, s))) return rc;
    if (r.nD >= 1) {
        if ((rc = c.recL.reserve((size_t)q.H * q.W * sizeof(PixRec)))) return rc;
        if ((rc = c.recR.reserve((size_t)q.H * q.W * sizeof(PixRec)))) return rc;
        if ((rc = get_prox(c, q.win, q.gammaP, s, &r.d_prox))) return rc;
        // Round 5: when the call goes straight to its final geometry (no trial launches) and the images are plain byte arrays, the
        // records are NOT launched here: the TAD volume is then built from the images' bytes, independent of the records, and both
        // jobs share one launch (asw_prepass_kernel, see asw_prepare_volume) -- two dependent launches per call instead of three.
        r.lab_pending = r.trial.empty() && !q.rm && t.prepass_fuse != 0;
        if (!r.lab_pending && (rc = asw_lab_records(r))) return rc;
        if (!r.trial.empty() && (rc = asw_autotune(r))) return rc;
        AswGeom final_geom = r.geom;
        if ((rc = asw_final_volume(r, final_geom))) return rc;
        if (r.lab_pending) {                   // no volume for this call (in-kernel e tiles, round-1 kernel): the records on their own
            r.lab_pending = false;
            if ((rc = asw_lab_records(r))) return rc;
        }
        if (r.exact) {
            if (!r.trial.empty()) {
                // the trial launches of the autotuner merged their winners into the keys: start the final launch from clean
                // ones, or its tile-local winners would meet their own copies (asw_exact_merge)
                if (r.need_keys && (rc = reset_keys(c.keyL, r.nout, s))) return rc;
                if (q.consistent && (rc = reset_keys(c.keyR, r.nout, s))) return rc;
            }
            if ((rc = asw_exact_prepare(r, asw_is_direct(r, final_geom)))) return rc;
        }
        Timed agg(c, s, SSAMD_K_ASW_AGG);
        if ((rc = asw_launch(r, final_geom))) return rc;
    }
    const bool direct = asw_is_direct(r, r.geom);
    if (r.exact && r.nD >= 1 && (rc = asw_exact_pass(r, direct))) return rc;
    if (!direct && q.skip > 0) {
        // decode / left-right check of the two bands only; the rows between keep what the interior call wrote
        if ((rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, 0, q.skip_at, q.W, q.d_disp, s)) ||
            (rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, q.skip_at + q.skip, q.rows - q.skip_at - q.skip, q.W, q.d_disp, s)))
            return rc;
    } else if (!direct && (rc = launch_finalize(c, SSAMD_K_ASW_FIN, q.consistent, 0, q.rows, q.W, q.d_disp, s, q.d_raw_right))) return rc;
    return q.alternate && q.rows > 1 ? asw_alternate_fill(r) : SSAMD_OK;
}

// The alternate-rows mode on a row range of a (sub-)image.  row_parity = parity of the sub-image's row 0 in the whole
// image: rows whose index in the whole image is even are matched exactly, the odd ones are filled from their two exact
// neighbours -- so a range that starts or ends with an odd row also needs the exact row just outside it (the caller's
// halo is winSize/2 + 1 rows then).  Those rows are computed into a scratch map and the requested rows copied out.
int asw_alternate_rows(Ctx &c, AswCall q, int row_parity)
{
    int rc = check_common(q.H, q.W, q.win, q.minD, q.maxD, q.row0, q.rows);
    if (rc) return rc;
    if (q.rows == 0) return SSAMD_OK;
    const int row0 = q.row0, rows = q.rows;
    const bool top_odd = ((row0 + row_parity) & 1) != 0, bottom_odd = ((row0 + rows - 1 + row_parity) & 1) != 0;
    if (top_odd && row0 == 0)
        return fail(SSAMD_EINVAL, "alternate rows: the first output row is an odd row of the image, the sub-image must start at least one row above it");
    const int e0 = top_odd ? row0 - 1 : row0, e1 = bottom_odd ? std::min(q.H, row0 + rows + 1) : row0 + rows;
    q.alternate = true;
    if (e0 == row0 && e1 == row0 + rows) return asw_device_impl(c, q);
    ScratchOrder order(c, q.s);
    if ((rc = c.altdisp.reserve((size_t)(e1 - e0) * q.W * 2))) return rc;
    int16_t *const d_disp = q.d_disp;
    q.row0 = e0; q.rows = e1 - e0; q.d_disp = (int16_t *)c.altdisp.ptr;
    if ((rc = asw_device_impl(c, q))) return rc;
    HIP_TRY(hipMemcpyAsync(d_disp, (const int16_t *)c.altdisp.ptr + (size_t)(row0 - e0) * q.W, (size_t)rows * q.W * 2, hipMemcpyDeviceToDevice, q.s));
    return SSAMD_OK;
}
}  // namespace
