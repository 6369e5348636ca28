// Host section of ssamd_api.hip: ASW's fp64 tie-break pass -- its steps before and after the aggregation, the reader of its counters.
namespace {
int get_prox64(Ctx &c, int win, double gammaP, hipStream_t s, const double **out);      // (host_asw.h, next to get_prox)

// fp64 tie-break pass (asw_exact_kernels.hip.h), part 1 -- BEFORE the aggregation: queue, pixel flags and counters of this call;
// fills the AswExactQueue the aggregation kernels append their near-ties to (round 6: no cost-image volume).
int asw_exact_prepare(Ctx &c, int W, int rows, int win, int nD, double gammaC, bool consistent, bool direct, hipStream_t s,
                      AswExactQueue &q, AswExactQueue &raw, AswExactQueue &kernel_q)
{
    const size_t nout = (size_t)rows * W;
    if (nout >= ((size_t)1 << 32)) return fail(SSAMD_ELIMIT, "exact mode: more than 2^32 output pixels per call");
    // queue: room for a few candidates of every pixel, bounded (a frame of saturated noise can flag every candidate of every
    // pixel; an overflow leaves the fp32 map and is reported: `exact_overflow`); frames of up to 4M candidates in all get room
    // for every one of them on both sides -- a flat test image cannot overflow
    // (a candidate can be queued once per side -- by a select and by a merge, or by the left and the right escalation)
    const size_t all_cands = 2 * (nout * (size_t)nD + nout);
    size_t cap = std::min<size_t>(std::max<size_t>(4 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (tune().exact_cap) cap = (size_t)tune().exact_cap;
    // raw queue of merging calls (12 B per entry): what workgroups select against their tile-local winners
    size_t rawcap = direct ? 0 : std::min<size_t>(std::max<size_t>(2 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (!direct && tune().exact_cap) rawcap = std::max<size_t>(rawcap, cap);
    if (!direct && tune().exact_rawcap) rawcap = (size_t)tune().exact_rawcap;
    int rc;
    // [64 B counters][flagL][flagR][zeroL][zeroR] (nout bytes each) [zrow rows]: one buffer, one memset
    if ((rc = c.xqueue.reserve(cap * 8)) || (rc = c.xcost.reserve(cap * 8)) || (rc = c.xflags.reserve(64 + 4 * nout + (size_t)rows)) ||
        (rc = c.xslots.reserve(nout * 32)) || (rawcap && (rc = c.xraw.reserve(rawcap * 12))))
        return rc;
    c.xcap = (unsigned int)cap;
    c.xrawcap = (unsigned int)rawcap;
    HIP_TRY(hipMemsetAsync(c.xflags.ptr, 0, 64 + 4 * nout + (size_t)rows, s));
    q.entries = (u64 *)c.xqueue.ptr;
    q.ekeys = nullptr;
    q.counter = (unsigned int *)c.xflags.ptr;
    q.flagL = (unsigned char *)c.xflags.ptr + 64;
    q.flagR = consistent ? q.flagL + nout : nullptr;
    q.zeroL = q.flagL + 2 * nout;
    q.zeroR = consistent ? q.flagL + 3 * nout : nullptr;
    q.zrow = q.flagL + 4 * nout;
    q.W = (unsigned int)W;
    q.cap = (unsigned int)cap;
    // Near-tie band.  128 ulps = 1.5e-5 relative at gammaC = 5 and a 35 x 35 window: the kernels' support weights inherit the
    // rounding of the Lab records to float (|dLab| <= ~1.3e-5 per colour distance), i.e. a relative error of ~2.6e-5 / gammaC on a
    // weight product -- scaled up for smaller gammaC; and the (N, S') sums are fp32 sums of win^2 products whose rounding errors
    // add up like a random walk (~win ulps): scaled up with the window beyond 35 (a fixed band ignored the tap
    // count; tests/test_gpu_exact.py::test_large_windows_against_the_oracle).
    // MEASURED (profiles/exact_band_margin.txt, tests/test_gpu_asw_band.py): what the band has to cover is the error of the
    // DIFFERENCE between the reference's winner and another candidate of the pixel, and their errors move together (shared left
    // weights).  Worst line: 43 of 128 ulps in use (window 21, gammaC 5, gammaP 100), 23 of 128 at 35 / 5 / 17.5, under 5 % of
    // the band wherever it is scaled up; half the band still reproduced every map of the canaries, a quarter did not.
    q.tol = (uint32_t)std::min(1.0e6, (double)tune().exact_tol * std::max(1.0, 5.0 / gammaC) * std::max(1.0, win / 35.0));
    // rounding noise of the reference's fp64 quotient sum(w e) / sum(w) over n = win^2 taps: <= ~(n + 3) u relative on numerator and
    // denominator each, u = 2^-53, i.e. 2 (n + 3) u 40 absolute near the cap; two candidates can swap places when they are
    // closer than twice that (x 1.5 margin)
    q.sat_abs = (float)(1.5 * 2.0 * 2.0 * ((double)win * win + 3.0) * 1.1102230246251565e-16 * 40.0);
    q.deep = 0xffffffffu;
    raw = AswExactQueue{};
    if (!direct) {
        raw = q;
        union { float f; uint32_t u; } sa; sa.f = q.sat_abs;
        raw.deep = 0xC0000000u - sa.u;                                   // images with 40 - cost <= sat_abs stay out of the raw queue
        raw.entries = (u64 *)c.xraw.ptr;
        raw.ekeys = (uint32_t *)((u64 *)c.xraw.ptr + rawcap);
        raw.counter = q.counter + 4;
        raw.flagL = raw.flagR = nullptr;
        raw.cap = (unsigned int)rawcap;
    }
    kernel_q = direct ? q : raw;
    return SSAMD_OK;
}

// ... part 2 -- AFTER the aggregation: the queue holds the near-ties of every winner, c.keyL / c.keyR (or the map itself when the
// aggregation wrote it: `direct`) the fp32 winners.  Rewrites the winners of pixels whose near-ties fp64 decides differently.
int asw_exact_pass(Ctx &c, const AswExactQueue &q, const AswExactQueue &raw, int H, int W, int row0, int rows, int win, int maxD, int minD, double gammaC, double gammaP,
                   bool consistent, bool direct, int16_t *d_disp, hipStream_t s)
{
    const int p = win / 2;
    const size_t nout = (size_t)rows * W, npix = (size_t)H * W;
    int rc;
    const double *d_prox = nullptr;
    if ((rc = get_prox64(c, win, gammaP, s, &d_prox))) return rc;
    if ((rc = c.xlabL.reserve(npix * 24)) || (rc = c.xlabR.reserve(npix * 24))) return rc;
    AswExactArgs x;
    x.recL = (const PixRec *)c.recL.ptr; x.recR = (const PixRec *)c.recR.ptr;
    x.labL = (const double *)c.xlabL.ptr; x.labR = (const double *)c.xlabR.ptr;
    x.prox = d_prox;
    x.keyL = direct ? nullptr : (u64 *)c.keyL.ptr; x.keyR = consistent ? (u64 *)c.keyR.ptr : nullptr;
    x.disp = d_disp;
    x.q = q;
    x.raw = raw;
    x.ecost = (double *)c.xcost.ptr;
    x.costL = (u64 *)c.xslots.ptr; x.costR = x.costL + nout;
    x.idxL = (uint32_t *)(x.costR + nout); x.idxR = x.idxL + nout;
    x.wslotL = x.idxR + nout; x.wslotR = x.wslotL + nout;
    // weight tables of flagged pixels: up to 64 MB of them (6 800 pixels at a 35 x 35 window; the bench frame flags 133, the 4K frame 3 044)
    {
        const size_t per = (size_t)win * win * 8;
        size_t wcap = std::min<size_t>(65536, ((size_t)64 << 20) / per);
        if (nout >= ((size_t)1 << 31)) wcap = 0;
        if (wcap && (rc = c.xwtab.reserve(wcap * 8 + wcap * per))) return rc;
        x.wcap = (unsigned int)wcap;
        x.wpix = (uint32_t *)c.xwtab.ptr;
        x.wtab = (double *)((char *)c.xwtab.ptr + wcap * 8);
    }
    x.H = H; x.W = W; x.win = win; x.pad = p; x.minD = minD; x.maxD = maxD; x.row0 = row0; x.rows = rows;
    x.gammaC = gammaC;
    Timed t(c, s, SSAMD_K_ASW_EXACT);
    {
        const int r0 = std::max(0, row0 - p), r1 = std::min(H, row0 + rows + p);
        const long long np2 = (long long)(r1 - r0) * W;
        const int blocks = (int)std::min<long long>((2 * np2 + 255) / 256, 256 * 8);
        hipLaunchKernelGGL(bgr2lab_f64_pair_kernel, dim3(blocks), dim3(256), 0, s, x.recL + (size_t)r0 * W, x.recR + (size_t)r0 * W,
                           (double *)c.xlabL.ptr + 3 * (size_t)r0 * W, (double *)c.xlabR.ptr + 3 * (size_t)r0 * W, np2);
    }
    const int pb = (int)std::min<long long>(((long long)nout + 255) / 256, 256 * 8);
    if (raw.entries) {
        hipLaunchKernelGGL(asw_exact_filter_kernel, dim3(256 * 8), dim3(256), 0, s, x);
        hipLaunchKernelGGL(asw_exact_escalate_kernel, dim3(pb), dim3(256), 0, s, x);
    }
    {
        const int zwin = std::min(win, EXACT_ZWIN_MAX - 1);
        const size_t zlds = (size_t)2 * zwin * (EXACT_ZSEG + 2 * (zwin / 2)) * 4;                      // two window-row tiles (<= 63 x 126 x 4 B x 2)
        if ((rc = grant_dyn_lds(c, (const void *)asw_exact_zero_kernel, (int)zlds))) return rc;
        const long long segs = (long long)rows * ((W + EXACT_ZSEG - 1) / EXACT_ZSEG);
        hipLaunchKernelGGL(asw_exact_zero_kernel, dim3((unsigned)std::min<long long>(segs, 256 * 64)), dim3(256), zlds, s, x);
    }
    hipLaunchKernelGGL(asw_exact_winners_kernel, dim3(pb), dim3(256), 0, s, x);
    if (x.wcap) hipLaunchKernelGGL(asw_exact_wtab_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_eval_kernel, dim3((unsigned)(c.cus * 5)), dim3(64 * EXACT_WAVES), 0, s, x);      // five 4-wave groups per CU are resident (91 VGPRs)
    hipLaunchKernelGGL(asw_exact_resolve_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_patch_kernel, dim3(pb), dim3(256), 0, s, x);
    HIP_TRY(hipGetLastError());
    ++c.exact_calls;
    return SSAMD_OK;
}

// The counters of the LAST exact call on this device (head of the flag buffer): final entries, flagged left / right, -, raw entries; 0 when none has run
int asw_exact_counters(Ctx &c, unsigned int (&ctr)[5])
{
    std::fill(ctr, ctr + 5, 0u);
    if (!c.xflags.ptr || c.exact_calls == 0) return SSAMD_OK;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ctr, c.xflags.ptr, sizeof(ctr), hipMemcpyDeviceToHost));
    return SSAMD_OK;
}
}  // namespace
