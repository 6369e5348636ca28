// Host section of ssamd_api.hip: ASW's fp64 tie-break pass -- its scratch, its steps before and after the aggregation, the reader of its counters.
namespace {
// The scratch of one call of the pass (the x* buffers of the context), said once: the bytes each buffer needs for these sizes ...
struct AswExactLayout { size_t nout, cap, rawcap, wcap, queue_bytes, cost_bytes, raw_bytes, flags_bytes, slots_bytes, wtab_bytes; };
AswExactLayout asw_exact_layout(size_t nout, size_t rows, size_t cap, size_t rawcap, int win)
{
    // weight tables of flagged pixels: up to 64 MB of them (6 800 pixels at a 35 x 35 window; the bench frame flags 133, the 4K frame 3 044)
    const size_t per = (size_t)win * win * 8;
    const size_t wcap = nout >= ((size_t)1 << 31) ? 0 : std::min<size_t>(65536, ((size_t)64 << 20) / per);      // (bit 31 of a slot's pixel is its side)
    return {nout, cap, rawcap, wcap, cap * 8, cap * 8, rawcap * 12, EXACT_CTR_COUNT * 4 + 4 * nout + rows, 2 * nout * (8 + 4 + 4), wcap * 8 + wcap * per};
}
// ... and where its arrays lie, once the buffers are reserved; each of q (final queue), raw (a copy of q to begin with) and x may be null
void asw_exact_carve(const Ctx &c, const AswExactLayout &L, bool consistent, AswExactQueue *q, AswExactQueue *raw, AswExactArgs *x)
{
    unsigned int *const ctr = (unsigned int *)c.xflags.ptr;              // xflags: [counter block][flagL][flagR][zeroL][zeroR] (nout bytes each) [zrow rows]: one memset
    if (q) {
        q->entries = (u64 *)c.xqueue.ptr;                                // xqueue: [cap] entries
        q->counter = ctr + EXACT_CTR_ENTRIES;
        q->flagL = (unsigned char *)(ctr + EXACT_CTR_COUNT);
        q->flagR = consistent ? q->flagL + L.nout : nullptr;
        q->zeroL = q->flagL + 2 * L.nout;
        q->zeroR = consistent ? q->flagL + 3 * L.nout : nullptr;
        q->zrow = q->flagL + 4 * L.nout;
        q->cap = (unsigned int)L.cap;
    }
    if (raw) {
        raw->entries = (u64 *)c.xraw.ptr;                                // xraw: [rawcap] entries, [rawcap] cost images
        raw->ekeys = (uint32_t *)(raw->entries + L.rawcap);
        raw->counter = ctr + EXACT_CTR_RAW;
        raw->flagL = raw->flagR = nullptr;
        raw->cap = (unsigned int)L.rawcap;
    }
    if (x) {
        x->ecost = (double *)c.xcost.ptr;                                // xcost: [cap] fp64 costs
        x->cost[0] = (u64 *)c.xslots.ptr; x->cost[1] = x->cost[0] + L.nout;      // xslots: cost bits of both sides, then idx of both, then wslot of both
        x->idx[0] = (uint32_t *)(x->cost[1] + L.nout); x->idx[1] = x->idx[0] + L.nout;
        x->wslot[0] = x->idx[1] + L.nout; x->wslot[1] = x->wslot[0] + L.nout;
        x->wcap = (unsigned int)L.wcap;
        x->wpix = (uint32_t *)c.xwtab.ptr;                               // xwtab: [wcap] slot pixels (in 8 bytes each), [wcap][win * win] weights
        x->wtab = (double *)((char *)c.xwtab.ptr + L.wcap * 8);
    }
}

// fp64 tie-break pass (asw_exact_kernels.hip.h), part 1 -- BEFORE the aggregation: queue, pixel flags and counters of this call;
// fills r.xq_kernel, the AswExactQueue the aggregation kernels append their near-ties to (round 6: no cost-image volume).
int asw_exact_prepare(AswRun &r, bool direct)
{
    Ctx &c = r.c;
    AswExactQueue &q = r.xq_final, &raw = r.xq_raw;
    const size_t nout = r.nout;
    if (nout >= ((size_t)1 << 32)) return fail(SSAMD_ELIMIT, "exact mode: more than 2^32 output pixels per call");
    // queue: room for a few candidates of every pixel, bounded (a frame of saturated noise can flag every candidate of every
    // pixel; an overflow leaves the fp32 map and is reported: `exact_overflow`); frames of up to 4M candidates in all get room
    // for every one of them on both sides -- a flat test image cannot overflow
    // (a candidate can be queued once per side -- by a select and by a merge, or by the left and the right escalation)
    const size_t all_cands = 2 * (nout * (size_t)r.nD + nout);
    size_t cap = std::min<size_t>(std::max<size_t>(4 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (tune().exact_cap) cap = (size_t)tune().exact_cap;
    // raw queue of merging calls (12 B per entry): what workgroups select against their tile-local winners
    size_t rawcap = direct ? 0 : std::min<size_t>(std::max<size_t>(2 * nout, std::min<size_t>(all_cands, (size_t)1 << 23)), (size_t)1 << 26);
    if (!direct && tune().exact_cap) rawcap = std::max<size_t>(rawcap, cap);
    if (!direct && tune().exact_rawcap) rawcap = (size_t)tune().exact_rawcap;
    const AswExactLayout L = asw_exact_layout(nout, (size_t)r.rows, cap, rawcap, r.win);
    int rc;
    if ((rc = c.xqueue.reserve(L.queue_bytes)) || (rc = c.xcost.reserve(L.cost_bytes)) || (rc = c.xflags.reserve(L.flags_bytes)) ||
        (rc = c.xslots.reserve(L.slots_bytes)) || (rawcap && (rc = c.xraw.reserve(L.raw_bytes))))
        return rc;
    HIP_TRY(hipMemsetAsync(c.xflags.ptr, 0, L.flags_bytes, r.s));
    asw_exact_carve(c, L, r.consistent, &q, nullptr, nullptr);
    q.W = (unsigned int)r.W;
    // Near-tie band.  128 ulps = 1.5e-5 relative at gammaC = 5 and a 35 x 35 window: the kernels' support weights inherit the
    // rounding of the Lab records to float (|dLab| <= ~1.3e-5 per colour distance), i.e. a relative error of ~2.6e-5 / gammaC on a
    // weight product -- scaled up for smaller gammaC; and the (N, S') sums are fp32 sums of win^2 products whose rounding errors
    // add up like a random walk (~win ulps): scaled up with the window beyond 35 (a fixed band ignored the tap
    // count; tests/test_gpu_exact.py::test_large_windows_against_the_oracle).
    // MEASURED (profiles/exact_band_margin.txt, tests/test_gpu_asw_band.py): what the band has to cover is the error of the
    // DIFFERENCE between the reference's winner and another candidate of the pixel, and their errors move together (shared left
    // weights).  Worst line: 43 of 128 ulps in use (window 21, gammaC 5, gammaP 100), 23 of 128 at 35 / 5 / 17.5, under 5 % of
    // the band wherever it is scaled up; half the band still reproduced every map of the canaries, a quarter did not.
    q.tol = (uint32_t)std::min(1.0e6, (double)tune().exact_tol * std::max(1.0, 5.0 / r.gammaC) * std::max(1.0, r.win / 35.0));
    // rounding noise of the reference's fp64 quotient sum(w e) / sum(w) over n = win^2 taps: <= ~(n + 3) u relative on numerator and
    // denominator each, u = 2^-53, i.e. 2 (n + 3) u 40 absolute near the cap; two candidates can swap places when they are
    // closer than twice that (x 1.5 margin)
    q.sat_abs = (float)(1.5 * 2.0 * 2.0 * ((double)r.win * r.win + 3.0) * 1.1102230246251565e-16 * 40.0);
    q.deep = 0xffffffffu;
    raw = AswExactQueue{};
    if (!direct) {
        raw = q;
        asw_exact_carve(c, L, r.consistent, nullptr, &raw, nullptr);
        raw.deep = asw_inv_key(q.sat_abs);                               // images with 40 - cost <= sat_abs stay out of the raw queue
    }
    r.xq_kernel = direct ? q : raw;
    c.xq[0] = q; c.xq[1] = raw;
    return SSAMD_OK;
}

// ... part 2 -- AFTER the aggregation: the queue holds the near-ties of every winner, c.keyL / c.keyR (or the map itself when the
// aggregation wrote it: `direct`) the fp32 winners.  Rewrites the winners of pixels whose near-ties fp64 decides differently.
int asw_exact_pass(AswRun &r, bool direct)
{
    Ctx &c = r.c;
    hipStream_t s = r.s;
    const int H = r.H, W = r.W, p = r.p;
    const size_t npix = (size_t)H * W;
    const AswExactLayout L = asw_exact_layout(r.nout, (size_t)r.rows, r.xq_final.cap, r.xq_raw.cap, r.win);
    int rc;
    AswExactArgs x;
    if ((rc = get_prox64(c, r.win, r.gammaP, s, &x.prox))) return rc;
    if ((rc = c.xlabL.reserve(npix * 24)) || (rc = c.xlabR.reserve(npix * 24))) return rc;
    if (L.wcap && (rc = c.xwtab.reserve(L.wtab_bytes))) return rc;
    x.rec[0] = (const PixRec *)c.recL.ptr; x.rec[1] = (const PixRec *)c.recR.ptr;
    x.lab[0] = (const double *)c.xlabL.ptr; x.lab[1] = (const double *)c.xlabR.ptr;
    x.keys[0] = direct ? nullptr : (u64 *)c.keyL.ptr; x.keys[1] = r.consistent ? (u64 *)c.keyR.ptr : nullptr;
    x.disp = r.d_disp;
    x.q = r.xq_final;
    x.raw = r.xq_raw;
    asw_exact_carve(c, L, r.consistent, nullptr, nullptr, &x);
    x.H = H; x.W = W; x.win = r.win; x.pad = p; x.minD = r.minD; x.maxD = r.maxD; x.row0 = r.row0; x.rows = r.rows;
    x.gammaC = r.gammaC;
    Timed t(c, s, SSAMD_K_ASW_EXACT);
    {
        const int r0 = std::max(0, r.row0 - p), r1 = std::min(H, r.row0 + r.rows + p);
        const long long np2 = (long long)(r1 - r0) * W;
        const int blocks = (int)std::min<long long>((2 * np2 + 255) / 256, 256 * 8);
        hipLaunchKernelGGL(bgr2lab_f64_pair_kernel, dim3(blocks), dim3(256), 0, s, x.rec[0] + (size_t)r0 * W, x.rec[1] + (size_t)r0 * W,
                           (double *)c.xlabL.ptr + 3 * (size_t)r0 * W, (double *)c.xlabR.ptr + 3 * (size_t)r0 * W, np2);
    }
    const int pb = (int)std::min<long long>(((long long)r.nout + 255) / 256, 256 * 8);
    if (x.raw.entries) {
        hipLaunchKernelGGL(asw_exact_filter_kernel, dim3(256 * 8), dim3(256), 0, s, x);
        hipLaunchKernelGGL(asw_exact_escalate_kernel, dim3(pb), dim3(256), 0, s, x);
    }
    {
        const int zwin = std::min(r.win, EXACT_ZWIN_MAX - 1);
        const size_t zlds = (size_t)2 * zwin * (EXACT_ZSEG + 2 * (zwin / 2)) * 4;                      // two window-row tiles (<= 63 x 126 x 4 B x 2)
        if ((rc = grant_dyn_lds(c, (const void *)asw_exact_zero_kernel, (int)zlds))) return rc;
        const long long segs = (long long)r.rows * ((W + EXACT_ZSEG - 1) / EXACT_ZSEG);
        hipLaunchKernelGGL(asw_exact_zero_kernel, dim3((unsigned)std::min<long long>(segs, 256 * 64)), dim3(256), zlds, s, x);
    }
    hipLaunchKernelGGL(asw_exact_winners_kernel, dim3(pb), dim3(256), 0, s, x);
    if (x.wcap) hipLaunchKernelGGL(asw_exact_wtab_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_eval_kernel, dim3((unsigned)(c.cus * EXACT_GROUPS_PER_CU)), dim3(64 * EXACT_WAVES), 0, s, x);
    hipLaunchKernelGGL(asw_exact_resolve_kernel, dim3(256 * 4), dim3(256), 0, s, x);
    hipLaunchKernelGGL(asw_exact_patch_kernel, dim3(pb), dim3(256), 0, s, x);
    HIP_TRY(hipGetLastError());
    ++c.exact_calls;
    return SSAMD_OK;
}

// The counter block (ExactCounter) of the LAST exact call on this device: the head of the flag buffer; all 0 when none has run
int asw_exact_counters(Ctx &c, unsigned int (&ctr)[EXACT_CTR_COUNT])
{
    std::fill(ctr, ctr + EXACT_CTR_COUNT, 0u);
    if (!c.xflags.ptr || c.exact_calls == 0) return SSAMD_OK;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ctr, c.xflags.ptr, sizeof(ctr), hipMemcpyDeviceToHost));
    return SSAMD_OK;
}
}  // namespace
