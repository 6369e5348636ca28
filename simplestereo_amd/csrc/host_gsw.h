// Host section of ssamd_api.hip: GSW -- the weight table, GswCall (what an entry point asks for) and one call.
namespace {
// support weight as a function of the integer squared colour distance, in the reference's
// arithmetic: fl32 distance (sqrt in double), float division by gamma, float exp (_passive.cpp:457-463, 495)
int get_gsw_table(Ctx &c, int gamma, hipStream_t s, const float **out)
{
    return get_table(c.gswTabs, gamma, 0.0, (size_t)GSW_TAB_SIZE, "GSW weight table", s, out, [&](float *host) {
        for (int v = 0; v < GSW_TAB_SIZE; ++v) {
            const float dist = (float)(0.0f + std::sqrt((double)v));
            host[v] = expf(-dist / gamma);
        }
    });
}

// What an entry point asks for, as AswCall (host_asw.h): images, geometry, window, disparity range, output and stream are
// MatchCall's; d_disp starts at row0.
struct GswCall : MatchCall {
    int gamma = 0;
    float fMax = 0;
    int iterations = 0;
    int16_t *d_raw_right = nullptr;     // verification dump (ssamd_gsw_argmins): both raw winners instead of the left-right check and filling
};

GswCall gsw_params(int H, int W, int win, int maxD, int minD, int gamma, float fMax, int iterations)      // (images, rows, output, stream: by field name)
{
    GswCall q;
    q.H = H; q.W = W; q.win = win; q.maxD = maxD; q.minD = minD; q.gamma = gamma; q.fMax = fMax; q.iterations = iterations;
    return q;
}

int gsw_device_impl(Ctx &c, const GswCall &q)
{
    const int H = q.H, W = q.W, row0 = q.row0, rows = q.rows, win = q.win, maxD = q.maxD, minD = q.minD;
    hipStream_t s = q.s;
    int rc = check_common(H, W, win, minD, maxD, row0, rows);
    if (rc) return rc;
    if (q.gamma == 0) return fail(SSAMD_EINVAL, "gamma must be non-zero");
    if (rows == 0) return SSAMD_OK;
    ScratchOrder order(c, s);
    const Tuning &opts = tune();
    const int p = win / 2, nD = maxD - minD + 1;
    const size_t npix = (size_t)H * W, nout = (size_t)rows * W;
    if ((rc = c.keyL.reserve(nout * 8)) || (rc = c.keyR.reserve(nout * 8))) return rc;
    HIP_TRY(hipMemsetAsync(c.keyL.ptr, 0xFF, nout * 8, s));
    HIP_TRY(hipMemsetAsync(c.keyR.ptr, 0xFF, nout * 8, s));
    if (nD >= 1) {
        // packed pixels live in the (larger) ASW record buffers: 4 B/pixel
        if ((rc = c.recL.reserve(npix * 4)) || (rc = c.recR.reserve(npix * 4))) return rc;
        const float *d_tab = nullptr;
        if ((rc = get_gsw_table(c, q.gamma, s, &d_tab))) return rc;
        const int r0 = std::max(0, row0 - p), r1 = std::min(H, row0 + rows + p);
        const long long np = (long long)(r1 - r0) * W;
        const int blocks = (int)std::min<long long>((np + 255) / 256, 256 * 8);
        {
            Timed t(c, s, SSAMD_K_LAB);
            if (q.rm) {       // raw frames through the rig's maps: rectification + packing of both images, one launch
                hipLaunchKernelGGL(remap_pack_pair_kernel, dim3(blocks), dim3(256), 0, s, *q.rm, (uint32_t *)c.recL.ptr, (uint32_t *)c.recR.ptr,
                                   (long long)r0 * W, np);
            } else {
                hipLaunchKernelGGL(bgr_pack_kernel, dim3(blocks), dim3(256), 0, s, q.dL + (size_t)r0 * W * 3,
                                   (uint32_t *)c.recL.ptr + (size_t)r0 * W, np);
                hipLaunchKernelGGL(bgr_pack_kernel, dim3(blocks), dim3(256), 0, s, q.dR + (size_t)r0 * W * 3,
                                   (uint32_t *)c.recR.ptr + (size_t)r0 * W, np);
            }
            HIP_TRY(hipGetLastError());
        }
        // The tiled kernel's layout assumes non-negative finite costs (its keys order cost bits as unsigned) and weight 0 for the
        // cells the relaxation never reaches (a skipped tap is w * 0): true for gamma > 0 and a cap >= 0.  The rest -- and any
        // call under SSAMD_GSW_PLAIN -- runs the reference's loops as they stand (gsw_plain_kernel), counted in gsw_plain_calls.
        if (q.gamma < 0 || q.fMax < 0 || q.fMax != q.fMax || opts.gsw_plain) {
            GswPlainArgs pa;
            pa.img[0] = (const uint32_t *)c.recL.ptr; pa.img[1] = (const uint32_t *)c.recR.ptr;
            pa.key[0] = (u64 *)c.keyL.ptr; pa.key[1] = (u64 *)c.keyR.ptr;
            pa.tab = d_tab;
            pa.H = H; pa.W = W; pa.win = win; pa.pad = p; pa.minD = minD; pa.maxD = maxD; pa.row0 = row0; pa.rows = rows;
            pa.iterations = q.iterations; pa.fMax = q.fMax;
            pa.w_unreached = expf(-INFINITY / q.gamma);
            ++c.gsw_plain_calls;
            hipLaunchKernelGGL(gsw_plain_kernel, dim3((unsigned)((nout + 255) / 256), 1, 2), dim3(256), 0, s, pa);
            HIP_TRY(hipGetLastError());
            return launch_finalize(c, SSAMD_K_GSW_FIN, true, 0, rows, W, q.d_disp, s, q.d_raw_right);
        }
        GswArgs a;
        if ((rc = gsw_choose_geometry(a.g, opts, W, rows, win, nD))) return rc;
        a.tab = d_tab;
        a.H = H; a.W = W; a.win = win; a.pad = p; a.minD = minD; a.maxD = maxD; a.row0 = row0; a.rows = rows;
        a.iterations = q.iterations; a.fMax = q.fMax;
        // both passes with geometry g (the winner-take-all keys merge by atomicMin: repeated launches are idempotent)
        auto launch = [&](const GswGeom &g) -> int {
            a.g = g;
            const int TyS = g.Ty * g.Hy;
            const dim3 grid((W + g.Tx - 1) / g.Tx, (rows + TyS - 1) / TyS, g.nchunks), block(g.threads * g.Hy);
            auto kernel = g.Ty == 2 ? gsw_aggregate_kernel<2, 4> : gsw_aggregate_kernel<1, 8>;
            if (int grc = grant_dyn_lds(c, (const void *)kernel, g.lds_bytes)) return grc;
            for (int pass = 0; pass < 2; ++pass) {
                a.right = pass;
                a.ref = (const uint32_t *)(pass ? c.recR.ptr : c.recL.ptr);
                a.tgt = (const uint32_t *)(pass ? c.recL.ptr : c.recR.ptr);
                a.key = (u64 *)(pass ? c.keyR.ptr : c.keyL.ptr);
                hipLaunchKernelGGL(kernel, grid, block, g.lds_bytes, s, a);
                HIP_TRY(hipGetLastError());
            }
            return SSAMD_OK;
        };
        // Autotuning (ssamd_autotune, as for ASW): the first call of a shape times the candidates of gsw_candidates on the
        // call's own buffers -- three rounds in round-robin order, fastest launch of each (autotune_rounds) -- and caches the winner.  Default
        // mode: calls of at most 6e10 window taps (both passes; 2 lane-ops each: about 5 ms), where the model is least reliable.
        const ShapeKey shape{W, rows, win, nD};
        if (autotune_due(g_gsw_geom, shape, 2.0 * (double)W * rows * nD * win * win) && opts.gsw_geom.empty()) {
            std::vector<GswGeom> trial;
            gsw_candidates(trial, a.g, W, rows, win, nD);
            if (trial.size() >= 2) {
                hipEvent_t e0 = nullptr, e1 = nullptr;
                HIP_TRY(hipEventCreate(&e0));
                if (hipEventCreate(&e1) != hipSuccess) {
                    (void)hipEventDestroy(e0);
                    return fail(SSAMD_EHIP, "hipEventCreate failed");
                }
                const int fastest = autotune_rounds(trial.size(), 3, true, e0, e1, s, nullptr, [&](size_t ci) { return launch(trial[ci]) == SSAMD_OK; });
                (void)hipGetLastError();
                g_err.clear();            // a failed trial launch is not the call's error
                a.g = trial[std::max(0, fastest)];
                (void)hipEventDestroy(e0);
                (void)hipEventDestroy(e1);
                autotune_keep(g_gsw_geom, shape, a.g);
            }
        }
        {
            const GswGeom final_geom = a.g;
            Timed t(c, s, SSAMD_K_GSW_AGG);
            if ((rc = launch(final_geom))) return rc;
        }
    }
    return launch_finalize(c, SSAMD_K_GSW_FIN, true, 0, rows, W, q.d_disp, s, q.d_raw_right);   // consistency is unconditional in GSW
}
}  // namespace
