// Host section of ssamd_api.hip: FTP phase of an image pair and of one image (ftp_kernels.hip.h, ftp_plan.h) -- check, twiddle
// tables, the one launch, entry points (include/ssamd.h; the one-image pair in include/ssamd_ftp_mapping.h).
namespace {
// band planning, table and launches of ssamd_ftp_phase*; the caller holds the context and has ordered the scratch (ScratchOrder)
static_assert(FTP_MAX_W == SSAMD_FTP_MAX_W, "ssamd.h states the width limit of ftp_plan.h");
int ftp_check(int ch_obj, int ch_ref, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau)
{
    if (h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if ((ch_obj != 1 && ch_obj != 3) || (ch_ref != 1 && ch_ref != 3)) return fail(SSAMD_EINVAL, "images must have 1 or 3 channels");
    if (!fmin || !fmax) return fail(SSAMD_EINVAL, "NULL band bounds");
    if (unwrap < 0 || unwrap > 2) return fail(SSAMD_EINVAL, "unwrap must be 0, 1 or 2");
    if (w > FTP_MAX_W) return fail(SSAMD_ELIMIT, "rows wider than %d columns are not supported (width %d)", FTP_MAX_W, w);
    if (unwrap == 2) {                                   // tau is not read
        NpuXY q;
        return npu_xy_check(1, h, w, q);
    }
    return unwrap == 1 ? unwrap_check(1, h, w, tau) : SSAMD_OK;
}

int ftp_twiddles(Ctx &c, int w, hipStream_t s, const double2 **tw)
{
    auto it = c.ftpTabs.find(w);
    if (it == c.ftpTabs.end()) {
        if (c.ftpTabs.size() >= 16) {                    // hipFree waits for the kernels that may still read a table
            for (auto &e : c.ftpTabs) e.second.release();
            c.ftpTabs.clear();
        }
        DevBuf buf;
        int rc = buf.reserve((size_t)w * sizeof(double2));
        if (rc) return rc;
        hipLaunchKernelGGL(ftp_twiddle_kernel, dim3((w + 255) / 256), dim3(256), 0, s, (double2 *)buf.ptr, w);
        HIP_TRY(hipGetLastError());
        it = c.ftpTabs.emplace(w, buf).first;
    }
    *tw = (const double2 *)it->second.ptr;
    return SSAMD_OK;
}

// The kept bins of every row, planned on the host and uploaded to c.ftpBand on `s`, and the twiddle table of the width: what
// ftp_dft_launch does before its kernel.  max_bins: the longest band.
int ftp_stage_bands(Ctx &c, int h, int w, const double *fmin, const double *fmax, hipStream_t s, int &max_bins, const double2 **tw)
{
    int rc;
    // the bands go through pinned staging that the previous call's upload may still be reading
    if (!c.ftp_band_copied) HIP_TRY(hipEventCreateWithFlags(&c.ftp_band_copied, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(c.ftp_band_copied));
    if ((size_t)h > c.ftpBandHostCap) {
        if (c.ftpBandHost) { (void)hipHostFree(c.ftpBandHost); c.ftpBandHost = nullptr; c.ftpBandHostCap = 0; }
        const size_t want = (size_t)h + (size_t)h / 8 + 64;
        HIP_TRY(hipHostMalloc((void **)&c.ftpBandHost, want * 2 * sizeof(int32_t), hipHostMallocDefault));
        c.ftpBandHostCap = want;
    }
    max_bins = 0;
    for (int y = 0; y < h; ++y) {
        int32_t lo, hi;
        ftp_band_row(w, fmin[y], fmax[y], lo, hi);
        c.ftpBandHost[2 * (size_t)y] = lo;
        c.ftpBandHost[2 * (size_t)y + 1] = hi;
        max_bins = std::max(max_bins, hi - lo + 1);
    }
    if ((rc = c.ftpBand.reserve((size_t)h * 2 * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(c.ftpBand.ptr, c.ftpBandHost, (size_t)h * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c.ftp_band_copied, s));
    return ftp_twiddles(c, w, s, tw);
}

// the unwrapping that follows a wrapped map on the same stream: 0 none, 1 IIR (d_phase, a buffer of the context's, -> d_out),
// 2 np.unwrap along x then y (in place in d_out)
int ftp_unwrap_tail(Ctx &c, int unwrap, double tau, const double *d_phase, int h, int w, double *d_out, hipStream_t s)
{
    if (unwrap == 2) {
        NpuXY q;
        int rc = npu_xy_check(1, h, w, q);               // cannot fail: ftp_check has asked before anything was enqueued
        if (rc) return rc;
        return npu_xy_launch(c, q, d_out, h, w, d_out, s);
    }
    return unwrap ? unwrap_launch(c, d_phase, 1, h, w, tau, d_out, s) : SSAMD_OK;
}

// One DFT launch and its unwrapping tail.  images == 2: ftp_phase_kernel of d_obj against d_ref; images == 1: ftp_carrier_kernel of
// d_obj alone (d_ref and ch_ref are not read).
int ftp_dft_launch(Ctx &c, int images, const uint8_t *d_obj, int ch_obj, const uint8_t *d_ref, int ch_ref, int h, int w, const double *fmin,
                   const double *fmax, int unwrap, double tau, double *d_out, hipStream_t s)
{
    int rc, max_bins;
    const double2 *tw = nullptr;
    if ((rc = ftp_stage_bands(c, h, w, fmin, fmax, s, max_bins, &tw))) return rc;
    double *d_phase = d_out;
    if (unwrap == 1) {                                   // the wavefront kernel does not work in place
        if ((rc = c.ftpPhase.reserve((size_t)h * w * sizeof(double)))) return rc;
        d_phase = (double *)c.ftpPhase.ptr;
    }
    const FtpGeom g = ftp_geometry(w, images);
    const int q = ftp_lanes_per_bin(g.threads, std::max(max_bins, 1));
    auto launch = [&](auto kernel, auto... images) -> int {
        int r = grant_dyn_lds(c, reinterpret_cast<const void *>(kernel), g.lds_bytes);
        if (r) return r;
        Timed t(c, s, SSAMD_K_FTP);
        hipLaunchKernelGGL(kernel, dim3(h), dim3(g.threads), g.lds_bytes, s, images..., w, (const int2 *)c.ftpBand.ptr, tw, q, FTP_BIN_CHUNK,
                           d_phase);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    };
    static constexpr decltype(&ftp_phase_kernel<1>) pair[4] = {ftp_phase_kernel<1>, ftp_phase_kernel<2>, ftp_phase_kernel<4>, ftp_phase_kernel<8>};
    static constexpr decltype(&ftp_carrier_kernel<1>) one[4] = {ftp_carrier_kernel<1>, ftp_carrier_kernel<2>, ftp_carrier_kernel<4>,
                                                                ftp_carrier_kernel<8>};
    const int i = g.cpt == 1 ? 0 : g.cpt == 2 ? 1 : g.cpt == 4 ? 2 : 3;                                  // by columns per thread
    if ((rc = images == 2 ? launch(pair[i], d_obj, ch_obj, d_ref, ch_ref) : launch(one[i], d_obj, ch_obj))) return rc;
    return ftp_unwrap_tail(c, unwrap, tau, d_phase, h, w, d_out, s);
}
}  // namespace

extern "C" {
int ssamd_ftp_band(int w, int h, const double *fmin, const double *fmax, int32_t *slo, int32_t *shi)
{
    if (w <= 0 || h < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (h > 0 && (!fmin || !fmax || !slo || !shi)) return fail(SSAMD_EINVAL, "NULL buffer");
    for (int y = 0; y < h; ++y) ftp_band_row(w, fmin[y], fmax[y], slo[y], shi[y]);
    return SSAMD_OK;
}

int ssamd_ftp_phase(const uint8_t *img_obj, int ch_obj, const uint8_t *img_ref, int ch_ref, int h, int w, const double *fmin,
                    const double *fmax, int unwrap, double tau, double *out, int device)
{
    if (!img_obj || !img_ref || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch_obj, ch_ref, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    const size_t px = (size_t)h * w;
    return host_route(device, {{&Ctx::imgL, img_obj, px * ch_obj}, {&Ctx::imgR, img_ref, px * ch_ref}}, {&Ctx::uwOut, out, px * sizeof(double)},
                      [&](Ctx &c, hipStream_t s) {
                          return ftp_dft_launch(c, 2, (const uint8_t *)c.imgL.ptr, ch_obj, (const uint8_t *)c.imgR.ptr, ch_ref, h, w, fmin, fmax, unwrap,
                                                tau, (double *)c.uwOut.ptr, s);
                      });
}

int ssamd_ftp_phase_device(const uint8_t *d_img_obj, int ch_obj, const uint8_t *d_img_ref, int ch_ref, int h, int w,
                           const double *fmin, const double *fmax, int unwrap, double tau, double *d_out, void *stream)
{
    if (!d_img_obj || !d_img_ref || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch_obj, ch_ref, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    ScratchOrder order(*c, (hipStream_t)stream);        // the band, the table and the wrapped map are the context's
    return ftp_dft_launch(*c, 2, d_img_obj, ch_obj, d_img_ref, ch_ref, h, w, fmin, fmax, unwrap, tau, d_out, (hipStream_t)stream);
}

// one image (include/ssamd_ftp_mapping.h): the checks of the pair with the one channel count twice
int ssamd_ftp_carrier_phase(const uint8_t *img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau,
                            double *out, int device)
{
    if (!img || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch, ch, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    const size_t px = (size_t)h * w;
    return host_route(device, {{&Ctx::imgL, img, px * ch}}, {&Ctx::uwOut, out, px * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        return ftp_dft_launch(c, 1, (const uint8_t *)c.imgL.ptr, ch, nullptr, 0, h, w, fmin, fmax, unwrap, tau, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_ftp_carrier_phase_device(const uint8_t *d_img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap,
                                   double tau, double *d_out, void *stream)
{
    if (!d_img || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch, ch, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    ScratchOrder order(*c, (hipStream_t)stream);        // the band, the table and the wrapped map are the context's
    return ftp_dft_launch(*c, 1, d_img, ch, nullptr, 0, h, w, fmin, fmax, unwrap, tau, d_out, (hipStream_t)stream);
}
}  // extern "C"
