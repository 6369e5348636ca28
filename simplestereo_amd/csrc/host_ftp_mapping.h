// Host section of ssamd_api.hip: FTP without a reference plane (ftp_carrier_kernel of ftp_kernels.hip.h, ftp_mapping_kernels.hip.h,
// include/ssamd_ftp_mapping.h) -- checks, launches, entry points.
namespace {
// one image through the band staging and the table of ftp_launch (host_ftp_phase.h), then the same unwrapping tail
int ftp_carrier_launch(Ctx &c, const uint8_t *d_img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau,
                       double *d_out, hipStream_t s)
{
    int rc, max_bins;
    const double2 *tw = nullptr;
    if ((rc = ftp_stage_bands(c, h, w, fmin, fmax, s, max_bins, &tw))) return rc;
    double *d_phase = d_out;
    if (unwrap == 1) {                                   // the wavefront kernel does not work in place
        if ((rc = c.ftpPhase.reserve((size_t)h * w * sizeof(double)))) return rc;
        d_phase = (double *)c.ftpPhase.ptr;
    }
    const FtpGeom g = ftp_carrier_geometry(w);
    const int q = ftp_lanes_per_bin(g.threads, std::max(max_bins, 1));
    auto launch = [&](auto kernel) -> int {
        int r = grant_dyn_lds(c, reinterpret_cast<const void *>(kernel), g.lds_bytes);
        if (r) return r;
        Timed t(c, s, SSAMD_K_FTP);
        hipLaunchKernelGGL(kernel, dim3(h), dim3(g.threads), g.lds_bytes, s, d_img, ch, w, (const int2 *)c.ftpBand.ptr, tw, q, FTP_BIN_CHUNK,
                           d_phase);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    };
    static constexpr decltype(&ftp_carrier_kernel<1>) kernels[4] = {ftp_carrier_kernel<1>, ftp_carrier_kernel<2>, ftp_carrier_kernel<4>,
                                                                    ftp_carrier_kernel<8>};
    if ((rc = launch(kernels[g.cpt == 1 ? 0 : g.cpt == 2 ? 1 : g.cpt == 4 ? 2 : 3]))) return rc;      // by columns per thread
    return ftp_unwrap_tail(c, unwrap, tau, d_phase, h, w, d_out, s);
}

// the checks shared by the host and the device form of ssamd_ftp_mapping_cloud; fills the by-value arguments.  Of the geometry
// the entries the triangulation reads ([12..36], [40..67]) and 2 pi fp ([39]); the others stay 0
int ftp_mapping_check(int h, int w, int x0, int y0, const double *geom, const double *F, double theta, double peak, FtpCloudGeom &G,
                      FtpMapArgs &A, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions or origin!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "phase map of %d x %d pixels: 2^31 or more", h, w);
    if (!geom || !F) return fail(SSAMD_EINVAL, "NULL buffer");
    if (!std::isfinite(theta) || !std::isfinite(peak)) return fail(SSAMD_EINVAL, "theta and peak must be finite");
    double g[SSAMD_FTP_CLOUD_NGEOM] = {0};
    for (int i = 12; i < SSAMD_FTP_CLOUD_NGEOM; ++i) {
        if (i == 37 || i == 38) continue;
        if (!std::isfinite(geom[i])) return fail(SSAMD_EINVAL, "geom[%d] is not finite", i);
        g[i] = geom[i];
    }
    std::memcpy(&G, g, sizeof(G));
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(F[i])) return fail(SSAMD_EINVAL, "F[%d] is not finite", i);
        A.F[i] = F[i];
    }
    A.theta = theta;
    A.peak = peak;
    A.two_pi_fp = G.two_pi_fp;
    auto any = [&](int a, int b) { for (int i = a; i < b; ++i) if (G.d[i] != 0) return true; return false; };
    model = any(8, 12) ? 3 : any(5, 8) ? 2 : any(0, 5) ? 1 : 0;
    return SSAMD_OK;
}

int ftp_mapping_launch(Ctx &c, const double *d_phase, int h, int w, int x0, int y0, const FtpCloudGeom &G, const FtpMapArgs &A, int model,
                       double *d_out, hipStream_t s)
{
    if (((uintptr_t)d_phase | (uintptr_t)d_out) & 15) return fail(SSAMD_EINVAL, "phase and point buffers must be 16-byte aligned");
    const long long npix = (long long)h * w, pairs = (npix + 1) / 2;
    const int blocks = (int)std::min<long long>((pairs + FTP_CLOUD_THREADS - 1) / FTP_CLOUD_THREADS, (long long)c.cus * 8);
    Timed t(c, s, SSAMD_K_REPROJECT);
    static constexpr decltype(&ftp_mapping_cloud_kernel<0>) kernels[4] = {ftp_mapping_cloud_kernel<0>, ftp_mapping_cloud_kernel<1>,
                                                                          ftp_mapping_cloud_kernel<2>, ftp_mapping_cloud_kernel<3>};
    hipLaunchKernelGGL(kernels[model & 3], dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, A, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_ftp_carrier_phase(const uint8_t *img, int ch, int h, int w, const double *fmin, const double *fmax, int unwrap, double tau,
                            double *out, int device)
{
    if (!img || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = ftp_check(ch, ch, h, w, fmin, fmax, unwrap, tau);
    if (rc) return rc;
    const size_t px = (size_t)h * w;
    return host_route(device, {{&Ctx::imgL, img, px * ch}}, {&Ctx::uwOut, out, px * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        return ftp_carrier_launch(c, (const uint8_t *)c.imgL.ptr, ch, h, w, fmin, fmax, unwrap, tau, (double *)c.uwOut.ptr, s);
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
    return ftp_carrier_launch(*c, d_img, ch, h, w, fmin, fmax, unwrap, tau, d_out, (hipStream_t)stream);
}

int ssamd_ftp_mapping_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, const double *F, double theta,
                            double peak, double *out, int device)
{
    FtpCloudGeom G;
    FtpMapArgs A;
    int model;
    int rc = ftp_mapping_check(h, w, x0, y0, geom, F, theta, peak, G, A, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!phase || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t bytes = (size_t)h * w * sizeof(double);
    return host_route(device, {{&Ctx::uwIn, phase, bytes}}, {&Ctx::uwOut, out, 3 * bytes}, [&](Ctx &c, hipStream_t s) {
        return ftp_mapping_launch(c, (const double *)c.uwIn.ptr, h, w, x0, y0, G, A, model, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_ftp_mapping_cloud_device(const double *d_phase, int h, int w, int x0, int y0, const double *geom, const double *F,
                                   double theta, double peak, double *d_out, void *stream)
{
    FtpCloudGeom G;
    FtpMapArgs A;
    int model;
    int rc = ftp_mapping_check(h, w, x0, y0, geom, F, theta, peak, G, A, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!d_phase || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return ftp_mapping_launch(*c, d_phase, h, w, x0, y0, G, A, model, d_out, (hipStream_t)stream);      // no scratch: nothing to order
}
}  // extern "C"
