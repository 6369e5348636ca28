// Host section of ssamd_api.hip: the per-pixel mapping cloud of FTP without a reference plane (ftp_mapping_kernels.hip.h,
// include/ssamd_ftp_mapping.h) -- check, entry points.  The one-image phase is with the pair's, in host_ftp_phase.h.
namespace {
constexpr decltype(&ftp_mapping_cloud_kernel<0>) FTP_MAPPING_KERNELS[4] = {ftp_mapping_cloud_kernel<0>, ftp_mapping_cloud_kernel<1>,
                                                                           ftp_mapping_cloud_kernel<2>, ftp_mapping_cloud_kernel<3>};

// the checks shared by the host and the device form of ssamd_ftp_mapping_cloud; fills the by-value arguments.  Of the geometry
// the entries the triangulation reads and 2 pi fp ([39])
int ftp_mapping_check(int h, int w, int x0, int y0, const double *geom, const double *F, double theta, double peak, FtpCloudGeom &G,
                      FtpMapArgs &A, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions or origin!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "phase map of %d x %d pixels: 2^31 or more", h, w);
    if (!geom || !F) return fail(SSAMD_EINVAL, "NULL buffer");
    if (!std::isfinite(theta) || !std::isfinite(peak)) return fail(SSAMD_EINVAL, "theta and peak must be finite");
    int rc = ftp_load_geom(geom, {{12, 37}, {39, SSAMD_FTP_CLOUD_NGEOM}}, G, model);
    if (rc) return rc;
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(F[i])) return fail(SSAMD_EINVAL, "F[%d] is not finite", i);
        A.F[i] = F[i];
    }
    A.theta = theta;
    A.peak = peak;
    A.two_pi_fp = G.two_pi_fp;
    return SSAMD_OK;
}
}  // namespace

extern "C" {
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
        return ftp_pointwise_launch(c, FTP_MAPPING_KERNELS, (const double *)c.uwIn.ptr, h, w, x0, y0, A, G, model, (double *)c.uwOut.ptr, s);
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
    return ftp_pointwise_launch(*c, FTP_MAPPING_KERNELS, d_phase, h, w, x0, y0, A, G, model, d_out, (hipStream_t)stream);      // no scratch: nothing to order
}
}  // extern "C"
