// Host section of ssamd_api.hip: FTP cloud (ftp_cloud_kernels.hip.h) -- check, launch, entry points.
namespace {
// FTP phase -> cloud (ftp_cloud_kernels.hip.h): the checks shared by the host and the device entry point; fills the by-value
// geometry, the phase shift of the fringe order and the distortion model the coefficients ask for
static_assert(SSAMD_FTP_CLOUD_NGEOM * sizeof(double) == sizeof(FtpCloudGeom), "geom layout of ssamd.h");
int ftp_cloud_check(int h, int w, int x0, int y0, const double *geom, double k, FtpCloudGeom &G, double &kshift, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions or origin!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "phase map of %d x %d pixels: 2^31 or more", h, w);
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    if (!std::isfinite(k)) return fail(SSAMD_EINVAL, "the fringe order k must be finite");
    for (int i = 0; i < SSAMD_FTP_CLOUD_NGEOM; ++i)
        if (!std::isfinite(geom[i])) return fail(SSAMD_EINVAL, "geom[%d] is not finite", i);
    std::memcpy(&G, geom, sizeof(G));
    kshift = (k * 2.0) * M_PI;                       // active.py:791: k * 2 * np.pi
    auto any = [&](int a, int b) { for (int i = a; i < b; ++i) if (G.d[i] != 0) return true; return false; };
    model = any(8, 12) ? 3 : any(5, 8) ? 2 : any(0, 5) ? 1 : 0;
    return SSAMD_OK;
}

int ftp_cloud_launch(Ctx &c, const double *d_phase, int h, int w, int x0, int y0, const FtpCloudGeom &G, double kshift, int model,
                     double *d_out, hipStream_t s)
{
    if (((uintptr_t)d_phase | (uintptr_t)d_out) & 15) return fail(SSAMD_EINVAL, "phase and point buffers must be 16-byte aligned");
    const long long npix = (long long)h * w, pairs = (npix + 1) / 2;
    const int blocks = (int)std::min<long long>((pairs + FTP_CLOUD_THREADS - 1) / FTP_CLOUD_THREADS, (long long)c.cus * 8);
    Timed t(c, s, SSAMD_K_REPROJECT);
    static constexpr decltype(&ftp_cloud_kernel<0>) kernels[4] = {ftp_cloud_kernel<0>, ftp_cloud_kernel<1>, ftp_cloud_kernel<2>, ftp_cloud_kernel<3>};
    hipLaunchKernelGGL(kernels[model & 3], dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, kshift, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_ftp_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, double k, double *out, int device)
{
    FtpCloudGeom G;
    double kshift;
    int model;
    int rc = ftp_cloud_check(h, w, x0, y0, geom, k, G, kshift, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!phase || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t bytes = (size_t)h * w * sizeof(double);
    return host_route(device, {{&Ctx::uwIn, phase, bytes}}, {&Ctx::uwOut, out, 3 * bytes}, [&](Ctx &c, hipStream_t s) {
        return ftp_cloud_launch(c, (const double *)c.uwIn.ptr, h, w, x0, y0, G, kshift, model, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_ftp_cloud_device(const double *d_phase, int h, int w, int x0, int y0, const double *geom, double k, double *d_out, void *stream)
{
    FtpCloudGeom G;
    double kshift;
    int model;
    int rc = ftp_cloud_check(h, w, x0, y0, geom, k, G, kshift, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!d_phase || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return ftp_cloud_launch(*c, d_phase, h, w, x0, y0, G, kshift, model, d_out, (hipStream_t)stream);      // no scratch: nothing to order
}
}  // extern "C"
