// Host section of ssamd_api.hip: FTP cloud (ftp_cloud_kernels.hip.h) -- the geometry loader and the pointwise launch that the
// mapping cloud (host_ftp_mapping.h) and, for the loader, Gray code (host_graycode.h) share; check, entry points.
namespace {
static_assert(SSAMD_FTP_CLOUD_NGEOM * sizeof(double) == sizeof(FtpCloudGeom), "geom layout of ssamd.h");

// The by-value geometry of a cloud kernel from the flat `geom` of the C ABI.  Of its SSAMD_FTP_CLOUD_NGEOM doubles the entries of the
// index ranges [from, to), given in rising order, must be finite and are copied; the others are not read and stay 0.  model: the
// distortion model the coefficients ask for (ftp_cloud_kernels.hip.h).
struct GeomRange { int from, to; };
int ftp_load_geom(const double *geom, std::initializer_list<GeomRange> ranges, FtpCloudGeom &G, int &model)
{
    double g[SSAMD_FTP_CLOUD_NGEOM] = {0};
    for (const GeomRange &r : ranges)
        for (int i = r.from; i < r.to; ++i) {
            if (!std::isfinite(geom[i])) return fail(SSAMD_EINVAL, "geom[%d] is not finite", i);
            g[i] = geom[i];
        }
    std::memcpy(&G, g, sizeof(G));
    auto any = [&](int a, int b) { for (int i = a; i < b; ++i) if (G.d[i] != 0) return true; return false; };
    model = any(8, 12) ? 3 : any(5, 8) ? 2 : any(0, 5) ? 1 : 0;
    return SSAMD_OK;
}

// The launch of a kernel in ftp_cloud_frame, kernels[model](d_phase, d_out, npix, w, x0, y0, extra, G): a thread per pixel pair,
// at most eight workgroups per compute unit.
template <class Kernel, class Extra>
int ftp_pointwise_launch(Ctx &c, const Kernel (&kernels)[4], const double *d_phase, int h, int w, int x0, int y0, const Extra &extra,
                         const FtpCloudGeom &G, int model, double *d_out, hipStream_t s)
{
    if (((uintptr_t)d_phase | (uintptr_t)d_out) & 15) return fail(SSAMD_EINVAL, "phase and point buffers must be 16-byte aligned");
    const long long npix = (long long)h * w, pairs = (npix + 1) / 2;
    const int blocks = (int)std::min<long long>((pairs + FTP_CLOUD_THREADS - 1) / FTP_CLOUD_THREADS, (long long)c.cus * 8);
    Timed t(c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(kernels[model & 3], dim3(blocks), dim3(FTP_CLOUD_THREADS), 0, s, d_phase, d_out, npix, w, x0, y0, extra, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// The instance of a kernel template for a distortion model 0 .. 3, where one launch names it:
//   model_instance(model, [](auto m) { return kernel<decltype(m)::value>; })
template <class Of>
auto model_instance(int model, Of of) -> decltype(of(std::integral_constant<int, 0>()))
{
    switch (model & 3) {
    case 0: return of(std::integral_constant<int, 0>());
    case 1: return of(std::integral_constant<int, 1>());
    case 2: return of(std::integral_constant<int, 2>());
    default: return of(std::integral_constant<int, 3>());
    }
}

constexpr decltype(&ftp_cloud_kernel<0>) FTP_CLOUD_KERNELS[4] = {ftp_cloud_kernel<0>, ftp_cloud_kernel<1>, ftp_cloud_kernel<2>, ftp_cloud_kernel<3>};

// FTP phase -> cloud: the checks shared by the host and the device entry point; fills the by-value geometry (all of it is read), the
// phase shift of the fringe order and the distortion model
int ftp_cloud_check(int h, int w, int x0, int y0, const double *geom, double k, FtpCloudGeom &G, double &kshift, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions or origin!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "phase map of %d x %d pixels: 2^31 or more", h, w);
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    if (!std::isfinite(k)) return fail(SSAMD_EINVAL, "the fringe order k must be finite");
    kshift = (k * 2.0) * M_PI;                       // active.py:791: k * 2 * np.pi
    return ftp_load_geom(geom, {{0, SSAMD_FTP_CLOUD_NGEOM}}, G, model);
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
        return ftp_pointwise_launch(c, FTP_CLOUD_KERNELS, (const double *)c.uwIn.ptr, h, w, x0, y0, kshift, G, model, (double *)c.uwOut.ptr, s);
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
    return ftp_pointwise_launch(*c, FTP_CLOUD_KERNELS, d_phase, h, w, x0, y0, kshift, G, model, d_out, (hipStream_t)stream);      // no scratch: nothing to order
}
}  // extern "C"
