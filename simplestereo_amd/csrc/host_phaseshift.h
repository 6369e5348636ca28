// Host section of ssamd_api.hip: phase-shift decode and the triangulation of correspondences (phaseshift_kernels.hip.h,
// include/ssamd_structured_light.h) -- checks, launches, entry points.  The plane stack is checked and staged by what
// host_graycode.h shares (plane_stack_check, PlaneStaging).
namespace {
static_assert(SSAMD_SL_MAX_PERIODS == SL_MAX_PERIODS, "period limit of ssamd_structured_light.h");

// the decode arguments once checked: everything of PhaseShiftArgs but `out`
int phaseshift_check(const void *planes, int n, int hc, int wc, const void *mapx, const void *mapy, int x0, int y0, int h, int w, int nx, int ny,
                     const double *periods_x, const double *periods_y, int pw, int ph, int thr2, PhaseShiftArgs &A)
{
    A = PhaseShiftArgs{};
    int rc = plane_stack_check(planes, hc, wc, mapx, mapy, x0, y0, h, w, A.stack);
    if (rc) return rc;
    if (nx < 1 || ny < 1 || nx > SL_MAX_PERIODS || ny > SL_MAX_PERIODS)
        return fail(SSAMD_EINVAL, "nx and ny must be in 1 .. %d (%d, %d)", SL_MAX_PERIODS, nx, ny);
    if (n != 4 * (nx + ny)) return fail(SSAMD_EINVAL, "%d images for %d x-periods and %d y-periods: must be %d", n, nx, ny, 4 * (nx + ny));
    if ((rc = projector_check(pw, ph))) return rc;
    if (thr2 < 0) return fail(SSAMD_EINVAL, "mod_thr2 must not be negative");
    if ((rc = maps_check(A.stack))) return rc;
    if (!periods_x || !periods_y) return fail(SSAMD_EINVAL, "NULL buffer");
    for (int axis = 0; axis < 2; ++axis)
        for (int k = 0; k < (axis ? ny : nx); ++k) {
            const double T = (axis ? periods_y : periods_x)[k];
            if (!(std::isfinite(T) && T > 0)) return fail(SSAMD_EINVAL, "periods_%c[%d] must be finite and positive", axis ? 'y' : 'x', k);
            A.T[axis][k] = T;
        }
    if ((rc = planes_check(A.stack, n))) return rc;
    A.n[0] = nx; A.n[1] = ny;
    A.thr2 = thr2;
    A.extent[0] = (double)pw; A.extent[1] = (double)ph;
    return SSAMD_OK;
}

// (the launches check alignment, so both routes do; a _device entry point asks first, to refuse a buffer without looking for a device)
int phaseshift_aligned(const PhaseShiftArgs &A)
{
    return ((uintptr_t)A.out & 15) || (((uintptr_t)A.stack.mapx | (uintptr_t)A.stack.mapy) & 3)
               ? fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte and the maps 4-byte aligned") : SSAMD_OK;
}

int phaseshift_launch(Ctx &c, const PhaseShiftArgs &A, hipStream_t s)
{
    int rc = phaseshift_aligned(A);
    if (rc) return rc;
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(A.stack.mapx ? phaseshift_decode_kernel<true> : phaseshift_decode_kernel<false>, dim3(gray_blocks(A.stack.npix)), dim3(GRAYCODE_THREADS), 0, s, A);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

constexpr long long SL_TRI_MAX_POINTS = 1ll << 38;      // 2^30 workgroups of SL_TRI_THREADS: one grid dimension

int sl_triangulate_check(const void *cam, long long n, int w, int x0, int y0, const double *geom, FtpCloudGeom &G, int &model)
{
    if (n < 0 || n > SL_TRI_MAX_POINTS) return fail(SSAMD_EINVAL, "n must be in 0 .. 2^38");
    if (!cam && (w < 1 || x0 < 0 || y0 < 0)) return fail(SSAMD_EINVAL, "the pixel grid needs w >= 1 and an origin that is not negative");
    return graycode_geom_check(geom, G, model);
}

int sl_triangulate_aligned(const void *cam, const void *proj, const void *out)
{
    return ((uintptr_t)cam | (uintptr_t)proj | (uintptr_t)out) & 7 ? fail(SSAMD_EINVAL, "point buffers must be 8-byte aligned") : SSAMD_OK;
}

int sl_triangulate_launch(Ctx &c, const double *d_cam, const double *d_proj, long long n, int w, int x0, int y0, const FtpCloudGeom &G, int model,
                          double *d_out, hipStream_t s)
{
    int rc = sl_triangulate_aligned(d_cam, d_proj, d_out);
    if (rc) return rc;
    const long long nblocks = (n + SL_TRI_THREADS - 1) / SL_TRI_THREADS;
    Timed t(c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(model_instance(model, [](auto m) { return sl_triangulate_kernel<decltype(m)::value>; }), dim3((unsigned)nblocks), dim3(SL_TRI_THREADS),
                       0, s, d_cam, d_proj, d_out, n, w, x0, y0, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_phaseshift_decode(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                            int nx, int ny, const double *periods_x, const double *periods_y, int proj_w, int proj_h, int mod_thr2,
                            double *out, int device)
{
    PhaseShiftArgs A;
    int rc = phaseshift_check(planes, n, hc, wc, mapx, mapy, x0, y0, h, w, nx, ny, periods_x, periods_y, proj_w, proj_h, mod_thr2, A);
    if (rc || A.stack.npix == 0) return rc;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    const PlaneStaging in(A.stack, n);      // the result alone in uwOut
    return host_route(device, {in.planes, in.mapx, in.mapy}, {&Ctx::uwOut, out, (size_t)A.stack.npix * 2 * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        PhaseShiftArgs D = A;
        D.stack = in.on_device(c, A.stack);
        D.out = (double *)staged(c, &Ctx::uwOut);
        return phaseshift_launch(c, D, s);
    });
}

int ssamd_phaseshift_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                   int h, int w, int nx, int ny, const double *periods_x, const double *periods_y, int proj_w, int proj_h,
                                   int mod_thr2, double *d_out, void *stream)
{
    PhaseShiftArgs A;
    int rc = phaseshift_check(d_planes, n, hc, wc, d_mapx, d_mapy, x0, y0, h, w, nx, ny, periods_x, periods_y, proj_w, proj_h, mod_thr2, A);
    if (rc || A.stack.npix == 0) return rc;
    if (!d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    A.out = d_out;
    CtxLock c;
    if ((rc = phaseshift_aligned(A)) || (rc = get_ctx(-1, c))) return rc;
    return phaseshift_launch(*c, A, (hipStream_t)stream);      // no scratch: nothing to order
}

int ssamd_sl_triangulate(const double *cam, const double *proj, long long n, int w, int x0, int y0, const double *geom, double *out, int device)
{
    FtpCloudGeom G;
    int model;
    int rc = sl_triangulate_check(cam, n, w, x0, y0, geom, G, model);
    if (rc || n == 0) return rc;
    if (!proj || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), cam_bytes = cam ? in_bytes : 0, at_cam = gray_round(in_bytes);
    return host_route(device, {{&Ctx::uwIn, proj, in_bytes, 0}, {&Ctx::uwIn, cam_bytes ? (const void *)cam : &G, cam_bytes, at_cam}},
                      {&Ctx::uwOut, out, (size_t)n * 3 * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        return sl_triangulate_launch(c, cam ? (const double *)staged(c, &Ctx::uwIn, at_cam) : nullptr, (const double *)staged(c, &Ctx::uwIn), n, w, x0, y0,
                                     G, model, (double *)staged(c, &Ctx::uwOut), s);
    });
}

int ssamd_sl_triangulate_device(const double *d_cam, const double *d_proj, long long n, int w, int x0, int y0, const double *geom,
                                double *d_out, void *stream)
{
    FtpCloudGeom G;
    int model;
    int rc = sl_triangulate_check(d_cam, n, w, x0, y0, geom, G, model);
    if (rc || n == 0) return rc;
    if (!d_proj || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = sl_triangulate_aligned(d_cam, d_proj, d_out)) || (rc = get_ctx(-1, c))) return rc;
    return sl_triangulate_launch(*c, d_cam, d_proj, n, w, x0, y0, G, model, d_out, (hipStream_t)stream);
}
}  // extern "C"
