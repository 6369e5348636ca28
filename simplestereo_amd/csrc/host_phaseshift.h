// Host section of ssamd_api.hip: phase-shift decode and the triangulation of correspondences (phaseshift_kernels.hip.h,
// include/ssamd_structured_light.h) -- checks, launches, entry points.
namespace {
static_assert(SSAMD_SL_MAX_PERIODS == SL_MAX_PERIODS, "period limit of ssamd_structured_light.h");

// the decode arguments once checked: everything of PhaseShiftArgs but the four device pointers
int phaseshift_check(const void *planes, int n, int hc, int wc, const void *mapx, const void *mapy, int x0, int y0, int h, int w, int nx, int ny,
                     const double *periods_x, const double *periods_y, int pw, int ph, int thr2, PhaseShiftArgs &A)
{
    GrayShape S;
    int rc = graycode_region_check(h, w, x0, y0, S);
    if (rc) return rc;
    if (hc < 0 || wc < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    S.plane = (long long)hc * wc;
    if (S.plane >= (1ll << 31)) return fail(SSAMD_EINVAL, "pattern images of %d x %d pixels: 2^31 or more", hc, wc);
    if ((long long)x0 + w > wc || (long long)y0 + h > hc)
        return fail(SSAMD_EINVAL, "region %d x %d at (%d, %d) leaves the pattern images (%d x %d)", w, h, x0, y0, wc, hc);
    if (nx < 1 || ny < 1 || nx > SL_MAX_PERIODS || ny > SL_MAX_PERIODS)
        return fail(SSAMD_EINVAL, "nx and ny must be in 1 .. %d (%d, %d)", SL_MAX_PERIODS, nx, ny);
    if (n != 4 * (nx + ny)) return fail(SSAMD_EINVAL, "%d images for %d x-periods and %d y-periods: must be %d", n, nx, ny, 4 * (nx + ny));
    if (pw < 1 || ph < 1 || pw > 65536 || ph > 65536) return fail(SSAMD_EINVAL, "projector size %d x %d outside 1 .. 65536", pw, ph);
    if (thr2 < 0) return fail(SSAMD_EINVAL, "mod_thr2 must not be negative");
    if ((mapx == nullptr) != (mapy == nullptr)) return fail(SSAMD_EINVAL, "mapx and mapy: both or neither");
    if (!periods_x || !periods_y) return fail(SSAMD_EINVAL, "NULL buffer");
    A = PhaseShiftArgs{};
    for (int axis = 0; axis < 2; ++axis)
        for (int k = 0; k < (axis ? ny : nx); ++k) {
            const double T = (axis ? periods_y : periods_x)[k];
            if (!(std::isfinite(T) && T > 0)) return fail(SSAMD_EINVAL, "periods_%c[%d] must be finite and positive", axis ? 'y' : 'x', k);
            A.T[axis][k] = T;
        }
    if (!planes && S.npix > 0) return fail(SSAMD_EINVAL, "NULL buffer");
    A.plane_stride = S.plane; A.npix = S.npix;
    A.hc = hc; A.wc = wc; A.x0 = x0; A.y0 = y0; A.w = w;
    A.n[0] = nx; A.n[1] = ny;
    A.thr2 = thr2;
    A.extent[0] = (double)pw; A.extent[1] = (double)ph;
    return SSAMD_OK;
}

int phaseshift_launch(Ctx &c, PhaseShiftArgs A, const uint8_t *d_planes, const float *d_mapx, const float *d_mapy, double *d_out, hipStream_t s)
{
    A.planes = d_planes; A.mapx = d_mapx; A.mapy = d_mapy; A.out = d_out;
    const int nblocks = (int)((A.npix + GRAYCODE_BLOCK - 1) / GRAYCODE_BLOCK);
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(d_mapx ? phaseshift_decode_kernel<true> : phaseshift_decode_kernel<false>, dim3(nblocks), dim3(GRAYCODE_THREADS), 0, s, A);
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

int sl_triangulate_launch(Ctx &c, const double *d_cam, const double *d_proj, long long n, int w, int x0, int y0, const FtpCloudGeom &G, int model,
                          double *d_out, hipStream_t s)
{
    const long long nblocks = (n + SL_TRI_THREADS - 1) / SL_TRI_THREADS;
    Timed t(c, s, SSAMD_K_REPROJECT);
    static constexpr decltype(&sl_triangulate_kernel<0>) kernels[4] = {sl_triangulate_kernel<0>, sl_triangulate_kernel<1>,
                                                                       sl_triangulate_kernel<2>, sl_triangulate_kernel<3>};
    hipLaunchKernelGGL(kernels[model & 3], dim3((unsigned)nblocks), dim3(SL_TRI_THREADS), 0, s, d_cam, d_proj, d_out, n, w, x0, y0, G);
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
    if (rc || A.npix == 0) return rc;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    // planes, mapx, mapy in uwIn, each at a multiple of 256 bytes; the result alone in uwOut
    const size_t plane_bytes = (size_t)n * A.plane_stride, map_bytes = mapx ? (size_t)A.plane_stride * sizeof(float) : 0;
    const size_t at_mapx = gray_round(plane_bytes), at_mapy = at_mapx + gray_round(map_bytes);
    return host_route(device, {{&Ctx::uwIn, planes, plane_bytes, 0}, {&Ctx::uwIn, map_bytes ? (const void *)mapx : &A, map_bytes, at_mapx},
                       {&Ctx::uwIn, map_bytes ? (const void *)mapy : &A, map_bytes, at_mapy}},      // (an absent input: 0 bytes of any address)
                      {&Ctx::uwOut, out, (size_t)A.npix * 2 * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        return phaseshift_launch(c, A, (const uint8_t *)staged(c, &Ctx::uwIn), mapx ? (const float *)staged(c, &Ctx::uwIn, at_mapx) : nullptr,
                                 mapx ? (const float *)staged(c, &Ctx::uwIn, at_mapy) : nullptr, (double *)staged(c, &Ctx::uwOut), s);
    });
}

int ssamd_phaseshift_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                   int h, int w, int nx, int ny, const double *periods_x, const double *periods_y, int proj_w, int proj_h,
                                   int mod_thr2, double *d_out, void *stream)
{
    PhaseShiftArgs A;
    int rc = phaseshift_check(d_planes, n, hc, wc, d_mapx, d_mapy, x0, y0, h, w, nx, ny, periods_x, periods_y, proj_w, proj_h, mod_thr2, A);
    if (rc || A.npix == 0) return rc;
    if (!d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    if (((uintptr_t)d_out & 15) || (((uintptr_t)d_mapx | (uintptr_t)d_mapy) & 3))
        return fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte and the maps 4-byte aligned");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return phaseshift_launch(*c, A, d_planes, d_mapx, d_mapy, d_out, (hipStream_t)stream);      // no scratch: nothing to order
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
    if (((uintptr_t)d_cam | (uintptr_t)d_proj | (uintptr_t)d_out) & 7) return fail(SSAMD_EINVAL, "point buffers must be 8-byte aligned");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return sl_triangulate_launch(*c, d_cam, d_proj, n, w, x0, y0, G, model, d_out, (hipStream_t)stream);
}
}  // extern "C"
