// Host section of ssamd_api.hip: Gray-code structured light (graycode_kernels.hip.h, include/ssamd_graycode.h) -- checks, launches, entry points.
namespace {
static_assert(SSAMD_GRAYCODE_BLOCK == GRAYCODE_BLOCK, "block size of ssamd_graycode.h");

struct GrayShape {       // what the decode arguments come to once checked
    long long plane, npix;
    int nblocks;
};

int graycode_region_check(int h, int w, int x0, int y0, GrayShape &S)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong region dimensions or origin!");
    S.npix = (long long)h * w;
    if (S.npix >= (1ll << 31)) return fail(SSAMD_EINVAL, "region of %d x %d pixels: 2^31 or more", h, w);
    S.nblocks = (int)((S.npix + GRAYCODE_BLOCK - 1) / GRAYCODE_BLOCK);
    return SSAMD_OK;
}

int graycode_decode_check(const void *planes, int n, int hc, int wc, const void *mapx, const void *mapy, int x0, int y0, int h, int w,
                          int ncol, int nrow, int pw, int ph, int thr, GrayShape &S)
{
    int rc = graycode_region_check(h, w, x0, y0, S);
    if (rc) return rc;
    if (hc < 0 || wc < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    S.plane = (long long)hc * wc;
    if (S.plane >= (1ll << 31)) return fail(SSAMD_EINVAL, "pattern images of %d x %d pixels: 2^31 or more", hc, wc);
    if ((long long)x0 + w > wc || (long long)y0 + h > hc)
        return fail(SSAMD_EINVAL, "region %d x %d at (%d, %d) leaves the pattern images (%d x %d)", w, h, x0, y0, wc, hc);
    if (ncol < 0 || nrow < 0 || ncol > 16 || nrow > 16) return fail(SSAMD_EINVAL, "ncol and nrow must be in 0 .. 16 (%d, %d)", ncol, nrow);
    if (n != 2 * (ncol + nrow)) return fail(SSAMD_EINVAL, "%d pattern images for %d column and %d row bits: must be %d", n, ncol, nrow, 2 * (ncol + nrow));
    if (pw < 1 || ph < 1 || pw > 65536 || ph > 65536) return fail(SSAMD_EINVAL, "projector size %d x %d outside 1 .. 65536", pw, ph);
    if (thr < 0 || thr > 256) return fail(SSAMD_EINVAL, "white_thr must be in 0 .. 256");
    if ((mapx == nullptr) != (mapy == nullptr)) return fail(SSAMD_EINVAL, "mapx and mapy: both or neither");
    if (!planes && n > 0 && S.npix > 0) return fail(SSAMD_EINVAL, "NULL buffer");
    return SSAMD_OK;
}

// the entries of the FTP cloud geometry the triangulation reads (ftp_load_geom, host_ftp_cloud.h)
int graycode_geom_check(const double *geom, FtpCloudGeom &G, int &model)
{
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    return ftp_load_geom(geom, {{12, 37}, {40, SSAMD_FTP_CLOUD_NGEOM}}, G, model);
}

int graycode_decode_launch(Ctx &c, const uint8_t *d_planes, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0, int w,
                           int ncol, int nrow, int pw, int ph, int thr, const GrayShape &S, int32_t *d_out, int32_t *d_counts, hipStream_t s)
{
    if ((uintptr_t)d_out & 15) return fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte aligned");
    if (((uintptr_t)d_counts | (uintptr_t)d_mapx | (uintptr_t)d_mapy) & 3) return fail(SSAMD_EINVAL, "maps and counts must be 4-byte aligned");
    const GrayDecodeArgs A{d_planes, d_mapx, d_mapy, d_out, d_counts, S.plane, S.npix, hc, wc, x0, y0, w, ncol, nrow, pw, ph, thr};
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(d_mapx ? graycode_decode_kernel<true> : graycode_decode_kernel<false>, dim3(S.nblocks), dim3(GRAYCODE_THREADS), 0, s, A);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int graycode_scan_launch(Ctx &c, const int32_t *d_counts, int nblocks, int32_t *d_offsets, hipStream_t s)
{
    if (((uintptr_t)d_counts | (uintptr_t)d_offsets) & 3) return fail(SSAMD_EINVAL, "counts and offsets must be 4-byte aligned");
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(graycode_scan_kernel, dim3(1), dim3(GRAYCODE_THREADS), 0, s, d_counts, d_offsets, nblocks);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int graycode_cloud_launch(Ctx &c, const int32_t *d_decoded, int w, int x0, int y0, const GrayShape &S, const FtpCloudGeom &G, int model,
                          const int32_t *d_offsets, double *d_out, hipStream_t s)
{
    if ((uintptr_t)d_decoded & 15) return fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte aligned");
    if (((uintptr_t)d_out & 7) || ((uintptr_t)d_offsets & 3)) return fail(SSAMD_EINVAL, "points must be 8-byte and offsets 4-byte aligned");
    Timed t(c, s, SSAMD_K_REPROJECT);
    static constexpr decltype(&graycode_cloud_kernel<0>) kernels[4] = {graycode_cloud_kernel<0>, graycode_cloud_kernel<1>,
                                                                       graycode_cloud_kernel<2>, graycode_cloud_kernel<3>};
    hipLaunchKernelGGL(kernels[model & 3], dim3(S.nblocks), dim3(GRAYCODE_THREADS), 0, s, d_decoded, d_offsets, d_out, S.npix, w, x0, y0, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// where the host forms keep things in the context's two staging buffers: planes, mapx, mapy in uwIn; counts, offsets, the decoded
// pixels and the points in uwOut, each at a multiple of 256 bytes
inline size_t gray_round(size_t b) { return (b + 255) & ~(size_t)255; }
struct GrayStaging {
    size_t planes, mapx, mapy;                 // uwIn (planes at 0)
    size_t counts, offsets, decoded, points;   // uwOut (counts at 0)
    GrayStaging(int n, const GrayShape &S)
    {
        planes = 0;
        mapx = gray_round((size_t)n * S.plane + 1);      // (+ 1: the buffer exists even without planes)
        mapy = mapx + gray_round((size_t)S.plane * sizeof(float));
        counts = 0;
        offsets = gray_round((size_t)S.nblocks * sizeof(int32_t));
        decoded = offsets + gray_round(((size_t)S.nblocks + 1) * sizeof(int32_t));
        points = decoded + gray_round((size_t)S.npix * 2 * sizeof(int32_t));
    }
};
}  // namespace

extern "C" {
int ssamd_graycode_decode(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                          int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *out, int32_t *counts, int device)
{
    GrayShape S;
    int rc = graycode_decode_check(planes, n, hc, wc, mapx, mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, S);
    if (rc || S.npix == 0) return rc;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    const GrayStaging at(n, S);
    const size_t plane_bytes = (size_t)n * S.plane, map_bytes = mapx ? (size_t)S.plane * sizeof(float) : 0;      // (an absent input: 0 bytes of any address)
    return host_route(device, {{&Ctx::uwIn, plane_bytes ? (const void *)planes : &at, plane_bytes, at.planes}, {&Ctx::uwIn, map_bytes ? (const void *)mapx : &at, map_bytes, at.mapx},
                       {&Ctx::uwIn, map_bytes ? (const void *)mapy : &at, map_bytes, at.mapy}},
                      {&Ctx::uwOut, out, (size_t)S.npix * 2 * sizeof(int32_t), at.decoded}, [&](Ctx &c, hipStream_t s) {
        int32_t *const d_counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts);
        int r = graycode_decode_launch(c, (const uint8_t *)staged(c, &Ctx::uwIn, at.planes), hc, wc,
                                       mapx ? (const float *)staged(c, &Ctx::uwIn, at.mapx) : nullptr, mapx ? (const float *)staged(c, &Ctx::uwIn, at.mapy) : nullptr,
                                       x0, y0, w, ncol, nrow, proj_w, proj_h, white_thr, S, (int32_t *)staged(c, &Ctx::uwOut, at.decoded), d_counts, s);
        if (r) return r;
        if (counts) HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)S.nblocks * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return SSAMD_OK;
    });
}

int ssamd_graycode_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                 int h, int w, int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *d_out, int32_t *d_counts,
                                 void *stream)
{
    GrayShape S;
    int rc = graycode_decode_check(d_planes, n, hc, wc, d_mapx, d_mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, S);
    if (rc || S.npix == 0) return rc;
    if (!d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return graycode_decode_launch(*c, d_planes, hc, wc, d_mapx, d_mapy, x0, y0, w, ncol, nrow, proj_w, proj_h, white_thr, S, d_out, d_counts,
                                  (hipStream_t)stream);      // no scratch: nothing to order
}

int ssamd_graycode_offsets(const int32_t *counts, int nblocks, int32_t *offsets, int device)
{
    if (nblocks < 0 || nblocks > (1 << 21)) return fail(SSAMD_EINVAL, "nblocks must be in 0 .. 2^21");
    if (!offsets || (!counts && nblocks)) return fail(SSAMD_EINVAL, "NULL buffer");
    if (nblocks == 0) { offsets[0] = 0; return SSAMD_OK; }      // the empty sum
    const size_t bytes = (size_t)nblocks * sizeof(int32_t);
    return host_route(device, {{&Ctx::uwIn, counts, bytes}}, {&Ctx::uwOut, offsets, bytes + sizeof(int32_t)}, [&](Ctx &c, hipStream_t s) {
        return graycode_scan_launch(c, (const int32_t *)c.uwIn.ptr, nblocks, (int32_t *)c.uwOut.ptr, s);
    });
}

int ssamd_graycode_offsets_device(const int32_t *d_counts, int nblocks, int32_t *d_offsets, void *stream)
{
    if (nblocks < 0 || nblocks > (1 << 21)) return fail(SSAMD_EINVAL, "nblocks must be in 0 .. 2^21");
    if (!d_offsets || (!d_counts && nblocks)) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    return graycode_scan_launch(*c, d_counts, nblocks, d_offsets, (hipStream_t)stream);
}

int ssamd_graycode_cloud(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                         int ncol, int nrow, int proj_w, int proj_h, int white_thr, const double *geom, int dense, double *out, int *npoints,
                         int device)
{
    GrayShape S;
    FtpCloudGeom G;
    int model;
    int rc = graycode_decode_check(planes, n, hc, wc, mapx, mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, S);
    if (rc || (rc = graycode_geom_check(geom, G, model))) return rc;
    if (!npoints) return fail(SSAMD_EINVAL, "NULL buffer");
    *npoints = 0;
    if (S.npix == 0) return SSAMD_OK;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    const GrayStaging at(n, S);
    const size_t plane_bytes = (size_t)n * S.plane, map_bytes = mapx ? (size_t)S.plane * sizeof(float) : 0;      // (an absent input: 0 bytes of any address)
    // the route reserves room for every pixel and copies down what `result.bytes` says once the launches are queued: the total is
    // known by then, because the compacted form waits for it to size the copy
    HostOut result{&Ctx::uwOut, out, (size_t)S.npix * 3 * sizeof(double), at.points};
    int total = 0;
    rc = host_route(device, {{&Ctx::uwIn, plane_bytes ? (const void *)planes : &at, plane_bytes, at.planes}, {&Ctx::uwIn, map_bytes ? (const void *)mapx : &at, map_bytes, at.mapx},
                       {&Ctx::uwIn, map_bytes ? (const void *)mapy : &at, map_bytes, at.mapy}},
                    result, [&](Ctx &c, hipStream_t s) {
        int32_t *const d_counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts), *const d_offsets = (int32_t *)staged(c, &Ctx::uwOut, at.offsets);
        int32_t *const d_decoded = (int32_t *)staged(c, &Ctx::uwOut, at.decoded);
        int r = graycode_decode_launch(c, (const uint8_t *)staged(c, &Ctx::uwIn, at.planes), hc, wc,
                                       mapx ? (const float *)staged(c, &Ctx::uwIn, at.mapx) : nullptr, mapx ? (const float *)staged(c, &Ctx::uwIn, at.mapy) : nullptr,
                                       x0, y0, w, ncol, nrow, proj_w, proj_h, white_thr, S, d_decoded, d_counts, s);
        if (r || (r = graycode_scan_launch(c, d_counts, S.nblocks, d_offsets, s))) return r;
        if ((r = graycode_cloud_launch(c, d_decoded, w, x0, y0, S, G, model, dense ? nullptr : d_offsets, (double *)staged(c, &Ctx::uwOut, at.points), s))) return r;
        HIP_TRY(hipMemcpyAsync(&total, d_offsets + S.nblocks, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!dense) result.bytes = (size_t)total * 3 * sizeof(double);
        return SSAMD_OK;
    });
    if (rc) return rc;
    *npoints = total;
    return SSAMD_OK;
}

int ssamd_graycode_cloud_device(const int32_t *d_decoded, int h, int w, int x0, int y0, const double *geom, const int32_t *d_offsets,
                                double *d_out, void *stream)
{
    GrayShape S;
    FtpCloudGeom G;
    int model;
    int rc = graycode_region_check(h, w, x0, y0, S);
    if (rc || (rc = graycode_geom_check(geom, G, model))) return rc;
    if (S.npix == 0) return SSAMD_OK;
    if (!d_decoded || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return graycode_cloud_launch(*c, d_decoded, w, x0, y0, S, G, model, d_offsets, d_out, (hipStream_t)stream);
}
}  // extern "C"
