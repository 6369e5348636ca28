// Host section of ssamd_api.hip: Gray-code structured light (graycode_kernels.hip.h, include/ssamd_graycode.h) -- checks, launches, entry
// points -- and what it shares with the phase-shift decoder (host_phaseshift.h): the check of a plane stack (plane_stack_check and
// three one-line checks) and its staging for the host entry points (PlaneStaging).
namespace {
static_assert(SSAMD_GRAYCODE_BLOCK == GRAYCODE_BLOCK, "block size of ssamd_graycode.h");

inline int gray_blocks(long long npix) { return (int)((npix + GRAYCODE_BLOCK - 1) / GRAYCODE_BLOCK); }

int region_check(int h, int w, int x0, int y0, long long &npix)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong region dimensions or origin!");
    npix = (long long)h * w;
    if (npix >= (1ll << 31)) return fail(SSAMD_EINVAL, "region of %d x %d pixels: 2^31 or more", h, w);
    return SSAMD_OK;
}

// the region, the images and the region inside the images -> S, with the caller's pointers (of the host or of the device)
int plane_stack_check(const void *planes, int hc, int wc, const void *mapx, const void *mapy, int x0, int y0, int h, int w, PlaneStack &S)
{
    int rc = region_check(h, w, x0, y0, S.npix);
    if (rc) return rc;
    if (hc < 0 || wc < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    S.plane_stride = (long long)hc * wc;
    if (S.plane_stride >= (1ll << 31)) return fail(SSAMD_EINVAL, "pattern images of %d x %d pixels: 2^31 or more", hc, wc);
    if ((long long)x0 + w > wc || (long long)y0 + h > hc)
        return fail(SSAMD_EINVAL, "region %d x %d at (%d, %d) leaves the pattern images (%d x %d)", w, h, x0, y0, wc, hc);
    S.planes = (const uint8_t *)planes; S.mapx = (const float *)mapx; S.mapy = (const float *)mapy;
    S.hc = hc; S.wc = wc; S.x0 = x0; S.y0 = y0; S.w = w;
    return SSAMD_OK;
}

int projector_check(int pw, int ph)
{
    return pw < 1 || ph < 1 || pw > 65536 || ph > 65536 ? fail(SSAMD_EINVAL, "projector size %d x %d outside 1 .. 65536", pw, ph) : SSAMD_OK;
}
int maps_check(const PlaneStack &S) { return (S.mapx == nullptr) != (S.mapy == nullptr) ? fail(SSAMD_EINVAL, "mapx and mapy: both or neither") : SSAMD_OK; }
int planes_check(const PlaneStack &S, int n) { return !S.planes && n > 0 && S.npix > 0 ? fail(SSAMD_EINVAL, "NULL buffer") : SSAMD_OK; }

// the decode arguments once checked: everything of GrayDecodeArgs but `out` and `counts`
int graycode_decode_check(const void *planes, int n, int hc, int wc, const void *mapx, const void *mapy, int x0, int y0, int h, int w,
                          int ncol, int nrow, int pw, int ph, int thr, GrayDecodeArgs &A)
{
    A = GrayDecodeArgs{};
    int rc = plane_stack_check(planes, hc, wc, mapx, mapy, x0, y0, h, w, A.stack);
    if (rc) return rc;
    if (ncol < 0 || nrow < 0 || ncol > 16 || nrow > 16) return fail(SSAMD_EINVAL, "ncol and nrow must be in 0 .. 16 (%d, %d)", ncol, nrow);
    if (n != 2 * (ncol + nrow)) return fail(SSAMD_EINVAL, "%d pattern images for %d column and %d row bits: must be %d", n, ncol, nrow, 2 * (ncol + nrow));
    if ((rc = projector_check(pw, ph))) return rc;
    if (thr < 0 || thr > 256) return fail(SSAMD_EINVAL, "white_thr must be in 0 .. 256");
    if ((rc = maps_check(A.stack)) || (rc = planes_check(A.stack, n))) return rc;
    A.ncol = ncol; A.nrow = nrow; A.pw = pw; A.ph = ph; A.thr = thr;
    return SSAMD_OK;
}

// the entries of the FTP cloud geometry the triangulation reads (ftp_load_geom, host_ftp_cloud.h)
int graycode_geom_check(const double *geom, FtpCloudGeom &G, int &model)
{
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    return ftp_load_geom(geom, {{12, 37}, {40, SSAMD_FTP_CLOUD_NGEOM}}, G, model);
}

int graycode_decode_launch(Ctx &c, const GrayDecodeArgs &A, hipStream_t s)
{
    if ((uintptr_t)A.out & 15) return fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte aligned");
    if (((uintptr_t)A.counts | (uintptr_t)A.stack.mapx | (uintptr_t)A.stack.mapy) & 3) return fail(SSAMD_EINVAL, "maps and counts must be 4-byte aligned");
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(A.stack.mapx ? graycode_decode_kernel<true> : graycode_decode_kernel<false>, dim3(gray_blocks(A.stack.npix)), dim3(GRAYCODE_THREADS), 0, s, A);
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

int graycode_cloud_launch(Ctx &c, const int32_t *d_decoded, long long npix, int w, int x0, int y0, const FtpCloudGeom &G, int model,
                          const int32_t *d_offsets, double *d_out, hipStream_t s)
{
    if ((uintptr_t)d_decoded & 15) return fail(SSAMD_EINVAL, "the decoded buffer must be 16-byte aligned");
    if (((uintptr_t)d_out & 7) || ((uintptr_t)d_offsets & 3)) return fail(SSAMD_EINVAL, "points must be 8-byte and offsets 4-byte aligned");
    Timed t(c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(model_instance(model, [](auto m) { return graycode_cloud_kernel<decltype(m)::value>; }), dim3(gray_blocks(npix)), dim3(GRAYCODE_THREADS),
                       0, s, d_decoded, d_offsets, d_out, npix, w, x0, y0, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// Where the host forms keep things in the context's two staging buffers, each at a multiple of 256 bytes.  uwIn: the planes, mapx
// and mapy of a checked stack S (host pointers); an absent input is 0 bytes of any address, and the buffer exists even without
// planes (+ 1).  on_device: S with the staged pointers, the maps nullptr when absent.  A second stack (host_graycode_stereo.h)
// starts at `base` = the first one's end().
inline size_t gray_round(size_t b) { return (b + 255) & ~(size_t)255; }
struct PlaneStaging {
    HostIn planes, mapx, mapy;
    PlaneStaging(const PlaneStack &S, int n, size_t base = 0)
    {
        const size_t plane_bytes = (size_t)n * S.plane_stride, map_bytes = S.mapx ? (size_t)S.plane_stride * sizeof(float) : 0;
        const size_t at_mapx = base + gray_round(plane_bytes + 1);
        planes = HostIn{&Ctx::uwIn, plane_bytes ? (const void *)S.planes : this, plane_bytes, base};
        mapx = HostIn{&Ctx::uwIn, map_bytes ? (const void *)S.mapx : this, map_bytes, at_mapx};
        mapy = HostIn{&Ctx::uwIn, map_bytes ? (const void *)S.mapy : this, map_bytes, at_mapx + gray_round(map_bytes)};
    }
    size_t end() const { return gray_round(mapy.at + mapy.bytes + 1); }
    PlaneStack on_device(Ctx &c, PlaneStack S) const
    {
        S.planes = (const uint8_t *)staged(c, &Ctx::uwIn, planes.at);
        S.mapx = mapx.bytes ? (const float *)staged(c, &Ctx::uwIn, mapx.at) : nullptr;
        S.mapy = mapy.bytes ? (const float *)staged(c, &Ctx::uwIn, mapy.at) : nullptr;
        return S;
    }
};
// uwOut of the Gray-code host forms: counts, offsets, the decoded pixels and the points
struct GrayStaging {
    size_t counts, offsets, decoded, points;
    explicit GrayStaging(long long npix)
    {
        const size_t nblocks = (size_t)gray_blocks(npix);
        counts = 0;
        offsets = gray_round(nblocks * sizeof(int32_t));
        decoded = offsets + gray_round((nblocks + 1) * sizeof(int32_t));
        points = decoded + gray_round((size_t)npix * 2 * sizeof(int32_t));
    }
};

// the checked decode on the staged inputs of a host form: the decoded pixels and the counts go to their places in uwOut
int graycode_decode_staged(Ctx &c, GrayDecodeArgs A, const PlaneStaging &in, const GrayStaging &at, hipStream_t s)
{
    A.stack = in.on_device(c, A.stack);
    A.out = (int32_t *)staged(c, &Ctx::uwOut, at.decoded);
    A.counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts);
    return graycode_decode_launch(c, A, s);
}
}  // namespace

extern "C" {
int ssamd_graycode_decode(const uint8_t *planes, int n, int hc, int wc, const float *mapx, const float *mapy, int x0, int y0, int h, int w,
                          int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *out, int32_t *counts, int device)
{
    GrayDecodeArgs A;
    int rc = graycode_decode_check(planes, n, hc, wc, mapx, mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, A);
    const long long npix = A.stack.npix;
    if (rc || npix == 0) return rc;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    const PlaneStaging in(A.stack, n);
    const GrayStaging at(npix);
    return host_route(device, {in.planes, in.mapx, in.mapy}, {&Ctx::uwOut, out, (size_t)npix * 2 * sizeof(int32_t), at.decoded}, [&](Ctx &c, hipStream_t s) {
        int r = graycode_decode_staged(c, A, in, at, s);
        if (r) return r;
        if (counts) HIP_TRY(hipMemcpyAsync(counts, staged(c, &Ctx::uwOut, at.counts), (size_t)gray_blocks(npix) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return SSAMD_OK;
    });
}

int ssamd_graycode_decode_device(const uint8_t *d_planes, int n, int hc, int wc, const float *d_mapx, const float *d_mapy, int x0, int y0,
                                 int h, int w, int ncol, int nrow, int proj_w, int proj_h, int white_thr, int32_t *d_out, int32_t *d_counts,
                                 void *stream)
{
    GrayDecodeArgs A;
    int rc = graycode_decode_check(d_planes, n, hc, wc, d_mapx, d_mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, A);
    if (rc || A.stack.npix == 0) return rc;
    if (!d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    A.out = d_out; A.counts = d_counts;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return graycode_decode_launch(*c, A, (hipStream_t)stream);      // no scratch: nothing to order
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
    GrayDecodeArgs A;
    FtpCloudGeom G;
    int model;
    int rc = graycode_decode_check(planes, n, hc, wc, mapx, mapy, x0, y0, h, w, ncol, nrow, proj_w, proj_h, white_thr, A);
    if (rc || (rc = graycode_geom_check(geom, G, model))) return rc;
    if (!npoints) return fail(SSAMD_EINVAL, "NULL buffer");
    *npoints = 0;
    const long long npix = A.stack.npix;
    if (npix == 0) return SSAMD_OK;
    if (!out) return fail(SSAMD_EINVAL, "NULL buffer");
    const PlaneStaging in(A.stack, n);
    const GrayStaging at(npix);
    // the route reserves room for every pixel and copies down what `result.bytes` says once the launches are queued: the total is
    // known by then, because the compacted form waits for it to size the copy
    HostOut result{&Ctx::uwOut, out, (size_t)npix * 3 * sizeof(double), at.points};
    int total = 0;
    rc = host_route(device, {in.planes, in.mapx, in.mapy}, result, [&](Ctx &c, hipStream_t s) {
        int32_t *const d_counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts), *const d_offsets = (int32_t *)staged(c, &Ctx::uwOut, at.offsets);
        int32_t *const d_decoded = (int32_t *)staged(c, &Ctx::uwOut, at.decoded);
        const int nblocks = gray_blocks(npix);
        int r = graycode_decode_staged(c, A, in, at, s);
        if (r || (r = graycode_scan_launch(c, d_counts, nblocks, d_offsets, s))) return r;
        if ((r = graycode_cloud_launch(c, d_decoded, npix, w, x0, y0, G, model, dense ? nullptr : d_offsets, (double *)staged(c, &Ctx::uwOut, at.points), s))) return r;
        HIP_TRY(hipMemcpyAsync(&total, d_offsets + nblocks, sizeof(int32_t), hipMemcpyDeviceToHost, s));
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
    long long npix;
    FtpCloudGeom G;
    int model;
    int rc = region_check(h, w, x0, y0, npix);
    if (rc || (rc = graycode_geom_check(geom, G, model))) return rc;
    if (npix == 0) return SSAMD_OK;
    if (!d_decoded || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return graycode_cloud_launch(*c, d_decoded, npix, w, x0, y0, G, model, d_offsets, d_out, (hipStream_t)stream);
}
}  // extern "C"
