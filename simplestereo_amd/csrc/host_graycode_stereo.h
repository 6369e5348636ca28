// Host section of ssamd_api.hip: Gray-code active stereo with two cameras (graycode_stereo_kernels.hip.h,
// include/ssamd_graycode_stereo.h) -- checks, launches, entry points.  The decode, the scan and the staging of a plane stack are
// those of host_graycode.h.
namespace {
static_assert(SSAMD_STEREO_LAST == STEREO_LAST && SSAMD_STEREO_MEAN == STEREO_MEAN, "reduce modes of ssamd_graycode_stereo.h");
static_assert(SSAMD_GRAYCODE_STEREO_SCRATCH(1000, SSAMD_STEREO_MEAN) == 40000 && SSAMD_GRAYCODE_STEREO_SCRATCH(3, SSAMD_STEREO_LAST) == 32,
              "scratch size of ssamd_graycode_stereo.h");

constexpr long long STEREO_TRI_MAX_POINTS = 1ll << 38;      // 2^28 workgroups of GRAYCODE_BLOCK points: one grid dimension

// one camera's decoded region as the scatter reads it
struct StereoSide {
    const int32_t *decoded;
    long long npix;
    int w, x0, y0;
};

int stereo_side_check(int h, int w, int x0, int y0, StereoSide &S)
{
    int rc = region_check(h, w, x0, y0, S.npix);
    if (rc) return rc;
    if (((long long)y0 + h) * ((long long)x0 + w) >= (1ll << 31))
        return fail(SSAMD_EINVAL, "region %d x %d at (%d, %d): (y0 + h) * (x0 + w) is 2^31 or more", w, h, x0, y0);
    S.w = w; S.x0 = x0; S.y0 = y0;
    return SSAMD_OK;
}

int stereo_projector_check(int pw, int ph, int reduce, long long &cells)
{
    int rc = projector_check(pw, ph);
    if (rc) return rc;
    cells = (long long)pw * ph;
    if (cells >= (1ll << 31)) return fail(SSAMD_EINVAL, "projector of %d x %d pixels: 2^31 or more", pw, ph);
    if (reduce != STEREO_LAST && reduce != STEREO_MEAN) return fail(SSAMD_EINVAL, "reduce must be SSAMD_STEREO_LAST or SSAMD_STEREO_MEAN");
    return SSAMD_OK;
}

int stereo_match_check(int h1, int w1, int x1, int y1, int h2, int w2, int x2, int y2, int pw, int ph, int reduce, StereoSide (&S)[2], long long &cells)
{
    int rc = stereo_side_check(h1, w1, x1, y1, S[0]);
    if (rc || (rc = stereo_side_check(h2, w2, x2, y2, S[1]))) return rc;
    return stereo_projector_check(pw, ph, reduce, cells);
}

// the entries of the FTP cloud geometry the two-camera triangulation reads
int stereo_geom_check(const double *geom, FtpCloudGeom &G)
{
    int model;
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    return ftp_load_geom(geom, {{40, SSAMD_FTP_CLOUD_NGEOM}}, G, model);
}

int stereo_match_aligned(const StereoSide (&S)[2], const void *matches, const void *counts, const void *scratch)
{
    if (((uintptr_t)S[0].decoded | (uintptr_t)S[1].decoded | (uintptr_t)matches) & 15)
        return fail(SSAMD_EINVAL, "the decoded buffers and the matches must be 16-byte aligned");
    if (((uintptr_t)scratch & 7) || ((uintptr_t)counts & 3)) return fail(SSAMD_EINVAL, "the scratch must be 8-byte and counts 4-byte aligned");
    return SSAMD_OK;
}

StereoTable stereo_table(char *base, long long cells, int stride)
{
    StereoTable T;
    T.key = (int32_t *)base;
    T.sx = (unsigned long long *)base;
    T.sy = T.sx + cells;
    T.cnt = (uint32_t *)(T.sy + cells);
    T.stride = stride > 0 ? stride : 1;
    return T;
}

// clear both tables, scatter each camera into its own, match: all on s, ordered by the kernel boundaries
int stereo_match_launch(Ctx &c, const StereoSide (&S)[2], int pw, int ph, long long cells, int reduce, double *d_matches, int32_t *d_counts,
                        void *d_scratch, hipStream_t s)
{
    int rc = stereo_match_aligned(S, d_matches, d_counts, d_scratch);
    if (rc) return rc;
    const size_t bytes = stereo_table_bytes(cells, reduce);
    StereoTable T[2];
    for (int i = 0; i < 2; ++i) T[i] = stereo_table((char *)d_scratch + i * bytes, cells, S[i].x0 + S[i].w);
    {   // (profile slots: the clearing and the scatters together in the decode's, the match in the remap's -- tools/time_graycode_stereo.py
        //  separates the scatters by leaving a camera's region empty)
        Timed t(c, s, SSAMD_K_FTP);
        HIP_TRY(hipMemsetAsync(d_scratch, reduce == STEREO_LAST ? 0xff : 0, 2 * bytes, s));
        for (int i = 0; i < 2; ++i) {
            if (S[i].npix == 0) continue;
            hipLaunchKernelGGL(reduce == STEREO_LAST ? graycode_scatter_kernel<STEREO_LAST> : graycode_scatter_kernel<STEREO_MEAN>, dim3(gray_blocks(S[i].npix)),
                               dim3(GRAYCODE_THREADS), 0, s, S[i].decoded, S[i].npix, S[i].w, S[i].x0, S[i].y0, pw, ph, T[i]);
            HIP_TRY(hipGetLastError());
        }
    }
    Timed t(c, s, SSAMD_K_REMAP);
    hipLaunchKernelGGL(reduce == STEREO_LAST ? graycode_match_kernel<STEREO_LAST> : graycode_match_kernel<STEREO_MEAN>, dim3(gray_blocks(cells)),
                       dim3(GRAYCODE_THREADS), 0, s, T[0], T[1], cells, d_matches, d_counts);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int stereo_cloud_aligned(const void *a, const void *b, const void *offsets, const void *out, bool pairs)
{
    if (!pairs && ((uintptr_t)a & 15)) return fail(SSAMD_EINVAL, "the matches must be 16-byte aligned");
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 7) || ((uintptr_t)offsets & 3))
        return fail(SSAMD_EINVAL, "point buffers must be 8-byte and offsets 4-byte aligned");
    return SSAMD_OK;
}

// matches [n][4] (b == nullptr) or the pairs a, b [n][2] -> points
int stereo_cloud_launch(Ctx &c, const double *d_a, const double *d_b, bool pairs, long long n, const FtpCloudGeom &G, const int32_t *d_offsets,
                        double *d_out, hipStream_t s)
{
    int rc = stereo_cloud_aligned(d_a, d_b, d_offsets, d_out, pairs);
    if (rc) return rc;
    const long long nblocks = (n + GRAYCODE_BLOCK - 1) / GRAYCODE_BLOCK;
    Timed t(c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(pairs ? graycode_stereo_cloud_kernel<true> : graycode_stereo_cloud_kernel<false>, dim3((unsigned)nblocks), dim3(GRAYCODE_THREADS), 0, s,
                       d_a, d_b, d_offsets, d_out, n, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// uwOut of the host forms: matches, counts, offsets, the tables, the points and both decoded maps
struct StereoStaging {
    size_t matches, counts, offsets, scratch, points, decoded[2], end;
    StereoStaging(long long cells, int reduce, long long npix1, long long npix2)
    {
        const size_t nblocks = (size_t)gray_blocks(cells);
        matches = 0;
        counts = gray_round((size_t)cells * 4 * sizeof(double));
        offsets = counts + gray_round(nblocks * sizeof(int32_t));
        scratch = offsets + gray_round((nblocks + 1) * sizeof(int32_t));
        points = scratch + gray_round(2 * stereo_table_bytes(cells, reduce));
        decoded[0] = points + gray_round((size_t)cells * 3 * sizeof(double));
        decoded[1] = decoded[0] + gray_round((size_t)npix1 * 2 * sizeof(int32_t) + 1);
        end = decoded[1] + gray_round((size_t)npix2 * 2 * sizeof(int32_t) + 1);
    }
};
}  // namespace

extern "C" {
int ssamd_graycode_stereo_match(const int32_t *decoded1, int h1, int w1, int x1, int y1, const int32_t *decoded2, int h2, int w2, int x2, int y2,
                                int proj_w, int proj_h, int reduce, double *matches, int32_t *counts, int device)
{
    StereoSide S[2];
    long long cells;
    int rc = stereo_match_check(h1, w1, x1, y1, h2, w2, x2, y2, proj_w, proj_h, reduce, S, cells);
    if (rc) return rc;
    if (!matches || (!decoded1 && S[0].npix) || (!decoded2 && S[1].npix)) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t bytes1 = (size_t)S[0].npix * 2 * sizeof(int32_t), bytes2 = (size_t)S[1].npix * 2 * sizeof(int32_t), at2 = gray_round(bytes1 + 1);
    const StereoStaging at(cells, reduce, 0, 0);
    return host_route(device, {{&Ctx::uwIn, bytes1 ? (const void *)decoded1 : &at, bytes1, 0}, {&Ctx::uwIn, bytes2 ? (const void *)decoded2 : &at, bytes2, at2}},
                      {&Ctx::uwOut, matches, (size_t)cells * 4 * sizeof(double), at.matches}, [&](Ctx &c, hipStream_t s) {
        int r = c.uwOut.reserve(at.points);
        if (r) return r;
        S[0].decoded = (const int32_t *)staged(c, &Ctx::uwIn, 0);
        S[1].decoded = (const int32_t *)staged(c, &Ctx::uwIn, at2);
        int32_t *const d_counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts);
        if ((r = stereo_match_launch(c, S, proj_w, proj_h, cells, reduce, (double *)staged(c, &Ctx::uwOut, at.matches), d_counts,
                                     staged(c, &Ctx::uwOut, at.scratch), s))) return r;
        if (counts) HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)gray_blocks(cells) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return SSAMD_OK;
    });
}

int ssamd_graycode_stereo_match_device(const int32_t *d_decoded1, int h1, int w1, int x1, int y1, const int32_t *d_decoded2, int h2, int w2,
                                       int x2, int y2, int proj_w, int proj_h, int reduce, double *d_matches, int32_t *d_counts,
                                       void *d_scratch, void *stream)
{
    StereoSide S[2];
    long long cells;
    int rc = stereo_match_check(h1, w1, x1, y1, h2, w2, x2, y2, proj_w, proj_h, reduce, S, cells);
    if (rc) return rc;
    if (!d_matches || !d_scratch || (!d_decoded1 && S[0].npix) || (!d_decoded2 && S[1].npix)) return fail(SSAMD_EINVAL, "NULL buffer");
    S[0].decoded = d_decoded1; S[1].decoded = d_decoded2;
    CtxLock c;
    if ((rc = stereo_match_aligned(S, d_matches, d_counts, d_scratch)) || (rc = get_ctx(-1, c))) return rc;
    return stereo_match_launch(*c, S, proj_w, proj_h, cells, reduce, d_matches, d_counts, d_scratch, (hipStream_t)stream);      // the caller's scratch: nothing to order
}

int ssamd_graycode_stereo_cloud(const double *matches, int proj_w, int proj_h, const double *geom, const int32_t *offsets, double *out, int device)
{
    long long cells;
    FtpCloudGeom G;
    int rc = stereo_projector_check(proj_w, proj_h, STEREO_LAST, cells);
    if (rc || (rc = stereo_geom_check(geom, G))) return rc;
    if (!matches || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const int nblocks = gray_blocks(cells);
    const long long total = offsets ? (long long)offsets[nblocks] : cells;
    if (total < 0 || total > cells) return fail(SSAMD_EINVAL, "offsets[nblocks] = %lld outside 0 .. %lld", total, cells);
    const size_t in_bytes = (size_t)cells * 4 * sizeof(double), off_bytes = offsets ? (size_t)(nblocks + 1) * sizeof(int32_t) : 0, at_off = gray_round(in_bytes);
    // (room for every cell: a block's points are written where the caller's offsets say)
    rc = host_route(device, {{&Ctx::uwIn, matches, in_bytes, 0}, {&Ctx::uwIn, off_bytes ? (const void *)offsets : &G, off_bytes, at_off}},
                    {&Ctx::uwOut, out, (size_t)total * 3 * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        int r = c.uwOut.reserve((size_t)cells * 3 * sizeof(double));
        if (r) return r;
        return stereo_cloud_launch(c, (const double *)staged(c, &Ctx::uwIn), nullptr, false, cells, G, offsets ? (const int32_t *)staged(c, &Ctx::uwIn, at_off) : nullptr,
                                   (double *)staged(c, &Ctx::uwOut), s);
    });
    return rc;
}

int ssamd_graycode_stereo_cloud_device(const double *d_matches, int proj_w, int proj_h, const double *geom, const int32_t *d_offsets,
                                       double *d_out, void *stream)
{
    long long cells;
    FtpCloudGeom G;
    int rc = stereo_projector_check(proj_w, proj_h, STEREO_LAST, cells);
    if (rc || (rc = stereo_geom_check(geom, G))) return rc;
    if (!d_matches || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = stereo_cloud_aligned(d_matches, nullptr, d_offsets, d_out, false)) || (rc = get_ctx(-1, c))) return rc;
    return stereo_cloud_launch(*c, d_matches, nullptr, false, cells, G, d_offsets, d_out, (hipStream_t)stream);
}

int ssamd_stereo_triangulate(const double *points1, const double *points2, long long n, const double *geom, double *out, int device)
{
    FtpCloudGeom G;
    if (n < 0 || n > STEREO_TRI_MAX_POINTS) return fail(SSAMD_EINVAL, "n must be in 0 .. 2^38");
    int rc = stereo_geom_check(geom, G);
    if (rc || n == 0) return rc;
    if (!points1 || !points2 || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), at2 = gray_round(in_bytes);
    return host_route(device, {{&Ctx::uwIn, points1, in_bytes, 0}, {&Ctx::uwIn, points2, in_bytes, at2}}, {&Ctx::uwOut, out, (size_t)n * 3 * sizeof(double)},
                      [&](Ctx &c, hipStream_t s) {
        return stereo_cloud_launch(c, (const double *)staged(c, &Ctx::uwIn), (const double *)staged(c, &Ctx::uwIn, at2), true, n, G, nullptr,
                                   (double *)staged(c, &Ctx::uwOut), s);
    });
}

int ssamd_stereo_triangulate_device(const double *d_points1, const double *d_points2, long long n, const double *geom, double *d_out,
                                    void *stream)
{
    FtpCloudGeom G;
    if (n < 0 || n > STEREO_TRI_MAX_POINTS) return fail(SSAMD_EINVAL, "n must be in 0 .. 2^38");
    int rc = stereo_geom_check(geom, G);
    if (rc || n == 0) return rc;
    if (!d_points1 || !d_points2 || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = stereo_cloud_aligned(d_points1, d_points2, nullptr, d_out, true)) || (rc = get_ctx(-1, c))) return rc;
    return stereo_cloud_launch(*c, d_points1, d_points2, true, n, G, nullptr, d_out, (hipStream_t)stream);
}

int ssamd_graycode_stereo_points(const uint8_t *planes1, int hc1, int wc1, const float *mapx1, const float *mapy1, int x1, int y1, int h1, int w1,
                                 const uint8_t *planes2, int hc2, int wc2, const float *mapx2, const float *mapy2, int x2, int y2, int h2, int w2,
                                 int n, int ncol, int nrow, int proj_w, int proj_h, int white_thr, int reduce, const double *geom, int dense,
                                 double *out, int *npoints, int device)
{
    GrayDecodeArgs A[2];
    StereoSide S[2];
    FtpCloudGeom G;
    long long cells;
    int rc = graycode_decode_check(planes1, n, hc1, wc1, mapx1, mapy1, x1, y1, h1, w1, ncol, nrow, proj_w, proj_h, white_thr, A[0]);
    if (rc || (rc = graycode_decode_check(planes2, n, hc2, wc2, mapx2, mapy2, x2, y2, h2, w2, ncol, nrow, proj_w, proj_h, white_thr, A[1]))) return rc;
    if ((rc = stereo_match_check(h1, w1, x1, y1, h2, w2, x2, y2, proj_w, proj_h, reduce, S, cells)) || (rc = stereo_geom_check(geom, G))) return rc;
    if (!npoints || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    *npoints = 0;
    const PlaneStaging in1(A[0].stack, n), in2(A[1].stack, n, in1.end());
    const StereoStaging at(cells, reduce, S[0].npix, S[1].npix);
    const int nblocks = gray_blocks(cells);
    HostOut result{&Ctx::uwOut, out, (size_t)cells * 3 * sizeof(double), at.points};
    int total = 0;
    rc = host_route(device, {in1.planes, in1.mapx, in1.mapy, in2.planes, in2.mapx, in2.mapy}, result, [&](Ctx &c, hipStream_t s) {
        int r = c.uwOut.reserve(at.end);
        if (r) return r;
        const PlaneStaging *const in[2] = {&in1, &in2};
        for (int i = 0; i < 2; ++i) {
            S[i].decoded = (const int32_t *)staged(c, &Ctx::uwOut, at.decoded[i]);
            if (S[i].npix == 0) continue;
            A[i].stack = in[i]->on_device(c, A[i].stack);
            A[i].out = (int32_t *)staged(c, &Ctx::uwOut, at.decoded[i]);
            A[i].counts = nullptr;
            if ((r = graycode_decode_launch(c, A[i], s))) return r;
        }
        int32_t *const d_counts = (int32_t *)staged(c, &Ctx::uwOut, at.counts), *const d_offsets = (int32_t *)staged(c, &Ctx::uwOut, at.offsets);
        double *const d_matches = (double *)staged(c, &Ctx::uwOut, at.matches);
        if ((r = stereo_match_launch(c, S, proj_w, proj_h, cells, reduce, d_matches, d_counts, staged(c, &Ctx::uwOut, at.scratch), s))) return r;
        if ((r = graycode_scan_launch(c, d_counts, nblocks, d_offsets, s))) return r;
        if ((r = stereo_cloud_launch(c, d_matches, nullptr, false, cells, G, dense ? nullptr : d_offsets, (double *)staged(c, &Ctx::uwOut, at.points), s))) return r;
        HIP_TRY(hipMemcpyAsync(&total, d_offsets + nblocks, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!dense) result.bytes = (size_t)total * 3 * sizeof(double);
        return SSAMD_OK;
    });
    if (rc) return rc;
    *npoints = total;
    return SSAMD_OK;
}
}  // extern "C"
