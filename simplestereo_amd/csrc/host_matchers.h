// Host section of ssamd_api.hip: the matcher ABI -- HostJob / host_rows / run_strips, shared checks, every ssamd_asw* / ssamd_gsw* entry point.
namespace {
// ---- host-buffer paths: H2D copy of rows [in0, in1) of both images, kernels on output rows [o0, o1), D2H copy.
// Used for the whole image (ssamd_asw / ssamd_gsw) and, one host thread per device, for the row strips of
// ssamd_*_multi: output row y needs input rows y-pad .. y+pad only and the left-right check and occlusion filling
// are row-local (_passive.cpp:38-40, 60-62, 251-285), so a strip that carries its halo reproduces the rows of the
// whole-image result bit for bit.
struct HostJob {
    const uint8_t *img1 = nullptr, *img2 = nullptr;      // the two host images, whole
    int16_t *disparity = nullptr;  // full-image outputs: [H][W],
    float *costs = nullptr;        // ... the cost dump (ssamd_asw_costs),
    int16_t *raw_right = nullptr;  // ... the raw right-referenced matches (verification dump of ssamd_asw_argmins / ssamd_gsw_argmins)
    int o0 = 0, o1 = 0;            // output rows of the full image
    bool is_gsw = false;           // which of the two holds the parameters: H x W the whole image, no buffers, rows or stream
    AswCall asw;
    GswCall gsw;
    HostJob(const uint8_t *a, const uint8_t *b, int16_t *d, const AswCall &q) : img1(a), img2(b), disparity(d), o1(q.H), asw(q) {}
    HostJob(const uint8_t *a, const uint8_t *b, int16_t *d, const GswCall &q) : img1(a), img2(b), disparity(d), o1(q.H), is_gsw(true), gsw(q) {}
};

// (Not host_route, host_context.h: two of the three outputs are optional, the cost dump is preset by a memset, and the copies
// address rows [in0, in1) / [o0, o1) of buffers that hold the whole image.)
int host_rows(const HostJob &j, int device)
{
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    AswCall a = j.asw;
    GswCall g = j.gsw;
    MatchCall &q = j.is_gsw ? static_cast<MatchCall &>(g) : a;          // the job's parameters, rebased to the strip's rows below
    const int H = q.H, W = q.W;
    if ((rc = check_common(H, W, q.win, q.minD, q.maxD, j.o0, j.o1 - j.o0))) return rc;
    const bool alternate = !j.is_gsw && a.alternate;
    const int p = q.win / 2 + (alternate ? 1 : 0);        // alternate rows: + the exact row beyond an odd first / last row
    const int in0 = std::max(0, j.o0 - p), in1 = std::min(H, j.o1 + p), rows = j.o1 - j.o0;
    const size_t nb = (size_t)(in1 - in0) * W * 3, nout = (size_t)rows * W;
    if ((rc = c->imgL.reserve(nb)) || (rc = c->imgR.reserve(nb)) || (rc = c->disp.reserve(nout * 2))) return rc;
    const size_t ncost = j.costs ? nout * (size_t)std::max(1, q.maxD - q.minD + 1) : 0;
    if (j.costs && (rc = c->costs.reserve(ncost * 4))) return rc;
    if (j.raw_right && (rc = c->lab.reserve(nout * 2))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, j.img1 + (size_t)in0 * W * 3, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->imgR.ptr, j.img2 + (size_t)in0 * W * 3, nb, hipMemcpyHostToDevice, s));
    if (j.costs) HIP_TRY(hipMemsetAsync(c->costs.ptr, 0xFF, ncost * 4, s));      // 0xFFFFFFFF = NaN
    q.dL = (const uint8_t *)c->imgL.ptr; q.dR = (const uint8_t *)c->imgR.ptr;
    q.H = in1 - in0; q.row0 = j.o0 - in0; q.rows = rows;
    q.d_disp = (int16_t *)c->disp.ptr; q.s = s;
    if (j.is_gsw) {
        g.d_raw_right = j.raw_right ? (int16_t *)c->lab.ptr : nullptr;
        rc = gsw_device_impl(*c, g);
    } else if (alternate) {            // (no exact pass and no dumps in this mode: left unset)
        a.exact = false;
        rc = asw_alternate_rows(*c, a, in0 & 1);
    } else {
        a.d_costs = j.costs ? (float *)c->costs.ptr : nullptr;
        a.d_raw_right = j.raw_right ? (int16_t *)c->lab.ptr : nullptr;
        rc = asw_device_impl(*c, a);
    }
    if (rc) return rc;
    if (j.raw_right)
        HIP_TRY(hipMemcpyAsync(j.raw_right + (size_t)j.o0 * W, c->lab.ptr, nout * 2, hipMemcpyDeviceToHost, s));
    if (j.disparity)
        HIP_TRY(hipMemcpyAsync(j.disparity + (size_t)j.o0 * W, c->disp.ptr, nout * 2, hipMemcpyDeviceToHost, s));
    if (j.costs) HIP_TRY(hipMemcpyAsync(j.costs, c->costs.ptr, ncost * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

// Contiguous row strips whose heights differ by at most one row (empty when there are more devices than rows) --
// the same cut as simplestereo_amd/strips.py::strip_bounds.  One host thread per strip: each takes its own device's lock, so the
// copies and kernels of all devices overlap.  The first failing strip's code and message are returned.
int run_strips(const HostJob &job, const int *devices, int n_devices)
{
    if (!devices || n_devices < 1) return fail(SSAMD_EINVAL, "devices must name at least one GPU");
    if (n_devices > 16) return fail(SSAMD_EINVAL, "at most 16 devices");
    for (int a = 0; a < n_devices; ++a) {
        if (devices[a] < 0) return fail(SSAMD_EINVAL, "devices[%d] = %d: explicit non-negative ordinals only", a, devices[a]);
        // test hook SSAMD_MULTI_ALLOW_REPEAT: a 1-GPU box exercises the strip cut with one device listed several
        // times (the strips then simply queue on that device's mutex)
        for (int b = 0; b < a && !tune().multi_allow_repeat; ++b)
            if (devices[a] == devices[b]) return fail(SSAMD_EINVAL, "device %d listed twice", devices[a]);
    }
    const MatchCall &q = job.is_gsw ? static_cast<const MatchCall &>(job.gsw) : job.asw;
    int rc = check_common(q.H, q.W, q.win, q.minD, q.maxD, 0, q.H);
    if (rc) return rc;
    const int base = q.H / n_devices, extra = q.H % n_devices;
    std::vector<int> codes(n_devices, SSAMD_OK);
    std::vector<std::string> msgs(n_devices);
    std::vector<std::thread> th;
    for (int k = 0; k < n_devices; ++k) {
        HostJob j = job;
        j.o0 = k * base + std::min(k, extra);
        j.o1 = j.o0 + base + (k < extra ? 1 : 0);
        if (j.o1 <= j.o0) continue;                      // more devices than rows: nothing for this one
        const int dev = devices[k];
        try {
            th.emplace_back([j, dev, k, &codes, &msgs]() {
                codes[k] = host_rows(j, dev);
                if (codes[k]) msgs[k] = g_err;           // thread-local message of the worker
            });
        } catch (const std::exception &e) {              // no exception may cross the C ABI: finish what runs, report
            codes[k] = SSAMD_ENOMEM;
            msgs[k] = std::string("could not start a host thread: ") + e.what();
            break;
        }
    }
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; ++k)
        if (codes[k]) return fail(codes[k], "strip %d on device %d: %s", k, devices[k], msgs[k].c_str());
    return SSAMD_OK;
}

// The rig's raw frames and maps of the *_rectified_device entry points, with their argument checks (d_out: checked with them)
int make_remap_src(RemapSrc &rm, const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                   const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int interpolation, const void *d_out)
{
    if (!d_raw1 || !d_raw2 || !d_mapx1 || !d_mapy1 || !d_mapx2 || !d_mapy2 || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    if (src_height <= 0 || src_width <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (interpolation != 0 && interpolation != 1) return fail(SSAMD_EINVAL, "only INTER_NEAREST (0) and INTER_LINEAR (1) are supported");
    rm.src1 = d_raw1; rm.src2 = d_raw2; rm.mapx1 = d_mapx1; rm.mapy1 = d_mapy1; rm.mapx2 = d_mapx2; rm.mapy2 = d_mapy2;
    rm.Hs = src_height; rm.Ws = src_width; rm.nearest = interpolation == 0 ? 1 : 0;
    return SSAMD_OK;
}

// "the skipped rows inside the output rows" of the _rows2 entry points
int check_skip_rows(int out_row0, int out_rows, int skip_row0, int skip_rows)
{
    if (skip_rows < 0 || (skip_rows > 0 && (skip_row0 < out_row0 || skip_row0 + skip_rows > out_row0 + out_rows)))
        return fail(SSAMD_EINVAL, "the skipped rows [%d,%d) must lie inside the output rows [%d,%d)", skip_row0, skip_row0 + skip_rows,
                    out_row0, out_row0 + out_rows);
    return SSAMD_OK;
}

// ssamd_asw_device, ssamd_asw_device_rows2 (skip_rows > 0), ssamd_asw_alternate_device and, with q.rm (checked by make_remap_src),
// ssamd_asw_rectified_device; `exact`: their _exact twins
int asw_device_entry(AswCall q, int skip_row0, int skip_rows)
{
    if (!q.rm && (!q.dL || !q.dR || !q.d_disp)) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    if ((rc = check_skip_rows(q.row0, q.rows, skip_row0, skip_rows))) return rc;
    q.skip_at = skip_rows > 0 ? skip_row0 - q.row0 : 0; q.skip = skip_rows;
    return asw_device_impl(*c, q);
}

int asw_rectified_entry(const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                        const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int interpolation, AswCall q)
{
    RemapSrc rm;
    const int rc = make_remap_src(rm, d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, interpolation, q.d_disp);
    q.rm = &rm;
    return rc ? rc : asw_device_entry(q, 0, 0);
}
}  // namespace

extern "C" {
// An ASW entry point and its _exact twin (the fp64 tie-break pass on top): one parameter list, one body, `exact` the only difference.
#define SSAMD_ASW_TWINS(SUFFIX, PARAMS, BODY)                                   \
    int ssamd_asw##SUFFIX PARAMS { const bool exact = false; return BODY; }     \
    int ssamd_asw_exact##SUFFIX PARAMS { const bool exact = true; return BODY; }

SSAMD_ASW_TWINS(_device, (const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows, int winSize,
                          int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent, int16_t *d_disparity, void *stream),
                asw_device_entry(asw_call(d_img1, d_img2, height, width, out_row0, out_rows, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                          consistent, d_disparity, stream, false, exact), 0, 0))

SSAMD_ASW_TWINS(_device_rows2, (const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows, int skip_row0,
                                int skip_rows, int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                                int16_t *d_disparity, void *stream),
                asw_device_entry(asw_call(d_img1, d_img2, height, width, out_row0, out_rows, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                          consistent, d_disparity, stream, false, exact), skip_row0, skip_rows))

SSAMD_ASW_TWINS(_rectified_device, (const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width, const float *d_mapx1,
                                    const float *d_mapy1, const float *d_mapx2, const float *d_mapy2, int height, int width, int interpolation,
                                    int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                                    int16_t *d_disparity, void *stream),
                asw_rectified_entry(d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, interpolation,
                                    asw_call(nullptr, nullptr, height, width, 0, height, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                             consistent, d_disparity, stream, false, exact)))
#undef SSAMD_ASW_TWINS

int ssamd_asw_alternate_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int winSize,
                               int maxDisparity, int minDisparity, double gammaC, double gammaP, int consistent,
                               int16_t *d_disparity, void *stream)
{
    return asw_device_entry(asw_call(d_img1, d_img2, height, width, 0, height, winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent,
                                     d_disparity, stream, true), 0, 0);
}

int ssamd_asw_alternate_rows_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                                    int row_parity, int winSize, int maxDisparity, int minDisparity, double gammaC, double gammaP,
                                    int consistent, int16_t *d_disparity, void *stream)
{
    if (!d_img1 || !d_img2 || !d_disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    if (row_parity != 0 && row_parity != 1) return fail(SSAMD_EINVAL, "row_parity must be 0 or 1");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    return asw_alternate_rows(*c, asw_call(d_img1, d_img2, height, width, out_row0, out_rows, winSize, maxDisparity, minDisparity, gammaC, gammaP,
                                           consistent, d_disparity, stream), row_parity);
}

// The matcher on host arrays, on one device or as row strips on several (rows are independent jobs and the tie-break pass is
// row-local: each strip runs its own): plain, exact, alternate rows
#define SSAMD_ASW_HOST_CALL(CONSISTENT, ALTERNATE, EXACT)      /* the parameters of the whole image: buffers, rows and stream are host_rows' */ \
    asw_call(nullptr, nullptr, height, width, 0, height, winSize, maxDisparity, minDisparity, gammaC, gammaP, CONSISTENT, nullptr, nullptr, ALTERNATE, EXACT)
#define SSAMD_ASW_HOST(NAME, ALTERNATE, EXACT)                                                                                              \
    int NAME(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity, int minDisparity,             \
             double gammaC, double gammaP, int consistent, int16_t *disparity, int device)                                                 \
    {                                                                                                                                      \
        if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");                                                        \
        return host_rows(HostJob(img1, img2, disparity, SSAMD_ASW_HOST_CALL(consistent, ALTERNATE, EXACT)), device);                       \
    }                                                                                                                                      \
    int NAME##_multi(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity, int minDisparity,     \
                     double gammaC, double gammaP, int consistent, int16_t *disparity, const int *devices, int n_devices)                  \
    {                                                                                                                                      \
        if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");                                                        \
        return run_strips(HostJob(img1, img2, disparity, SSAMD_ASW_HOST_CALL(consistent, ALTERNATE, EXACT)), devices, n_devices);          \
    }
SSAMD_ASW_HOST(ssamd_asw, false, false)
SSAMD_ASW_HOST(ssamd_asw_exact, false, true)
SSAMD_ASW_HOST(ssamd_asw_alternate, true, false)

int ssamd_asw_costs(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                    int minDisparity, double gammaC, double gammaP, float *costs, int device)
{
    if (!img1 || !img2 || !costs) return fail(SSAMD_EINVAL, "NULL buffer");
    if (maxDisparity < minDisparity) return fail(SSAMD_EINVAL, "empty disparity range");
    HostJob j(img1, img2, nullptr, SSAMD_ASW_HOST_CALL(0, false, false));
    j.costs = costs;
    return host_rows(j, device);
}

int ssamd_asw_argmins(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                      int minDisparity, double gammaC, double gammaP, int16_t *left_disparity, int16_t *right_match,
                      int device)
{
    if (!img1 || !img2 || !left_disparity || !right_match) return fail(SSAMD_EINVAL, "NULL buffer");
    if (maxDisparity < minDisparity) return fail(SSAMD_EINVAL, "empty disparity range");
    HostJob j(img1, img2, left_disparity, SSAMD_ASW_HOST_CALL(1, false, false));
    j.raw_right = right_match;
    return host_rows(j, device);
}
#undef SSAMD_ASW_HOST
#undef SSAMD_ASW_HOST_CALL

int ssamd_gsw_device(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                     int winSize, int maxDisparity, int minDisparity, int gamma, float fMax, int iterations, int bins,
                     int16_t *d_disparity, void *stream)
{
    return ssamd_gsw_device_rows2(d_img1, d_img2, height, width, out_row0, out_rows, 0, 0, winSize, maxDisparity, minDisparity, gamma, fMax,
                                  iterations, bins, d_disparity, stream);
}

// ssamd_gsw_device on TWO row ranges (round 6: the border bands of a row strip whose interior rows ran while the halo was in flight,
// strips.py).  GSW workgroups are small (two 8-wave groups per CU, strips of 2-8 rows) and a band is winSize/2 = 5 rows at the class
// default: each band is an ordinary call on its rows -- pack, both passes, left-right check -- written at its place in d_disparity.
int ssamd_gsw_device_rows2(const uint8_t *d_img1, const uint8_t *d_img2, int height, int width, int out_row0, int out_rows,
                           int skip_row0, int skip_rows, int winSize, int maxDisparity, int minDisparity, int gamma, float fMax,
                           int iterations, int bins, int16_t *d_disparity, void *stream)
{
    (void)bins;                       // never read by the reference either (_passive.cpp:410)
    if (!d_img1 || !d_img2 || !d_disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = check_skip_rows(out_row0, out_rows, skip_row0, skip_rows);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    GswCall q = gsw_params(height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations);
    q.dL = d_img1; q.dR = d_img2; q.row0 = out_row0; q.rows = out_rows; q.d_disp = d_disparity; q.s = (hipStream_t)stream;
    if (skip_rows == 0) return gsw_device_impl(*c, q);
    if ((rc = check_common(height, width, winSize, minDisparity, maxDisparity, out_row0, out_rows))) return rc;
    const int bot0 = skip_row0 + skip_rows, band0[2] = {out_row0, bot0}, band_rows[2] = {skip_row0 - out_row0, out_row0 + out_rows - bot0};
    for (int k = 0; k < 2; ++k) {
        q.row0 = band0[k]; q.rows = band_rows[k]; q.d_disp = d_disparity + (size_t)(band0[k] - out_row0) * width;
        if (band_rows[k] > 0 && (rc = gsw_device_impl(*c, q))) return rc;
    }
    return SSAMD_OK;
}

int ssamd_gsw_rectified_device(const uint8_t *d_raw1, const uint8_t *d_raw2, int src_height, int src_width,
                               const float *d_mapx1, const float *d_mapy1, const float *d_mapx2, const float *d_mapy2,
                               int height, int width, int interpolation, int winSize, int maxDisparity, int minDisparity,
                               int gamma, float fMax, int iterations, int bins, int16_t *d_disparity, void *stream)
{
    (void)bins;
    RemapSrc rm;
    int rc = make_remap_src(rm, d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, interpolation, d_disparity);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    GswCall q = gsw_params(height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations);
    q.rm = &rm; q.rows = height; q.d_disp = d_disparity; q.s = (hipStream_t)stream;
    return gsw_device_impl(*c, q);
}

int ssamd_gsw(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
              int minDisparity, int gamma, float fMax, int iterations, int bins, int16_t *disparity, int device)
{
    (void)bins;
    if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    return host_rows(HostJob(img1, img2, disparity, gsw_params(height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations)), device);
}

int ssamd_gsw_argmins(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                      int minDisparity, int gamma, float fMax, int iterations, int bins, int16_t *left_disparity,
                      int16_t *right_match, int device)
{
    (void)bins;
    if (!img1 || !img2 || !left_disparity || !right_match) return fail(SSAMD_EINVAL, "NULL buffer");
    HostJob j(img1, img2, left_disparity, gsw_params(height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations));
    j.raw_right = right_match;
    return host_rows(j, device);
}

int ssamd_gsw_multi(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, int maxDisparity,
                    int minDisparity, int gamma, float fMax, int iterations, int bins, int16_t *disparity,
                    const int *devices, int n_devices)
{
    (void)bins;
    if (!img1 || !img2 || !disparity) return fail(SSAMD_EINVAL, "NULL buffer");
    return run_strips(HostJob(img1, img2, disparity, gsw_params(height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations)),
                      devices, n_devices);
}
}  // extern "C"
