// Host section of ssamd_api.hip: verification and debug entry points (ssamd_bgr2lab, ssamd_debug_*) with debug_libm_kernel.
namespace {
// (C linkage: internal to the unit like everything here, under the plain name its symbol in the code object has always had)
extern "C" __global__ void debug_libm_kernel(int which, int n, const void *in, void *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (which == 0) reinterpret_cast<double *>(out)[i] = glibc_exp(reinterpret_cast<const double *>(in)[i]);
    else if (which == 1) reinterpret_cast<float *>(out)[i] = glibc_powf_pos(reinterpret_cast<const float *>(in)[i], (float)(1 / 3.0));
    else if (which == 2) reinterpret_cast<double *>(out)[i] = ssamd::exact_sqrt(reinterpret_cast<const double *>(in)[i]);
    else reinterpret_cast<double *>(out)[i] = reinterpret_cast<const double *>(in)[i] / 0.7 + reinterpret_cast<const double *>(in)[i] / 5.0;
}
}  // namespace

extern "C" {
int ssamd_bgr2lab(const uint8_t *img, int height, int width, float *lab, int device)
{
    if (!img || !lab || height <= 0 || width <= 0) return fail(SSAMD_EINVAL, "bad argument");
    const size_t npix = (size_t)height * width;
    return host_route(device, {{&Ctx::imgL, img, npix * 3}}, {&Ctx::lab, lab, npix * 12}, [&](Ctx &c, hipStream_t s) {
        const int blocks = (int)std::min<size_t>((npix + 255) / 256, 256 * 8);
        hipLaunchKernelGGL(bgr2lab_f32_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t *)c.imgL.ptr, (float *)c.lab.ptr, (long long)npix);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    });
}

// Verification: the fp64 costs the tie-break pass computes for n given candidates (y, x, d triples), and optionally the fp64 Lab
// images it reads -- to compare with the oracle's fp64 costs bit for bit.
int ssamd_debug_exact_costs(const uint8_t *img1, const uint8_t *img2, int height, int width, int winSize, double gammaC, double gammaP,
                            int n, const int *yxd, double *costs, double *lab1, double *lab2)
{
    if (!img1 || !img2 || !yxd || !costs || n < 0) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = check_common(height, width, winSize, 0, 0, 0, height);
    if (rc) return rc;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    const size_t npix = (size_t)height * width;
    hipStream_t s = c->stream;
    ScratchOrder order(*c, s);
    if ((rc = c->imgL.reserve(npix * 3)) || (rc = c->imgR.reserve(npix * 3)) || (rc = c->recL.reserve(npix * sizeof(PixRec))) ||
        (rc = c->recR.reserve(npix * sizeof(PixRec))) || (rc = c->xlabL.reserve(npix * 24)) || (rc = c->xlabR.reserve(npix * 24)) ||
        (rc = c->xqueue.reserve((size_t)std::max(n, 1) * 8)) || (rc = c->xcost.reserve((size_t)std::max(n, 1) * 8)) || (rc = c->xctr.reserve(64)))
        return rc;
    if (c->xq[0].entries) c->xq[0].entries = (u64 *)c->xqueue.ptr;      // (the reservation may have moved the last exact call's queue buffer)
    HIP_TRY(hipMemcpyAsync(c->imgL.ptr, img1, npix * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->imgR.ptr, img2, npix * 3, hipMemcpyHostToDevice, s));
    const int blocks = (int)std::min<long long>((2 * (long long)npix + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(bgr2lab_records_pair_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t *)c->imgL.ptr, (const uint8_t *)c->imgR.ptr,
                       (PixRec *)c->recL.ptr, (PixRec *)c->recR.ptr, (long long)npix);
    hipLaunchKernelGGL(bgr2lab_f64_pair_kernel, dim3(blocks), dim3(256), 0, s, (const PixRec *)c->recL.ptr, (const PixRec *)c->recR.ptr,
                       (double *)c->xlabL.ptr, (double *)c->xlabR.ptr, (long long)npix);
    std::vector<u64> ent((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int y = yxd[3 * k], x = yxd[3 * k + 1], d = yxd[3 * k + 2];
        if (y < 0 || y >= height || x < 0 || x >= width || d < 0 || x - d < 0) return fail(SSAMD_EINVAL, "candidate %d outside the image", k);
        ent[k] = exact_entry((uint32_t)y * (uint32_t)width + (uint32_t)x, d, 0u);       // sides = 0: cost only
    }
    unsigned int ctr[EXACT_CTR_COUNT] = {};
    ctr[EXACT_CTR_ENTRIES] = (unsigned int)n;
    HIP_TRY(hipMemcpyAsync(c->xqueue.ptr, ent.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->xctr.ptr, ctr, sizeof(ctr), hipMemcpyHostToDevice, s));
    const double *d_prox = nullptr;
    if ((rc = get_prox64(*c, winSize, gammaP, s, &d_prox))) return rc;
    AswExactArgs x{};
    x.rec[0] = (const PixRec *)c->recL.ptr; x.rec[1] = (const PixRec *)c->recR.ptr;
    x.lab[0] = (const double *)c->xlabL.ptr; x.lab[1] = (const double *)c->xlabR.ptr;
    x.prox = d_prox; x.q.entries = (u64 *)c->xqueue.ptr; x.q.counter = (unsigned int *)c->xctr.ptr; x.q.cap = (unsigned int)std::max(n, 1);
    x.ecost = (double *)c->xcost.ptr;
    x.H = height; x.W = width; x.win = winSize; x.pad = winSize / 2; x.row0 = 0; x.rows = height; x.gammaC = gammaC;
    hipLaunchKernelGGL(asw_exact_eval_kernel, dim3(256), dim3(64 * EXACT_WAVES), 0, s, x);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(costs, c->xcost.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (lab1) HIP_TRY(hipMemcpyAsync(lab1, c->xlabL.ptr, npix * 24, hipMemcpyDeviceToHost, s));
    if (lab2) HIP_TRY(hipMemcpyAsync(lab2, c->xlabR.ptr, npix * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SSAMD_OK;
}

// Verification / diagnosis: the queues of the LAST exact call on the current device.  which = 0: the final queue (entries
// re-evaluated in fp64), 1: the raw queue of a merging call with its cost images.  Copies up to max_n entries; *n = entries appended.
int ssamd_debug_exact_queue(int which, long long max_n, unsigned long long *entries, unsigned int *keys, long long *n)
{
    if (!n || max_n < 0 || (max_n > 0 && !entries)) return fail(SSAMD_EINVAL, "bad argument");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    *n = 0;
    unsigned int ctr[EXACT_CTR_COUNT];
    if ((rc = asw_exact_counters(*c, ctr))) return rc;      // (all zero when no exact call has run: nothing to copy)
    const unsigned int cnt = ctr[which ? EXACT_CTR_RAW : EXACT_CTR_ENTRIES], cap = c->xq[which ? 1 : 0].cap;
    *n = cnt;
    const size_t m = (size_t)std::min<long long>(std::min<unsigned int>(cnt, cap), max_n);
    if (m == 0) return SSAMD_OK;
    const AswExactQueue &q = c->xq[which ? 1 : 0];         // (as asw_exact_prepare carved it)
    if (!q.entries) return SSAMD_OK;
    HIP_TRY(hipMemcpy(entries, q.entries, m * 8, hipMemcpyDeviceToHost));
    if (which && keys) HIP_TRY(hipMemcpy(keys, q.ekeys, m * 4, hipMemcpyDeviceToHost));
    return SSAMD_OK;
}

int ssamd_debug_libm(int which, int n, const void *in, void *out)
{
    if (!in || !out || n < 0 || which < 0 || which > 3)
        return fail(SSAMD_EINVAL, "ssamd_debug_libm: which = 0 (exp, doubles), 1 (powf(x, 1/3), floats), 2 (sqrt, doubles), 3 (x / 0.7 + x / 5.0, doubles)");
    if (n == 0) return SSAMD_OK;
    // both halves of one scratch buffer: the input in the upper one, so that the first reservation is the buffer's only one
    const size_t bytes = (size_t)n * (which == 1 ? 4 : 8);
    return host_route(-1, {{&Ctx::lab, in, bytes, bytes}}, {&Ctx::lab, out, bytes}, [&](Ctx &c, hipStream_t s) {
        hipLaunchKernelGGL(debug_libm_kernel, dim3((n + 255) / 256), dim3(256), 0, s, which, n, (const void *)staged(c, &Ctx::lab, bytes),
                           (void *)staged(c, &Ctx::lab));
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    });
}

int ssamd_debug_gsw_sqrt(int n, float *out)
{
    int what = 0;
    if (n < 0) { what = 1; n = -n; }       // n < 0: the bare v_sqrt_f32 over 0 .. -n - 1 (measurement of why it is not used)
    if (!out || n <= 0 || n > GSW_TAB_SIZE) return fail(SSAMD_EINVAL, "bad argument");
    return host_route(-1, {}, {&Ctx::lab, out, (size_t)n * 4}, [&](Ctx &c, hipStream_t s) {
        hipLaunchKernelGGL(gsw_sqrt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (float *)c.lab.ptr, n, what);
        HIP_TRY(hipGetLastError());
        return SSAMD_OK;
    });
}
}  // extern "C"
