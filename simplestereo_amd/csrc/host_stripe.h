// Host section of ssamd_api.hip: findCentralStripe's per-row centroid (stripe_centroid_kernel, ftp_reference_kernels.hip.h) -- check, launch, entry points.
namespace {
int stripe_check(int h, int w, int channel, int threshold)
{
    if (h < 0 || w < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if ((long long)h * w * 3 >= (1ll << 40)) return fail(SSAMD_EINVAL, "image of %d x %d pixels too large", h, w);
    if (channel < 0 || channel > 2) return fail(SSAMD_EINVAL, "channel must be 0, 1 or 2");
    if (threshold < 0 || threshold > 256) return fail(SSAMD_EINVAL, "threshold must be in 0 .. 256");
    return SSAMD_OK;
}

int stripe_launch(Ctx &c, const uint8_t *d_img, int h, int w, int channel, int threshold, double *d_out, hipStream_t s)
{
    const int per_block = STRIPE_THREADS / 64;
    const int blocks = std::min((h + per_block - 1) / per_block, c.cus * 8);
    Timed t(c, s, SSAMD_K_FTP);
    hipLaunchKernelGGL(stripe_centroid_kernel, dim3(blocks), dim3(STRIPE_THREADS), 0, s, d_img, h, w, channel, threshold, d_out);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_stripe_centroids(const uint8_t *img, int h, int w, int channel, int threshold, double *out, int device)
{
    int rc = stripe_check(h, w, channel, threshold);
    if (rc || h == 0 || w == 0) return rc;
    if (!img || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    return host_route(device, {{&Ctx::uwIn, img, (size_t)h * w * 3}}, {&Ctx::uwOut, out, (size_t)h * sizeof(double)}, [&](Ctx &c, hipStream_t s) {
        return stripe_launch(c, (const uint8_t *)c.uwIn.ptr, h, w, channel, threshold, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_stripe_centroids_device(const uint8_t *d_img, int h, int w, int channel, int threshold, double *d_out, void *stream)
{
    int rc = stripe_check(h, w, channel, threshold);
    if (rc || h == 0 || w == 0) return rc;
    if (!d_img || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return stripe_launch(*c, d_img, h, w, channel, threshold, d_out, (hipStream_t)stream);
}
}  // extern "C"
