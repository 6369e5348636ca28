// Host section of ssamd_api.hip: IIR phase unwrapping (unwrap_kernels.hip.h) -- check, launch, entry points.
namespace {
// _unwrapping.infiniteImpulseResponse's checks (_unwrapping.cpp:63-74) on n [h][w] maps, plus the kernel's own limits
int unwrap_check(int n, int h, int w, double tau)
{
    if (n < 0 || h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    if (tau < 0 || tau > 1) return fail(SSAMD_EINVAL, "Wrong tau value!");                   // NaN passes, as in the reference
    if (w > UNWRAP_MAX_W) return fail(SSAMD_ELIMIT, "phase maps wider than %d columns are not supported (width %d)", UNWRAP_MAX_W, w);
    if ((long long)h * w > (1ll << 40)) return fail(SSAMD_ELIMIT, "phase map of %d x %d pixels too large", h, w);
    return SSAMD_OK;
}

// One workgroup per map.  Bands as few as the row cap allows, their heights as even as whole waves make them: the step count,
// bands * w + 2 (h - bands), depends on the number of bands only, and fewer waves per workgroup share the CU's SIMDs.
int unwrap_launch(Ctx &c, const double *d_phase, int n, int h, int w, double tau, double *d_out, hipStream_t s)
{
    if (n == 0) return SSAMD_OK;
    const int cap = tune().unwrap_rows > 0 ? round_up(tune().unwrap_rows, 64) : UNWRAP_MAX_ROWS;
    const int bands = (h + cap - 1) / cap;
    const int R = round_up((h + bands - 1) / bands, 64);
    const int lds = (w + 2 * R) * (int)sizeof(double);
    int rc = grant_dyn_lds(c, reinterpret_cast<const void *>(&iir_unwrap_kernel), lds);
    if (rc) return rc;
    Timed t(c, s, SSAMD_K_UNWRAP);
    hipLaunchKernelGGL(iir_unwrap_kernel, dim3(n), dim3(R), lds, s, d_phase, d_out, h, w, tau);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_iir_unwrap(const double *phase, int n, int h, int w, double tau, double *out, int device)
{
    if (!phase || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = unwrap_check(n, h, w, tau);
    if (rc) return rc;
    if (n == 0) return SSAMD_OK;
    const size_t bytes = (size_t)n * h * w * sizeof(double);
    return host_route(device, {{&Ctx::uwIn, phase, bytes}}, {&Ctx::uwOut, out, bytes}, [&](Ctx &c, hipStream_t s) {
        return unwrap_launch(c, (const double *)c.uwIn.ptr, n, h, w, tau, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_iir_unwrap_device(const double *d_phase, int n, int h, int w, double tau, double *d_out, void *stream)
{
    if (!d_phase || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    int rc = unwrap_check(n, h, w, tau);
    if (rc) return rc;
    if (n == 0) return SSAMD_OK;
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return unwrap_launch(*c, d_phase, n, h, w, tau, d_out, (hipStream_t)stream);
}
}  // extern "C"
