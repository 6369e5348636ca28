// Host section of ssamd_api.hip: np.unwrap (np_unwrap_kernels.hip.h, np_unwrap_plan.h) -- check, launch, entry points.
namespace {
// np.unwrap on the geometry [outer][len][inner] (np_unwrap_plan.h): the checks shared by the host and the device entry points
int npu_check(long long outer, long long len, long long inner, double period, NpuPlan &plan)
{
    if (!(period > 0) || !std::isfinite(period)) return fail(SSAMD_EINVAL, "period must be a finite positive number");
    switch (npu_plan(outer, len, inner, plan)) {
    case NPU_OK: return SSAMD_OK;
    case NPU_NEGATIVE: return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    case NPU_TOO_MANY_ELEMS: return fail(SSAMD_ELIMIT, "more than 2^40 phase samples (%lld x %lld x %lld)", outer, len, inner);
    default:
        return fail(SSAMD_ELIMIT, "more than %lld %s to scan (%lld x %lld): one launch holds fewer than 2^32 threads",
                    NPU_MAX_LAUNCH_THREADS / plan.threads, plan.form == 0 ? "lines" : "groups of 16 columns", outer, inner);
    }
}

// one scan; d_out may be d_p (the kernels work in place)
int npu_launch(Ctx &c, const NpuPlan &plan, const double *d_p, long long len, long long inner, double discont, double period,
               double *d_out, hipStream_t s)
{
    if (plan.blocks == 0) return SSAMD_OK;
    const double hi = period / 2, lo = -hi;
    Timed t(c, s, SSAMD_K_NPUNWRAP);
    if (plan.form == 0)
        hipLaunchKernelGGL(np_unwrap_row_kernel, dim3((unsigned)plan.blocks), dim3(plan.threads), 0, s, d_p, d_out, len, discont, period,
                           hi, lo);
    else
        hipLaunchKernelGGL(np_unwrap_col_kernel, dim3((unsigned)plan.blocks), dim3(plan.threads), 0, s, d_p, d_out, len, inner,
                           plan.groups, discont, period, hi, lo);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

// the reference's default composition (active.py:739-745) on n maps [h][w]: along x (axis 1), then along y (axis 0), discont = pi
struct NpuXY { NpuPlan x, y; };
int npu_xy_check(int n, int h, int w, NpuXY &q)
{
    if (n < 0 || h < 0 || w < 0) return fail(SSAMD_EINVAL, "Wrong phase dimensions!");
    int rc = npu_check((long long)n * h, w, 1, 2 * M_PI, q.x);
    return rc ? rc : npu_check(n, h, w, 2 * M_PI, q.y);
}
int npu_xy_launch(Ctx &c, const NpuXY &q, const double *d_p, int h, int w, double *d_out, hipStream_t s)
{
    int rc = npu_launch(c, q.x, d_p, w, 1, M_PI, 2 * M_PI, d_out, s);
    return rc ? rc : npu_launch(c, q.y, d_out, h, w, M_PI, 2 * M_PI, d_out, s);
}
}  // namespace

extern "C" {
int ssamd_np_unwrap_plan(long long outer, long long len, long long inner, int32_t *plan)
{
    if (!plan) return fail(SSAMD_EINVAL, "NULL buffer");
    NpuPlan q;
    int rc = npu_check(outer, len, inner, 1.0, q);
    if (rc) return rc;
    const int32_t v[8] = {q.form, q.chunk, q.lanes, q.threads, (int32_t)q.blocks, q.lds_bytes, q.per_thread, (int32_t)q.groups};
    std::copy(v, v + 8, plan);
    return SSAMD_OK;
}

int ssamd_np_unwrap(const double *p, long long outer, long long len, long long inner, double discont, double period, double *out,
                    int device)
{
    NpuPlan q;
    int rc = npu_check(outer, len, inner, period, q);
    if (rc || q.blocks == 0) return rc;
    if (!p || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t bytes = (size_t)outer * len * inner * sizeof(double);
    return host_route(device, {{&Ctx::uwIn, p, bytes}}, {&Ctx::uwOut, out, bytes}, [&](Ctx &c, hipStream_t s) {
        return npu_launch(c, q, (const double *)c.uwIn.ptr, len, inner, discont, period, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_np_unwrap_device(const double *d_p, long long outer, long long len, long long inner, double discont, double period,
                           double *d_out, void *stream)
{
    NpuPlan q;
    int rc = npu_check(outer, len, inner, period, q);
    if (rc || q.blocks == 0) return rc;
    if (!d_p || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return npu_launch(*c, q, d_p, len, inner, discont, period, d_out, (hipStream_t)stream);
}

int ssamd_np_unwrap_xy(const double *p, int n, int h, int w, double *out, int device)
{
    NpuXY q;
    int rc = npu_xy_check(n, h, w, q);
    if (rc || q.y.blocks == 0) return rc;
    if (!p || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    const size_t bytes = (size_t)n * h * w * sizeof(double);
    return host_route(device, {{&Ctx::uwIn, p, bytes}}, {&Ctx::uwOut, out, bytes}, [&](Ctx &c, hipStream_t s) {
        return npu_xy_launch(c, q, (const double *)c.uwIn.ptr, h, w, (double *)c.uwOut.ptr, s);
    });
}

int ssamd_np_unwrap_xy_device(const double *d_p, int n, int h, int w, double *d_out, void *stream)
{
    NpuXY q;
    int rc = npu_xy_check(n, h, w, q);
    if (rc || q.y.blocks == 0) return rc;
    if (!d_p || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return npu_xy_launch(*c, q, d_p, h, w, d_out, (hipStream_t)stream);
}
}  // extern "C"
