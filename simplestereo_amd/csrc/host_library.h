// Host section of ssamd_api.hip: library-wide entry points -- version, last error, devices, kernel names, options, counters, autotune, geometry queries, profile.
namespace {
int check_geometry_query(int width, int winSize, int maxDisparity, int minDisparity, const int *out, int *nD)
{
    if (!out) return fail(SSAMD_EINVAL, "out is NULL");
    int rc = check_common(1 << 14, width, winSize, minDisparity, maxDisparity, 0, 0);
    if (rc) return rc;
    *nD = maxDisparity - minDisparity + 1;
    return *nD < 1 ? fail(SSAMD_EINVAL, "empty disparity range") : SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_abi_version(void) { return SSAMD_ABI_VERSION; }
const char *ssamd_last_error(void) { return g_err.c_str(); }

int ssamd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ssamd_kernel_name(int slot)
{
    static const char *names[SSAMD_K_COUNT] = {"asw pre-pass (asw_prepass_kernel: Lab records + TAD volume; or bgr2lab_records_pair_kernel, asw_tad_volume_kernel)", "asw aggregation kernel (asw_aggregate_pipe / _wave / asw_aggregate_kernel)",
                                               "asw finalize (wta_decode / lr_check_fill)",
                                               "gsw_aggregate_kernel", "gsw finalize (lr_check_fill)", "remap_bgr_kernel / ftp_reference_kernel", "reproject_kernel / ftp_cloud_kernel",
                                               "asw_alt_fill_kernel", "asw fp64 tie-break pass (bgr2lab_f64_pair + asw_exact_winners / _eval / _resolve / _patch kernels)",
                                               "iir_unwrap_kernel", "ftp_phase_kernel", "np_unwrap_row_kernel / np_unwrap_col_kernel"};
    return (slot >= 0 && slot < SSAMD_K_COUNT) ? names[slot] : "";
}

int ssamd_set_option(const char *name, const char *value)
{
    if (!name) return fail(SSAMD_EINVAL, "option name is NULL");
    std::lock_guard<std::mutex> lk(g_tune_mutex);
    if (value) {
        if (!tuning_assign(g_tuning, name, value)) return fail(SSAMD_EINVAL, "unknown option %s", name);
    } else {
        // NULL = back to the value the library loaded from the environment (not "unset": a process started with
        // SSAMD_ASW_WAVE=0 keeps that setting after a `with options(...)` block of a test)
        const auto it = g_tuning_env.find(name);
        if (!tuning_assign(g_tuning, name, it == g_tuning_env.end() ? nullptr : it->second.c_str()))
            return fail(SSAMD_EINVAL, "unknown option %s", name);
    }
    if (std::string(name) == "SSAMD_AUTOTUNE")
        g_autotune.store(g_tuning.autotune_env != -2 ? g_tuning.autotune_env : -1);
    g_tune_version.fetch_add(1, std::memory_order_release);
    return SSAMD_OK;
}

int ssamd_counter(int device, const char *name, long long *value)
{
    if (!name || !value) return fail(SSAMD_EINVAL, "name / value is NULL");
    CtxLock c;
    int rc = get_ctx(device, c);
    if (rc) return rc;
    const std::string n(name);
    if (n == "evol_fallbacks") *value = c->evol_fallbacks;
    else if (n == "evol_bytes") *value = (long long)c->evol.cap;
    else if (n == "tail_splits") *value = c->tail_splits;
    else if (n == "exact_calls") *value = c->exact_calls;
    else if (n == "pipe_persist_launches") *value = c->persist_launches;
    else if (n == "gsw_plain_calls") *value = c->gsw_plain_calls;
    else if (n == "pipe_persist_items") {
        // tiles finished by persistent phase-shifted launches on this device so far (counted on the device, once per finished item)
        unsigned long long done = 0;
        if (c->pq.ptr) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(&done, (const unsigned int *)c->pq.ptr + ASW_PQ_QUEUES * ASW_PQ_LINE, sizeof(done), hipMemcpyDeviceToHost));
        }
        *value = (long long)done;
    }
    else if (n == "exact_entries" || n == "exact_flagged_left" || n == "exact_flagged_right" || n == "exact_overflow" || n == "exact_raw_entries") {
        // of the LAST exact call on this device: candidates re-evaluated in fp64, pixels with near-ties, whether the queue overflowed
        unsigned int ctr[EXACT_CTR_COUNT];
        if ((rc = asw_exact_counters(*c, ctr))) return rc;
        *value = n == "exact_entries" ? ctr[EXACT_CTR_ENTRIES] : n == "exact_flagged_left" ? ctr[EXACT_CTR_FLAGGED_L] :
                 n == "exact_flagged_right" ? ctr[EXACT_CTR_FLAGGED_R] : n == "exact_raw_entries" ? ctr[EXACT_CTR_RAW] :
                 ((ctr[EXACT_CTR_ENTRIES] > c->xq[0].cap || (c->xq[1].cap && ctr[EXACT_CTR_RAW] > c->xq[1].cap)) ? 1 : 0);
    }
    else return fail(SSAMD_EINVAL, "unknown counter %s", name);
    return SSAMD_OK;
}

int ssamd_autotune(int on)
{
    return g_autotune.exchange(on > 0 ? 1 : (on < 0 ? -1 : 0));
}

int ssamd_asw_geometry(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    const Tuning &t = tune();
    const PlanOptions po{t, false};
    AswGeom g;
    if ((rc = asw_choose_geometry(g, po, width, rows, winSize, nD))) return rc;
    out[0] = g.Tx; out[1] = g.Dc; out[2] = g.nchunks; out[3] = g.threads; out[4] = g.lds_bytes;
    out[5] = (width + g.Tx - 1) / g.Tx; out[6] = rows; out[7] = g.nchunks;
    AswWaveGeom wg;
    if (g.wave_rx && asw_wave_layout(wg, po, winSize, nD, g.wave_rx, t.wave_unroll != 0)) {      // a "tile" = the four strips of a workgroup's waves (LDS of the plain call: no cost dump)
        out[0] = wg.Txw * wg.waves; out[1] = wg.Dc; out[2] = 1; out[3] = 64 * wg.waves; out[4] = wg.wave_lds * wg.waves;
        out[5] = (width + out[0] - 1) / out[0]; out[7] = 1;
    }
    return SSAMD_OK;
}

int ssamd_asw_kernel_form(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    const Tuning &t = tune();
    AswGeom g;
    if ((rc = asw_choose_geometry(g, PlanOptions{t, false}, width, rows, winSize, nD))) return rc;
    out[0] = g.pipe; out[1] = g.Rx; out[2] = g.JC >= winSize ? 0 : g.JC; out[3] = g.pipe ? g.dephase : 0;
    out[4] = g.wave_rx & 15;
    if (g.wave_rx) { out[0] = 0; out[1] = g.wave_rx & 15; out[2] = 0; out[3] = 0; }
    return SSAMD_OK;
}

int ssamd_gsw_geometry(int width, int rows, int winSize, int maxDisparity, int minDisparity, int *out)
{
    int nD, rc = check_geometry_query(width, winSize, maxDisparity, minDisparity, out, &nD);
    if (rc) return rc;
    GswGeom g;
    if ((rc = gsw_choose_geometry(g, tune(), width, rows, winSize, nD))) return rc;
    out[0] = g.Tx; out[1] = g.Dc; out[2] = g.nchunks; out[3] = g.threads * g.Hy; out[4] = g.lds_bytes;
    out[5] = (width + g.Tx - 1) / g.Tx; out[6] = (rows + g.Ty * g.Hy - 1) / (g.Ty * g.Hy); out[7] = g.nchunks; out[8] = g.Ty * g.Hy;
    return SSAMD_OK;
}

int ssamd_profile_enable(int on)
{
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        c.prof.on = on != 0;
    }
    return SSAMD_OK;
}

int ssamd_profile_reset(void)
{
    DeviceGuard guard;
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.dev < 0) continue;
        (void)hipSetDevice(c.dev);
        c.prof.drain();
        std::fill(c.prof.ms, c.prof.ms + SSAMD_K_COUNT, 0.0);
        std::fill(c.prof.n, c.prof.n + SSAMD_K_COUNT, 0LL);
    }
    return SSAMD_OK;
}

int ssamd_profile_read(double *ms, long long *launches)
{
    DeviceGuard guard;
    for (int k = 0; k < SSAMD_K_COUNT; ++k) { if (ms) ms[k] = 0; if (launches) launches[k] = 0; }
    for (auto &c : g_ctx) {
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.dev < 0) continue;
        (void)hipSetDevice(c.dev);
        c.prof.drain();
        for (int k = 0; k < SSAMD_K_COUNT; ++k) { if (ms) ms[k] += c.prof.ms[k]; if (launches) launches[k] += c.prof.n[k]; }
    }
    return SSAMD_OK;
}
}  // extern "C"
