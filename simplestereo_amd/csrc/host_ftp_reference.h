// Host section of ssamd_api.hip: FTP virtual reference image (ftp_reference_kernels.hip.h) -- weight table, check, launch, entry points.
namespace {
// OpenCV's initInterTab2D(INTER_CUBIC, fixpt) as published (modules/imgproc/src/imgwarp.cpp), [fy][fx][tap row][tap column]:
// float32 cubic coefficients with A = -0.75 at the fractions i / 32 (interpolateCubic; every operation is exact in float32
// there: the values are multiples of 2^-17 below 2^4), the float32 outer product times 32768 rounded half to even and saturated to short (the 1.0 of fraction (0, 0) is 32767),
// and where the 16 shorts do not sum to 32768 the difference goes to ONE entry found among the taps (2..3, 2..3) of the 4 x 4:
// the largest of them when the sum is short, the smallest when it is over -- with OpenCV's scan, which starts at (2, 2) and
// tests "smaller than the minimum" first and "larger than the maximum" only otherwise.  simplestereo_amd/_rigs.py
// (_cubic_table) and tests/_stereo_ftp_ref.py state the same table in numpy.
const short *ftp_reference_table()
{
#pragma clang fp contract(off)
    static const std::vector<short> table = [] {
        std::vector<short> t(FTP_REF_TAB);
        float c[32][4];
        const float A = -0.75f;
        for (int i = 0; i < 32; ++i) {
            const float x = i * (1.f / 32);
            c[i][0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
            c[i][1] = ((A + 2) * x - (A + 3)) * x * x + 1;
            c[i][2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
            c[i][3] = 1.f - c[i][0] - c[i][1] - c[i][2];
        }
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                short *const it = t.data() + (i * 32 + j) * 16;
                int isum = 0;
                for (int k1 = 0; k1 < 4; ++k1)
                    for (int k2 = 0; k2 < 4; ++k2) {
                        const float v = c[i][k1] * c[j][k2];
                        isum += it[k1 * 4 + k2] = (short)std::min(std::max(lrintf(v * 32768.f), -32768l), 32767l);      // saturate_cast<short>: 1.0 -> 32767
                    }
                if (isum != 32768) {
                    const int diff = isum - 32768;
                    int Mk1 = 2, Mk2 = 2, mk1 = 2, mk2 = 2;
                    for (int k1 = 2; k1 < 4; ++k1)
                        for (int k2 = 2; k2 < 4; ++k2) {
                            if (it[k1 * 4 + k2] < it[mk1 * 4 + mk2]) mk1 = k1, mk2 = k2;
                            else if (it[k1 * 4 + k2] > it[Mk1 * 4 + Mk2]) Mk1 = k1, Mk2 = k2;
                        }
                    if (diff < 0) it[Mk1 * 4 + Mk2] = (short)(it[Mk1 * 4 + Mk2] - diff);
                    else it[mk1 * 4 + mk2] = (short)(it[mk1 * 4 + mk2] - diff);
                }
            }
        return t;
    }();
    return table.data();
}

// the checks shared by the host and the device entry point; fills the by-value geometry and the distortion model
static_assert(sizeof(FtpProjGeom) <= SSAMD_FTP_CLOUD_NGEOM * sizeof(double), "geom layout of ssamd.h");
int ftp_reference_check(int hp, int wp, int h, int w, int x0, int y0, const double *geom, FtpProjGeom &G, int &model)
{
    if (h < 0 || w < 0 || x0 < 0 || y0 < 0) return fail(SSAMD_EINVAL, "Wrong image dimensions or origin!");
    if (hp <= 0 || wp <= 0) return fail(SSAMD_EINVAL, "Wrong fringe dimensions!");
    if ((long long)h * w >= (1ll << 31)) return fail(SSAMD_EINVAL, "reference image of %d x %d pixels: 2^31 or more", h, w);
    if ((long long)hp * wp >= (1ll << 31)) return fail(SSAMD_EINVAL, "fringe of %d x %d pixels: 2^31 or more", hp, wp);
    if (!geom) return fail(SSAMD_EINVAL, "NULL buffer");
    for (int i = 0; i < (int)(sizeof(G) / sizeof(double)); ++i)
        if (!std::isfinite(geom[i])) return fail(SSAMD_EINVAL, "geom[%d] is not finite", i);
    std::memcpy(&G, geom, sizeof(G));
    auto any = [&](int a, int b) { for (int i = a; i < b; ++i) if (G.d[i] != 0) return true; return false; };
    model = any(8, 12) ? 3 : any(5, 8) ? 2 : any(0, 5) ? 1 : 0;
    return SSAMD_OK;
}

// the table goes up once per device, on the stream of the first call, which waits for it: every later call, on any stream,
// finds it complete
int ftp_reference_launch(Ctx &c, const uint8_t *d_fringe, int hp, int wp, int h, int w, int x0, int y0, const FtpProjGeom &G, int model,
                         uint8_t *d_out, hipStream_t s)
{
    if ((uintptr_t)d_out & 3) return fail(SSAMD_EINVAL, "the reference image buffer must be 4-byte aligned");
    if (!c.ftpRefTabReady) {
        int rc = c.ftpRefTab.reserve(FTP_REF_TAB * sizeof(short));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c.ftpRefTab.ptr, ftp_reference_table(), FTP_REF_TAB * sizeof(short), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        c.ftpRefTabReady = true;
    }
    const long long npix = (long long)h * w, quads = (npix + 3) / 4;
    const int blocks = (int)std::min<long long>((quads + FTP_REF_THREADS - 1) / FTP_REF_THREADS, (long long)c.cus * 2);
    Timed t(c, s, SSAMD_K_REMAP);
    static constexpr decltype(&ftp_reference_kernel<0>) kernels[4] = {ftp_reference_kernel<0>, ftp_reference_kernel<1>,
                                                                      ftp_reference_kernel<2>, ftp_reference_kernel<3>};
    hipLaunchKernelGGL(kernels[model & 3], dim3(blocks), dim3(FTP_REF_THREADS), 0, s, d_fringe, hp, wp, (const short *)c.ftpRefTab.ptr,
                       d_out, npix, w, x0, y0, G);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // namespace

extern "C" {
int ssamd_ftp_reference(const uint8_t *fringe, int hp, int wp, int h, int w, int x0, int y0, const double *geom, uint8_t *out, int device)
{
    FtpProjGeom G;
    int model;
    int rc = ftp_reference_check(hp, wp, h, w, x0, y0, geom, G, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!fringe || !out) return fail(SSAMD_EINVAL, "NULL buffer");
    return host_route(device, {{&Ctx::uwIn, fringe, (size_t)hp * wp}}, {&Ctx::uwOut, out, (size_t)h * w}, [&](Ctx &c, hipStream_t s) {
        return ftp_reference_launch(c, (const uint8_t *)c.uwIn.ptr, hp, wp, h, w, x0, y0, G, model, (uint8_t *)c.uwOut.ptr, s);
    });
}

int ssamd_ftp_reference_device(const uint8_t *d_fringe, int hp, int wp, int h, int w, int x0, int y0, const double *geom,
                               uint8_t *d_out, void *stream)
{
    FtpProjGeom G;
    int model;
    int rc = ftp_reference_check(hp, wp, h, w, x0, y0, geom, G, model);
    if (rc || h == 0 || w == 0) return rc;
    if (!d_fringe || !d_out) return fail(SSAMD_EINVAL, "NULL buffer");
    CtxLock c;
    if ((rc = get_ctx(-1, c))) return rc;
    return ftp_reference_launch(*c, d_fringe, hp, wp, h, w, x0, y0, G, model, d_out, (hipStream_t)stream);
}
}  // extern "C"
