// Host section of ssamd_api.hip: the rig's pointwise operators on device buffers (rig_kernels.hip.h) -- remap and reproject.
extern "C" {
int ssamd_remap_bgr_device(const uint8_t *d_src, int src_h, int src_w, const float *d_mapx, const float *d_mapy,
                           int dst_h, int dst_w, int interpolation, uint8_t *d_dst, void *stream)
{
    if (!d_src || !d_mapx || !d_mapy || !d_dst) return fail(SSAMD_EINVAL, "NULL buffer");
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    if (interpolation != 0 && interpolation != 1) return fail(SSAMD_EINVAL, "only INTER_NEAREST (0) and INTER_LINEAR (1) are supported");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)dst_h * dst_w;
    // (a thread owns four output pixels; the map and output pointers are 16- / 4-byte aligned: device allocations)
    if (((uintptr_t)d_mapx | (uintptr_t)d_mapy) & 15 || ((uintptr_t)d_dst & 3)) return fail(SSAMD_EINVAL, "maps must be 16-byte and the output 4-byte aligned");
    const int blocks = (int)std::min<long long>((npix / 4 + 255) / 256 + 1, 256 * 16);
    Timed t(*c, s, SSAMD_K_REMAP);
    hipLaunchKernelGGL(remap_bgr_kernel, dim3(blocks), dim3(256), 0, s, d_src, src_h, src_w, d_mapx, d_mapy, d_dst, npix,
                       interpolation == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}

int ssamd_reproject_device(const int16_t *d_disparity, int h, int w, const double *Q, float *d_points, void *stream)
{
    if (!d_disparity || !Q || !d_points) return fail(SSAMD_EINVAL, "NULL buffer");
    if (h <= 0 || w <= 0) return fail(SSAMD_EINVAL, "Wrong image dimensions!");
    CtxLock c;
    int rc = get_ctx(-1, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    Mat4 q;
    for (int k = 0; k < 16; ++k) q.m[k] = Q[k];
    if (h > 65535) return fail(SSAMD_ELIMIT, "more than 65535 rows");
    if ((w & 3) == 0 && (((uintptr_t)d_disparity & 7) || ((uintptr_t)d_points & 15)))
        return fail(SSAMD_EINVAL, "disparity / point buffers must be 8- / 16-byte aligned");
    const int per_row = (w & 3) == 0 ? w / 4 : w;                 // threads a row needs
    Timed t(*c, s, SSAMD_K_REPROJECT);
    hipLaunchKernelGGL(reproject_kernel, dim3((per_row + 255) / 256, h), dim3(256), 0, s, d_disparity, d_points, h, w, q);
    HIP_TRY(hipGetLastError());
    return SSAMD_OK;
}
}  // extern "C"
