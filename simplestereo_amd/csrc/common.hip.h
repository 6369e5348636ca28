// Shared device-side types for libssamd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssamd {

// One pixel as the ASW kernels consume it: CIELab (float32) + the raw BGR bytes
// packed in one dword (byte3 = 0), 16 B so that one global_load_dwordx4 / one
// ds_read_b128 moves a pixel.  Replaces the reference's separate u8 image and
// fp64 Lab image (_passive.cpp:333-341).
struct __attribute__((aligned(16))) PixRec {
    float L, a, b;
    uint32_t bgrx;
};

// The last two operations of an ASW support weight (_passive.cpp:47-50, 71-74): proximity weight x exp(-colour distance / gammaC).
// Every ASW kernel goes through this one function, so they stay bit-identical to each other.  (Round 3 measured the product folded
// into the exponent -- a table of log2 weights, one fused multiply-add, one VALU instruction less per weight: results within an ulp
// of the exponent, no golden figure changed, D 0..7 -2.4 %, D 0..192 +-0; left off as not worth a change of the weights' rounding.)
__device__ __forceinline__ float asw_weight_finish(float dist, float kC, float prox)
{
    return prox * __builtin_amdgcn_exp2f(dist * kC);
}

// The fp32 steps every ASW kernel family shares, each written once: the families agree bit for bit because they call these, not
// because copies of the arithmetic are kept in step.  (asw_exact_kernels.hip.h holds the fp64 twin of the weight.)

// Squared CIELab distance of a tap to its window centre (_passive.cpp:47-49 and 71-73); T, C: anything with the Lab values in .x .y .z
template <class T, class C>
__device__ __forceinline__ float asw_lab_dist2(const T &tp, const C &cen)
{
    const float dL = tp.x - cen.x, da = tp.y - cen.y, db = tp.z - cen.z;
    return fmaf(db, db, fmaf(da, da, dL * dL));
}

// The support weight of a tap (_passive.cpp:47-50, 71-74): v_sqrt_f32 of the squared distance, then asw_weight_finish; on staged
// Lab values and on pixel records
template <class T, class C>
__device__ __forceinline__ float asw_support_weight(const T &tp, const C &cen, float kC, float prox)
{
    return asw_weight_finish(__builtin_amdgcn_sqrtf(asw_lab_dist2(tp, cen)), kC, prox);
}
__device__ __forceinline__ float asw_support_weight(const PixRec &tp, const PixRec &cen, float kC, float prox)
{
    return asw_support_weight(make_float4(tp.L, tp.a, tp.b, 0.f), make_float4(cen.L, cen.a, cen.b, 0.f), kC, prox);
}
// A batch of N support weights from their squared distances, in place: the same two operations stage by stage (all square roots,
// then all exponentials and products), the order in which the batched builds hand their N independent chains to the scheduler.
// (kC by reference: the kernel argument is read where it is used, as in the statements this replaces; by value, one instance
// of the phase-shifted kernel allocated its scalar registers differently.)
template <int N>
__device__ __forceinline__ void asw_support_weights(float (&w)[N], const float &kC, const float (&prox)[N])
{
#pragma unroll
    for (int u = 0; u < N; ++u) w[u] = __builtin_amdgcn_sqrtf(w[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) w[u] = asw_weight_finish(w[u], kC, prox[u]);
}

// Truncated absolute difference min(40, |dB| + |dG| + |dR|) of two packed pixels (_passive.cpp:77-79): the bytes are B, G, R, 0,
// so one v_sad_u8 sums the three channels
__device__ __forceinline__ uint32_t asw_tad(uint32_t l, uint32_t r)
{
    return min(__builtin_amdgcn_sad_u8(l, r, 0u), 40u);
}

// The e-tile task "one left pixel x 8 disparities": the bytes of lo are the TADs of lp with rp[0], rp[-1], rp[-2], rp[-3]
// (disparities d .. d + 3 when rp points at R[u - d]), those of hi with rp[-4] .. rp[-7]
__device__ __forceinline__ void asw_tad8(uint32_t lp, const uint32_t *rp, uint32_t &lo, uint32_t &hi)
{
    lo = hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= asw_tad(lp, rp[-k]) << (8 * k);
        hi |= asw_tad(lp, rp[-4 - k]) << (8 * k);
    }
}

typedef unsigned long long u64;
static constexpr u64 KEY_NONE = ~0ull;

// WTA key: non-negative float cost bits in the high word (monotone as unsigned),
// candidate index in the low word, so that an unsigned 64-bit min implements
// "lowest cost, then lowest index" -- the reference's strict `<` scan keeps the
// first minimum, which is the smallest disparity in both passes
// (_passive.cpp:56,90-93 and 211,243-246).
__device__ __forceinline__ u64 make_key(float cost, uint32_t idx)
{
    return ((u64)__float_as_uint(cost) << 32) | (u64)idx;
}

}  // namespace ssamd
