// geo.hip -- libmi_nerf_geo.so (include/mi_nerf_geo.h): alpha compositing with the gradients the geometry losses need.  A library of its
// own: it shares stage_dev.h / common.h with libmi_nerf.so at compile time (the wave helpers, and so that the forward below can be held
// against composite_ray line by line) and nothing at link time.
//
//   geo_composite_kernel<C>            one 64-lane wavefront per ray, lane l owns samples [l*C, (l+1)*C): composite_ray's arithmetic
//                                      operation for operation (same bits), every output optional, plus THE DISTORTION RULE of the header
//   geo_composite_bwd_kernel<C, MODE>  composite_bwd_kernel of stages.hip with q_i = dL/dw_i widened by the new terms.  MODE 0: g_rgb alone,
//                                      the parent's expression; MODE 1: + g_acc, g_depth, g_weights (q_i changes, the scans do not);
//                                      MODE 2: + g_distortion (four more exclusive scans across the lanes for W<, W>, M<, M>)
//
// Forward quantities are recomputed in the backward; no LDS, no scratch, no atomic.  Compiled with -ffp-contract=off like stages.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_geo.h"
#include "abi_error.h"
#include "common.h"
#include "stage_dev.h"

namespace migeo {

using minerf::f32x4;
using minerf::wave_excl_prod;
using minerf::wave_excl_suffix_sum;
using minerf::wave_excl_sum;
using minerf::wave_sum;

// ---- error plumbing (abi_error.h): the library's one buffer; lattice_reg.hip reaches set_error / hip_fail, which the library does not export
ABI_ERROR_STATE(__attribute__((visibility("hidden"))), MI_GEO_EHIP)
#define GEO_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::migeo, MI_GEO_EINVAL, cond, __VA_ARGS__)
#define GEO_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::migeo, name)

// THE DISTORTION RULE, the interval half: t_i, delta_i, m_i of one sample from its depth and the next one's (zn == zv for the last sample)
__device__ __forceinline__ void interval(float zv, float zn, float near_, float span, float& m, float& delta) {
    const float t0 = (zv - near_) / span, t1 = (zn - near_) / span;
    delta = t1 - t0;
    m = t0 + 0.5f * delta;
}

// ... the pair half: pt_i = m_i (W<_i - W>_i) - (M<_i - M>_i) for the lane's C samples.  Per lane the sums of w and w m, exclusive prefix and
// suffix scans of both across the lanes, then one ascending and one descending walk over the lane's own samples.  A sample beyond S has w = 0.
template <int C>
__device__ __forceinline__ void pair_terms(const float (&w)[C], const float (&m)[C], int lane, float (&pt)[C]) {
    float lw = 0.0f, lm = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) { lw += w[c]; lm += w[c] * m[c]; }
    float Wlt = wave_excl_sum(lw, lane), Mlt = wave_excl_sum(lm, lane);
    float Wgt = wave_excl_suffix_sum(lw, lane), Mgt = wave_excl_suffix_sum(lm, lane);
    float wl[C], ml[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        wl[c] = Wlt; ml[c] = Mlt;
        Wlt += w[c]; Mlt += w[c] * m[c];
    }
#pragma unroll
    for (int c = C - 1; c >= 0; --c) {
        pt[c] = m[c] * (wl[c] - Wgt) - (ml[c] - Mgt);
        Wgt += w[c]; Mgt += w[c] * m[c];
    }
}

// ------------------------------------------------------------------------------------------------
// forward: composite_ray (stage_dev.h) with optional outputs, and the distortion loss
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void geo_composite_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                             const float* __restrict__ rays, int ray_stride, long long n, int S, float near_,
                                                             float span, float* __restrict__ rgb_o, float* __restrict__ disp_o,
                                                             float* __restrict__ acc_o, float* __restrict__ w_o, float* __restrict__ depth_o,
                                                             float* __restrict__ dist_o) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n) return;
    const float* dp = rays + ray * ray_stride + (ray_stride == 6 ? 3 : 0);
    const float dx = dp[0], dy = dp[1], dz = dp[2];
    const float dnorm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    const float* zr = z + ray * S;
    const f32x4* rr = (const f32x4*)(raw + ray * S * 4);

    float alpha[C], zv[C], cr[C], cg[C], cb[C], mv[C], dl[C];
    float local = 1.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int s = lane * C + c;
        const bool in = s < S;
        const int sc = in ? s : S - 1;
        const f32x4 v = rr[sc];
        zv[c] = zr[sc];
        const float zn = (s + 1 < S) ? zr[s + 1] : zv[c];
        float dist = (s + 1 < S) ? (zn - zv[c]) : 1e10f;
        dist = dist * dnorm;
        const float sig = __builtin_fmaxf(v[3], 0.0f);
        float a = 1.0f - expf(-sig * dist);
        if (!in || S == 1) a = 0.0f;
        alpha[c] = a;
        cr[c] = 1.0f / (1.0f + expf(-v[0]));
        cg[c] = 1.0f / (1.0f + expf(-v[1]));
        cb[c] = 1.0f / (1.0f + expf(-v[2]));
        local *= in ? (1.0f - a + 1e-10f) : 1.0f;
        interval(zv[c], zn, near_, span, mv[c], dl[c]);
    }
    float T = wave_excl_prod(local, lane);
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f;
    float w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int s = lane * C + c;
        w[c] = alpha[c] * T;
        if (s < S) {
            if (w_o) w_o[ray * S + s] = w[c];
            sw += w[c]; sr += w[c] * cr[c]; sg += w[c] * cg[c]; sb += w[c] * cb[c]; sd += w[c] * zv[c];
        }
        T *= (1.0f - alpha[c] + 1e-10f);
    }
    sw = wave_sum(sw); sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sd = wave_sum(sd);
    float dsum = 0.0f;
    if (dist_o) {                                                            // wave-uniform
        float pt[C];
        pair_terms<C>(w, mv, lane, pt);
#pragma unroll
        for (int c = 0; c < C; ++c) dsum += w[c] * pt[c] + (1.0f / 3.0f) * (w[c] * w[c] * dl[c]);
        dsum = wave_sum(dsum);
    }
    if (lane == 0) {
        const float q = sd / sw;
        const float m = (q != q) ? q : __builtin_fmaxf(1e-10f, q);
        float disp = 1.0f / m;
        if (disp != disp) disp = 0.0f;
        if (disp > 5.0f) disp = 5.0f;
        const float bg = 1.0f - sw;
        if (rgb_o) { rgb_o[ray * 3 + 0] = sr + bg; rgb_o[ray * 3 + 1] = sg + bg; rgb_o[ray * 3 + 2] = sb + bg; }
        if (disp_o) disp_o[ray] = disp;
        if (acc_o) acc_o[ray] = sw;
        if (depth_o) depth_o[ray] = sd;
        if (dist_o) dist_o[ray] = dsum;
    }
}

// ------------------------------------------------------------------------------------------------
// backward: (g_rgb, g_acc, g_depth, g_distortion, g_weights) -> d_raw.  The structure of composite_bwd_kernel (stages.hip); every new
// loss enters through q_i alone.
// ------------------------------------------------------------------------------------------------
struct GeoGrads { const float *rgb, *acc, *depth, *dist, *w; };

template <int C, int MODE>
__global__ __launch_bounds__(256) void geo_composite_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                 const float* __restrict__ rays, int ray_stride, long long n, int S,
                                                                 float near_, float span, GeoGrads g, float* __restrict__ d_raw) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n) return;
    const float* dp = rays + ray * ray_stride + (ray_stride == 6 ? 3 : 0);
    const float dx = dp[0], dy = dp[1], dz = dp[2];
    const float dnorm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    const float* zr = z + ray * S;
    const f32x4* rr = (const f32x4*)(raw + ray * S * 4);
    f32x4* out = (f32x4*)(d_raw + ray * S * 4);
    const float Gr = g.rgb ? g.rgb[ray * 3 + 0] : 0.0f, Gg = g.rgb ? g.rgb[ray * 3 + 1] : 0.0f, Gb = g.rgb ? g.rgb[ray * 3 + 2] : 0.0f;

    float alpha[C], dads[C], cr[C], cg[C], cb[C];
    float zv[MODE >= 1 ? C : 1], mv[MODE == 2 ? C : 1], dl[MODE == 2 ? C : 1];
    float local = 1.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int s = lane * C + c;
        const bool in = s < S;
        const int sc = in ? s : S - 1;
        const f32x4 v = rr[sc];
        const float z0 = zr[sc];
        const float zn = (s + 1 < S) ? zr[s + 1] : z0;
        float dist = (s + 1 < S) ? (zn - z0) : 1e10f;
        dist = dist * dnorm;
        const float sig = __builtin_fmaxf(v[3], 0.0f);
        const float e = expf(-sig * dist);
        float a = 1.0f - e;
        float ds = (v[3] > 0.0f) ? dist * e : 0.0f;
        if (!in || S == 1) { a = 0.0f; ds = 0.0f; }
        alpha[c] = a;
        dads[c] = ds;
        cr[c] = 1.0f / (1.0f + expf(-v[0]));
        cg[c] = 1.0f / (1.0f + expf(-v[1]));
        cb[c] = 1.0f / (1.0f + expf(-v[2]));
        local *= in ? (1.0f - a + 1e-10f) : 1.0f;
        if constexpr (MODE >= 1) zv[c] = z0;
        if constexpr (MODE == 2) interval(z0, zn, near_, span, mv[c], dl[c]);
    }
    float T = wave_excl_prod(local, lane);
    float Tc[C], q[C], w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        Tc[c] = T;
        w[c] = alpha[c] * T;
        q[c] = Gr * (cr[c] - 1.0f) + Gg * (cg[c] - 1.0f) + Gb * (cb[c] - 1.0f);
        T *= (1.0f - alpha[c] + 1e-10f);
    }
    // The part of q that is the same for every sample of the ray, q0 = G_acc + G_depth z_0, is taken out of q and through the formula in
    // closed form.  With w_k = T_k - T_{k+1} + 1e-10 T_k (T_{k+1} = u_k T_k) the suffix sum telescopes:
    //     q0 (T_i - (sum_{k>i} w_k) / u_i) = q0 (T_S - 1e-10 sum_{k>i} T_k) / u_i,    T_S the product over all samples.
    // Left in q it is the difference of two numbers near T_i that is as small as T_S: on a ray that ends opaque the rounding of the 1024-term
    // suffix sum is then as large as the result (1.0e-4 of the largest entry at 2 x 1024 with g_acc alone, measured against float64 autograd).
    float q0 = 0.0f, T_end = 0.0f, Tgt = 0.0f;
    if constexpr (MODE >= 1) {
        const float Ga = g.acc ? g.acc[ray] : 0.0f, Gd = g.depth ? g.depth[ray] : 0.0f;
        const float z_first = zr[0];
        q0 = Ga + Gd * z_first;
        float lT = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int s = lane * C + c;
            const float gw = (g.w && s < S) ? g.w[ray * S + s] : 0.0f;
            q[c] = q[c] + Gd * (zv[c] - z_first) + gw;
            lT += (s < S) ? Tc[c] : 0.0f;
        }
        T_end = __shfl(T, 63, 64);                   // lane 63 has walked to the end of the ray (a sample beyond S leaves T as it is)
        Tgt = wave_excl_suffix_sum(lT, lane);        // sum of T_k over the samples owned by higher lanes
    }
    if constexpr (MODE == 2) {
        const float Gx = g.dist[ray];
        float pt[C];
        pair_terms<C>(w, mv, lane, pt);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = q[c] + Gx * (2.0f * pt[c] + (2.0f / 3.0f) * (w[c] * dl[c]));
    }
    float lsum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) lsum += q[c] * w[c];
    float R = wave_excl_suffix_sum(lsum, lane);     // sum over the samples owned by higher lanes
#pragma unroll
    for (int c = C - 1; c >= 0; --c) {
        const int s = lane * C + c;
        const float u = 1.0f - alpha[c] + 1e-10f;
        float dLda = q[c] * Tc[c] - R / u;
        R += q[c] * w[c];
        if constexpr (MODE >= 1) {
            dLda += q0 * ((T_end - 1e-10f * Tgt) / u);
            Tgt += (s < S) ? Tc[c] : 0.0f;
        }
        if (s < S) {
            f32x4 o;
            o[0] = Gr * w[c] * cr[c] * (1.0f - cr[c]);
            o[1] = Gg * w[c] * cg[c] * (1.0f - cg[c]);
            o[2] = Gb * w[c] * cb[c] * (1.0f - cb[c]);
            o[3] = dLda * dads[c];
            out[s] = o;
        }
    }
}

// what both entries check before any HIP call
static int check_common(const char* who, const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int S, float near_,
                        float far_) {
    GEO_CHECK_ARG(n >= 0 && n <= (int64_t)4 * 0x7fffffff, "%s: n=%lld: 0 .. 4 (2^31 - 1)", who, (long long)n);
    GEO_CHECK_ARG(S >= 1 && S <= MI_GEO_MAX_SAMPLES, "%s: S=%d: 1..%d", who, S, MI_GEO_MAX_SAMPLES);
    GEO_CHECK_ARG(ray_stride == 3 || ray_stride == 6, "%s: ray_stride=%d must be 3 or 6", who, ray_stride);
    GEO_CHECK_ARG(isfinite(near_) && isfinite(far_) && near_ < far_, "%s: near=%g must be below far=%g, both finite", who, (double)near_, (double)far_);
    GEO_CHECK_ARG(isfinite(far_ - near_) && far_ - near_ > 0.0f, "%s: far - near = %g is not a positive finite fp32 number", who, (double)(far_ - near_));
    GEO_CHECK_ARG(n == 0 || (raw != nullptr && z != nullptr && rays != nullptr), "%s: raw / z / rays is NULL", who);
    GEO_CHECK_ARG(((uintptr_t)raw & 15) == 0, "%s: raw must be 16-byte aligned", who);
    return MI_GEO_OK;
}

}  // namespace migeo

using namespace migeo;

extern "C" {

int mi_geo_abi_version(void) { return MI_GEO_ABI_VERSION; }
const char* mi_geo_last_error(void) { return g_err; }

int mi_geo_composite(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int S, float near_, float far_, float* rgb,
                     float* disp, float* acc, float* weights, float* depth, float* distortion, void* stream) {
    const int rc = check_common("mi_geo_composite", raw, z, rays, ray_stride, n, S, near_, far_);
    if (rc != MI_GEO_OK) return rc;
    if (n == 0) return MI_GEO_OK;
    const dim3 grid(blocks_for(n, 4)), block(256);
    const float span = far_ - near_;
    const int C = (S + 63) / 64;
#define GEO_COMP(CC)                                                                                                                           \
    hipLaunchKernelGGL(geo_composite_kernel<CC>, grid, block, 0, (hipStream_t)stream, raw, z, rays, ray_stride, (long long)n, S, near_, span, rgb, \
                       disp, acc, weights, depth, distortion)
    if (C == 1) GEO_COMP(1); else if (C == 2) GEO_COMP(2); else if (C == 3) GEO_COMP(3); else if (C == 4) GEO_COMP(4);
    else if (C <= 8) GEO_COMP(8); else GEO_COMP(16);
#undef GEO_COMP
    GEO_LAUNCH_CHECK("geo_composite_kernel");
    return MI_GEO_OK;
}

int mi_geo_composite_backward(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int S, float near_, float far_,
                              const float* g_rgb, const float* g_acc, const float* g_depth, const float* g_distortion, const float* g_weights,
                              float* d_raw, void* stream) {
    const int rc = check_common("mi_geo_composite_backward", raw, z, rays, ray_stride, n, S, near_, far_);
    if (rc != MI_GEO_OK) return rc;
    GEO_CHECK_ARG(n == 0 || d_raw != nullptr, "mi_geo_composite_backward: d_raw is NULL");
    GEO_CHECK_ARG(((uintptr_t)d_raw & 15) == 0, "mi_geo_composite_backward: d_raw must be 16-byte aligned");
    if (n == 0) return MI_GEO_OK;
    if (!g_rgb && !g_acc && !g_depth && !g_distortion && !g_weights) {      // no gradient at all: zeros, without reading anything
        const hipError_t e = hipMemsetAsync(d_raw, 0, (size_t)n * S * 4 * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(d_raw)");
        return MI_GEO_OK;
    }
    const dim3 grid(blocks_for(n, 4)), block(256);
    const float span = far_ - near_;
    const GeoGrads g{g_rgb, g_acc, g_depth, g_distortion, g_weights};
    const int C = (S + 63) / 64;
    const int mode = g_distortion ? 2 : (g_acc || g_depth || g_weights) ? 1 : 0;
#define GEO_BWD(CC, MM)                                                                                                                       \
    hipLaunchKernelGGL((geo_composite_bwd_kernel<CC, MM>), grid, block, 0, (hipStream_t)stream, raw, z, rays, ray_stride, (long long)n, S, near_, \
                       span, g, d_raw)
#define GEO_BWD_C(MM)                                                                                                  \
    do {                                                                                                               \
        if (C == 1) GEO_BWD(1, MM); else if (C == 2) GEO_BWD(2, MM); else if (C == 3) GEO_BWD(3, MM);                   \
        else if (C == 4) GEO_BWD(4, MM); else if (C <= 8) GEO_BWD(8, MM); else GEO_BWD(16, MM);                         \
    } while (0)
    if (mode == 0) GEO_BWD_C(0); else if (mode == 1) GEO_BWD_C(1); else GEO_BWD_C(2);
#undef GEO_BWD_C
#undef GEO_BWD
    GEO_LAUNCH_CHECK("geo_composite_bwd_kernel");
    return MI_GEO_OK;
}

}  // extern "C"
