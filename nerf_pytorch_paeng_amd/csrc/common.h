// common.h -- libmi_nerf.so's names for the error plumbing of abi_error.h, and small device helpers shared by all translation units.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include "../../include/mi_nerf.h"
#include "abi_error.h"

namespace minerf {

// libmi_nerf.so's one message buffer lives in api.hip (ABI_ERROR_STATE of abi_error.h); every translation unit writes it through these
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define MN_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::minerf, MI_NERF_EINVAL, cond, __VA_ARGS__)
#define MN_HIP(call) ABI_HIP(::minerf, call, #call)
#define MN_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::minerf, name)

// Per-DEVICE launch state (a process may drive several GPUs: the 160 KB dynamic-LDS opt-in is an attribute of the function ON a
// device, and the CU count is a property of the device): small arrays indexed by the current device ordinal.
// The entry points are re-entrant per stream and callable from several host threads: the only state the library keeps between calls are
// these per-device words, atomics written with the same value by whoever gets there first (hipFuncSetAttribute is idempotent), and the
// thread-local error text.  tests/test_gpu_streams.py.
constexpr int MN_MAX_DEVICES = 64;
struct LdsOptIn { std::atomic<bool> done[MN_MAX_DEVICES]; };
int device_cus();                                             // multiProcessorCount of the current device (cached per device)
int ensure_lds_opt_in(LdsOptIn& state, const void* kernel);  // hipFuncSetAttribute(MaxDynamicSharedMemorySize = 160 KB), once per device
// grid of a persistent kernel: one workgroup per CU, fewer when the launch has fewer workgroups' worth of work
static inline int persistent_grid(long long n_wg) { const long long cus = device_cus(); return (int)(n_wg < cus ? n_wg : cus); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// An MFMA written as an asm statement keeps WRITING its destination tuple until P + 4 wait states after issue (8-pass 16x16x32: 12), and hipcc
// does not know: an element of the tuple that no later code reads is free for the allocator the moment the statement ends, and whatever
// lands there first (an address, a shuffle result) is overwritten when the matrix result arrives.  That took down round 3's NOPACK ablation
// build and sat as a 1-2 wait-state near miss in the shipped STASH kernel (colour tile element 3 vs. a ds_bpermute of
// finish_masks).  Rule: every tuple with elements the code does not read (density tile: only [3]; colour tile: only [0..2]) is named whole by
// keep_tuple() at a point >= 12 wait states behind its last MFMA.  tools/mfma_hazard_check.py checks the objects (tests/test_packing_cpu.py).
__device__ __forceinline__ void keep_tuple(const f32x4& x) { asm volatile("" ::"v"(x)); }

// ---------------------------------------------------------------------------------------------
// counter-based uniform generator (numpy mirror: oracle/restate.py counter_uniform)
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ inline float counter_uniform(uint32_t seed, uint32_t stream_id, uint32_t ray, uint32_t sample) {
    uint32_t h = fmix32(ray + 0x9E3779B9u * seed + 0x632BE5ABu);
    h = fmix32(h ^ (sample * 0x85EBCA6Bu + stream_id * 0xC2B2AE35u + 0x27D4EB2Fu));
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// ---------------------------------------------------------------------------------------------
// stratified coarse depths and their jitter (stages.hip: stratified_kernel; mlp_bf16.hip draws them in its own prologue)
// ---------------------------------------------------------------------------------------------
// torch.linspace(0,1,S)[i] in fp32 (symmetric fill: ATen RangeFactories) and z = near*(1-t) + far*t
__device__ __forceinline__ float strat_edge(int i, int S, float step, float near_, float far_) {
    const float t = (S == 1) ? 0.0f : (i < S / 2) ? step * (float)i : 1.0f - step * (float)(S - 1 - i);   // steps=1 -> [start]
    return near_ * (1.0f - t) + far_ * t;               // nerf_process.py:53
}

// Where a stage's uniforms come from: an explicit [n, S] tensor (injected randomness: parity tests, the training path), or -- values ==
// NULL -- the counter-based generator evaluated in the consuming kernel itself, keyed on (seed, stream, ray0 + ray, sample): the
// values mi_nerf_fill_uniform would have written, without the tensor, its launch or its HBM round trip.
struct Jitter {
    const float* values;
    uint32_t seed, stream;
    long long ray0;
};
__device__ __forceinline__ float jitter_at(const Jitter& j, long long ray, int sample, int S) {
    return j.values ? j.values[ray * S + sample] : counter_uniform(j.seed, j.stream, (uint32_t)(j.ray0 + ray), (uint32_t)sample);
}

// what a kernel needs to draw the coarse depths itself (host side of mlp_rays_bf16's strat argument)
struct StratDraw { float near_, far_; const float* t_rand; uint32_t seed; int64_t ray0; float* z_out; };
// what the bf16 coarse launch needs to ALSO do render_rays' middle (composite the coarse pass, resample, merge: stage_composite_fine_z) for the
// rays its workgroups wholly own -- offered by mi_nerf_render_rays, taken by mlp_rays_bf16 only for small launches (`taken` says which)
struct FineDraw { int Nf, det; const float* u; uint32_t seed; int64_t ray0; float *rgb_c, *disp_c, *w_c, *z_f; bool taken; };
// one stratified coarse depth (nerf_process.py:42-60): sample i of S on ray `ray`
__device__ __forceinline__ float stratified_depth(long long ray, int i, int S, float step, float near_, float far_, const Jitter& t_rand) {
    const float zi = strat_edge(i, S, step, near_, far_);
    const float lower = (i == 0) ? zi : 0.5f * (zi + strat_edge(i - 1, S, step, near_, far_));       // :55,57
    const float upper = (i == S - 1) ? zi : 0.5f * (strat_edge(i + 1, S, step, near_, far_) + zi);   // :55,56
    return lower + (upper - lower) * jitter_at(t_rand, ray, i, S);     // :60
}

// ---------------------------------------------------------------------------------------------
// accurate sin / cos for positional encoding.  Arguments are 2^k * x (exact in fp32) and reach
// ~3e3 rad for lego, so the reduction matters: 3-term Cody-Waite with FMA (pi/2 = HI + MID + LO),
// then the Cephes single-precision minimax polynomials on [-pi/4, pi/4].
// quad_shift 0 -> sin(y), 1 -> cos(y) (cos y = sin(y + pi/2): same reduction, next quadrant).
// Accuracy: |error| <= 1.3e-7 for |y| < 2^20 (measured against float64, tests/test_gpu_far_points.py: 9.3e-8 up to 2^19, 1.2e-7 in
// [2^19, 2^20)).  The weak point is the multiple count: nf = rint(y * 2/pi) is an fp32 product, whose ulp is 2^-5 at 2^19 and 0.25 at
// 4e6, so nf is off by one over a growing share of each quadrant, |r| exceeds pi/4 (0.88 at 2^20, 0.97 at 2^21, 1.14 at 4e6) and the
// polynomials leave their interval: 3.7e-7 in [2^20, 2^21), 2.8e-6 up to 4e6.  The subtraction itself stays exact far beyond.
// Hence the limit below: from 2^20 on callers take the libm path.
// ---------------------------------------------------------------------------------------------
// The three stages are separate functions so that a caller can spread one evaluation over several instruction groups
// (mlp_fp32.hip computes the NEXT tile's gamma(x) under the current tile's MFMAs); sin_cos_fast is their composition.
__device__ __forceinline__ void sc_reduce(float y, int quad_shift, float& r, int& q) {      // Cody-Waite, 3 terms
    const float nf = __builtin_rintf(y * 0.636619772367581343f);
    r = __builtin_fmaf(-nf, 1.57079637050628662109375f, y);
    r = __builtin_fmaf(-nf, -4.371138828673793e-08f, r);
    r = __builtin_fmaf(-nf, -1.7151245100058819e-15f, r);
    q = (int)nf + quad_shift;
}
__device__ __forceinline__ void sc_poly_sin(float r, float& r2, float& sp) {               // Cephes sinf kernel
    r2 = r * r;
    sp = __builtin_fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
    sp = __builtin_fmaf(sp, r2, -1.6666654611e-1f);
    sp = __builtin_fmaf(sp * r2, r, r);
}
__device__ __forceinline__ void sc_poly_cos(float r2, float& cp) {                          // Cephes cosf kernel
    cp = __builtin_fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
    cp = __builtin_fmaf(cp, r2, 4.166664568298827e-2f);
    cp = __builtin_fmaf(cp * r2, r2, __builtin_fmaf(-0.5f, r2, 1.0f));
}
__device__ __forceinline__ void sc_poly(float r, float& sp, float& cp) {
    float r2;
    sc_poly_sin(r, r2, sp);
    sc_poly_cos(r2, cp);
}
__device__ __forceinline__ float sc_select(float sp, float cp, int q) {
    const float v = (q & 1) ? cp : sp;
    return (q & 2) ? -v : v;
}
__device__ __forceinline__ float sin_cos_fast(float y, int quad_shift) {
    float r, sp, cp;
    int q;
    sc_reduce(y, quad_shift, r, q);
    sc_poly(r, sp, cp);
    return sc_select(sp, cp, q);
}
// |y| below this bound keeps the multiple count close enough for the accuracy stated above; callers branch ONCE per point on the
// largest argument and use the libm path (sinf/cosf, Payne-Hanek) for anything bigger or non-finite.  (4e6 until the far-point tests.)
constexpr float SINCOS_FAST_LIMIT = 1048576.0f;      // 2^20
__device__ __forceinline__ float sin_cos_slow(float y, int quad_shift) { return quad_shift ? cosf(y) : sinf(y); }
__device__ __forceinline__ float sin_cos_any(float y, bool fast, int quad_shift) { return fast ? sin_cos_fast(y, quad_shift) : sin_cos_slow(y, quad_shift); }

// ---------------------------------------------------------------------------------------------
// the ray prologue of the fused MLP kernels (mlp_fp32.hip, mlp_fp32_wide.hip, mlp_half_core.h, mlp_f16s_core.h)
// ---------------------------------------------------------------------------------------------
// pts = rays_o + rays_d * z : separate multiply and add (nerf_process.py:69-70), no contraction
__device__ __forceinline__ void sample_point(float (&pt)[3], const float (&o)[3], const float (&d)[3], float z) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pt[c] = o[c] + d[c] * z;
}
// the ONE branch per point: every argument 2^k pt_c, k < LX, is below SINCOS_FAST_LIMIT (false for huge or non-finite coordinates: libm path)
template <int LX>
__device__ __forceinline__ bool point_is_fast(const float (&pt)[3]) {
    const float amax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(pt[0]), __builtin_fabsf(pt[1])), __builtin_fabsf(pt[2])) * (float)(1 << (LX - 1));
    return amax < SINCOS_FAST_LIMIT;
}
// sin / cos of 2^k pt_c, every channel evaluated on its own (the argument is exact: a power-of-two scale)
template <int LX>
__device__ __forceinline__ void sincos_octaves(const float (&pt)[3], bool fast, float (&sn)[LX][3], float (&cs)[LX][3]) {
#pragma unroll
    for (int k = 0; k < LX; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = pt[c] * (float)(1 << k);
            sn[k][c] = sin_cos_any(y, fast, 0);
            cs[k][c] = sin_cos_any(y, fast, 1);
        }
}
// channel u of gamma(x) in the reference's order (PositionalEncoding.py:18-24), zero beyond the last; u is a constant at every use
template <int LX>
__device__ __forceinline__ float gamma_channel(int u, const float (&pt)[3], const float (&sn)[LX][3], const float (&cs)[LX][3]) {
    if (u >= 3 + 6 * LX) return 0.0f;
    if (u < 3) return pt[u];
    const int k = (u - 3) / 6, r = (u - 3) % 6;
    return r < 3 ? sn[k][r] : cs[k][r - 3];
}
// hoisted view-direction term of linear_d (fp32), constant over a ray's samples: dst[n] = b_d[n] + sum_f Wd[n][W + f] * gamma(d / |d|)[f] for the
// W / 2 outputs, lane `lane` of the wave taking n = lane, lane + 64, ...  wdt: that block of Wd transposed, [3 + 6 LD][W / 2]; all three in LDS.
template <int W, int LD>
__device__ __forceinline__ void hoisted_dir_bias(float* dst, float dx, float dy, float dz, const float* wdt, const float* bd, int lane) {
    constexpr int IN_D = 3 + 6 * LD;
    const float nrm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    const float v[3] = {dx / nrm, dy / nrm, dz / nrm};
    float g[IN_D];
    g[0] = v[0]; g[1] = v[1]; g[2] = v[2];
#pragma unroll
    for (int k = 0; k < LD; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = v[c] * (float)(1 << k);
            g[3 + 6 * k + c] = sin_cos_fast(y, 0);       // |y| <= 2^(LD-1): no fallback needed
            g[3 + 6 * k + 3 + c] = sin_cos_fast(y, 1);
        }
#pragma unroll
    for (int n0 = 0; n0 < W / 2; n0 += 64) {
        const int n = n0 + lane;
        float s = bd[n];
#pragma unroll
        for (int f = 0; f < IN_D; ++f) s = __builtin_fmaf(wdt[f * (W / 2) + n], g[f], s);
        dst[n] = s;
    }
}

}  // namespace minerf
