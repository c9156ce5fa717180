// voxgrad.hip -- libmi_nerf_voxgrad.so (include/mi_nerf_voxgrad.h): the backward pass of the radiance-grid renderer.  A library of its
// own: it shares abi_error.h with the others, and vox_rule.h (the rule's building blocks in device code, the grid and march checks) with
// vox.hip, at compile time and nothing at link time.
//
//   backward_kernel<B>     the forward's shape: a GROUP OF 8 LANES PER RAY, 32 rays per workgroup, lane e owns corner e of the sample's
//                          cell, sums over the group with DPP row operations, no LDS.  All control flow but the adds themselves is uniform
//                          within a group.
//                          March 1 is THE RENDER RULE of include/mi_nerf_vox.h as csrc/vox.hip evaluates it, operation by operation (the
//                          rgb / acc / depth check outputs hold this copy to that renderer bit for bit), and sums S = sum w_k s_k.
//                          March 2 walks the same samples front to back with the running prefix P and the transmittance T, evaluates the
//                          colour at every sample (also where sigma_s == 0), and forms dL/d sigma_s and dL/d q[c].  It does not jump: with
//                          use_skip it reads the block byte of every sample's cell, which is the header's rule per sample.
//                          Consecutive samples of a ray share a cell (the default step is half a cell): lane e keeps FOUR partial sums
//                          while the cell is unchanged -- sum w_e dL/d sigma_s and sum w_e dL/d q[c], c = 0..2 -- and flushes on a cell
//                          change and at the end: one add into d_sigma and 3 B adds Y_b * (sum of channel c) into its corner's record.
//                          Y_b is constant along the ray, so the 3 B sums of the rule collapse into 3 registers.  A value that is exactly
//                          0 issues no add: a sample with w_k == 0 costs no coefficient traffic.
//                          The adds are fp32 hardware atomics without return (global_atomic_add_f32): the one entry of the project whose
//                          result depends on arrival order in its last bits.
//                          The rule's domain is a signed plane as well (the header's Signed paragraph): both marches take
//                          sigma_s = fmaxf(the group's sum, 0), and march 2 adds w_e dL/d sigma_s only where that sum is >= 0.  On a plane
//                          that is >= 0 neither changes a bit.
//
// No host synchronisation, no copy, no allocation.  Compiled with -ffp-contract=off: the rule is evaluated as it is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/mi_nerf_voxgrad.h"
#include "abi_error.h"
#define VOX_RULE_NAMESPACE mivoxgrad
#include "vox_rule.h"

namespace mivoxgrad {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_VOXGRAD_EHIP)
#define VG_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mivoxgrad, MI_VOXGRAD_EINVAL, cond, __VA_ARGS__)
#define VG_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mivoxgrad, name)

static_assert(BLK == MI_VOXGRAD_BLOCK, "vox_rule.h and mi_nerf_voxgrad.h disagree on the block edge");

struct BackArgs {
    Lattice g;
    const float* sigma;
    const float4* coef;
    const uint8_t* skip;
    const float* rays;
    long long n;
    float step, t_near, t_far, T_min;
    float bg[3];
    int use_skip;
    int max_steps;
    const float *g_rgb, *g_acc, *g_depth;
    float *d_sigma, *d_coef;
    float *rgb, *acc, *depth;                            // the check outputs
};

// interval k of a ray: a_k < t1 decides whether it exists; the cell and the fractions of its midpoint
struct Sample {
    float ak, bk, mk;
    int c[3];
    float f[3];
};

__device__ __forceinline__ bool interval(const Lattice& g, const float (&o)[3], const float (&d)[3], float t0, float t1, float dt, int k, Sample& s) {
    s.ak = t0 + (float)k * dt;
    if (!(s.ak < t1)) return false;
    s.bk = fminf(t0 + (float)(k + 1) * dt, t1);
    s.mk = 0.5f * (s.ak + s.bk);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float p = o[i] + s.mk * d[i];
        const float gi = (p - g.lo[i]) * g.inv[i];
        s.c[i] = min(max((int)floorf(gi), 0), g.res[i] - 1);
        s.f[i] = fminf(fmaxf(gi - (float)s.c[i], 0.0f), 1.0f);
    }
    return true;
}

// lane e's share w_e * q_e[ch] of the pre-clamp colour: the basis applied to its corner's record, in increasing b
template <int B>
__device__ __forceinline__ void corner_colour(const float4* __restrict__ coef, long long at, const float (&Y)[B], float w, float (&wq)[3]) {
    float kc[record_regs<B, DENSE>()];
    fetch_record<B, DENSE>(coef, nullptr, 0, at, kc);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float q = kc[ch] * Y[0];
#pragma unroll
        for (int b = 1; b < B; ++b) q += kc[3 * b + ch] * Y[b];
        wq[ch] = w * q;
    }
}

// a lane's partial sums of one cell go out: one add into d_sigma, 3 B into the corner's record; zeros are not added
template <int B>
__device__ __forceinline__ void flush(const BackArgs& a, long long at, const float (&Y)[B], float ps, const float (&pc)[3]) {
    if (ps != 0.0f) atomicAdd(a.d_sigma + at, ps);
    float* rec = a.d_coef + at * record_floats(B);
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = Y[b] * pc[ch];
            if (v != 0.0f) atomicAdd(rec + 3 * b + ch, v);
        }
    }
}

template <int B>
__global__ __launch_bounds__(THREADS) void backward_kernel(const BackArgs a) {
    const int e = threadIdx.x & (GROUP - 1);               // this lane's corner
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 3);
    if (ray >= a.n) return;                                // a whole group leaves together
    const Lattice& g = a.g;
    const float* rp = a.rays + ray * 6;
    const float o[3] = {rp[0], rp[1], rp[2]}, d[3] = {rp[3], rp[4], rp[5]};
    const float L = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    bool miss = !(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(L)) || L == 0.0f;
    float entry = -INFINITY, exit_ = INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (d[i] != 0.0f) {
            const float ta = (g.lo[i] - o[i]) / d[i], tb = (g.hi[i] - o[i]) / d[i];
            entry = fmaxf(entry, fminf(ta, tb));
            exit_ = fminf(exit_, fmaxf(ta, tb));
        } else if (!(g.lo[i] <= o[i] && o[i] <= g.hi[i])) {
            miss = true;
        }
    }
    const float t0 = fmaxf(a.t_near, entry), t1 = fminf(a.t_far, exit_);
    if (!(t1 > t0)) miss = true;
    // upstream
    const float G[3] = {a.g_rgb[ray * 3 + 0], a.g_rgb[ray * 3 + 1], a.g_rgb[ray * 3 + 2]};
    const float ga = a.g_acc ? a.g_acc[ray] : 0.0f, gd = a.g_depth ? a.g_depth[ray] : 0.0f;
    const float gap = ga - ((G[0] * a.bg[0] + G[1] * a.bg[1]) + G[2] * a.bg[2]);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    if (!miss) {
        const float dt = a.step / L;
        const float ux = d[0] / L, uy = d[1] / L, uz = d[2] / L;
        float Y[B];
        sh_basis<B>(ux, uy, uz, Y);
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        // ---- march 1: the forward, and S ------------------------------------------------------------------
        // jumping over an empty block: allowed only where the fp32 position error stays below an eighth of a cell
        const float tmax = fmaxf(fabsf(t0), fabsf(t1));
        float gu[3], gv[3];
        bool can_jump = a.use_skip != 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gu[i] = (o[i] - g.lo[i]) * g.inv[i];
            gv[i] = d[i] * g.inv[i];
            const float err = 16.0f * EPS32 * (fabsf(o[i]) + tmax * fabsf(d[i]) + fabsf(g.lo[i]) + fabsf(g.hi[i])) * g.inv[i];
            can_jump = can_jump && err <= 0.125f;
        }
        float S = 0.0f;
        {
            float T = 1.0f;
            int k = 0;
            Sample s;
            while (k < a.max_steps) {
                if (!interval(g, o, d, t0, t1, dt, k, s)) break;
                if (a.use_skip) {
                    const int bx = s.c[0] >> 3, by = s.c[1] >> 3, bz = s.c[2] >> 3;
                    if (a.skip[(bz * g.nb[1] + by) * g.nb[0] + bx] == 0) {
                        int next = k + 1;
                        if (can_jump) {
                            const int bb[3] = {bx, by, bz};
                            float t_exit = INFINITY;
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                const float far_ = (float)min(BLK * bb[i] + BLK, g.res[i]) + 0.5f, near_ = (float)(BLK * bb[i]) - 0.5f;
                                if (gv[i] > 0.0f) t_exit = fminf(t_exit, (far_ - gu[i]) / gv[i]);
                                else if (gv[i] < 0.0f) t_exit = fminf(t_exit, (near_ - gu[i]) / gv[i]);
                            }
                            const float kf = floorf((t_exit - t0) / dt) - 1.0f;
                            if (kf > (float)next) next = (int)fminf(kf, (float)a.max_steps);
                        }
                        k = next;
                        continue;
                    }
                }
                const long long at = ((long long)(s.c[2] + ez) * g.P[1] + (s.c[1] + ey)) * g.P[0] + (s.c[0] + ex);
                const float wx = ex ? s.f[0] : 1.0f - s.f[0], wy = ey ? s.f[1] : 1.0f - s.f[1], wz = ez ? s.f[2] : 1.0f - s.f[2];
                const float w = (wx * wy) * wz;
                const float sigma_s = fmaxf(group_sum(w * a.sigma[at]), 0.0f);             // A SIGNED GRID: the ReLU after the interpolation
                const float delta = (s.bk - s.ak) * L;
                const float alpha = 1.0f - expf(-(sigma_s * delta));
                const float wt = T * alpha;
                if (sigma_s > 0.0f) {
                    float wq[3], col[3];
                    corner_colour<B>(a.coef, at, Y, w, wq);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) col[ch] = fminf(fmaxf(group_sum(wq[ch]), 0.0f), 1.0f);
                    sr += wt * col[0]; sg += wt * col[1]; sb += wt * col[2];
                    const float sk = (((G[0] * col[0] + G[1] * col[1]) + G[2] * col[2]) + gap) + gd * s.mk;
                    S += wt * sk;
                }
                sw += wt;
                sd += wt * s.mk;
                T = T * (1.0f - alpha);
                ++k;
                if (T < a.T_min) break;
            }
        }
        // ---- march 2: the same samples with the prefix; every sample's own block byte -------------------------
        {
            float T = 1.0f, P = 0.0f;
            long long held = -1;                               // this lane's corner of the cell whose sums it holds
            float ps = 0.0f, pc[3] = {0.0f, 0.0f, 0.0f};
            Sample s;
            for (int k = 0; k < a.max_steps; ++k) {
                if (!interval(g, o, d, t0, t1, dt, k, s)) break;
                if (a.use_skip && a.skip[((s.c[2] >> 3) * g.nb[1] + (s.c[1] >> 3)) * g.nb[0] + (s.c[0] >> 3)] == 0) continue;
                const long long at = ((long long)(s.c[2] + ez) * g.P[1] + (s.c[1] + ey)) * g.P[0] + (s.c[0] + ex);
                if (at != held) {                              // the cell changed: the same decision in all eight lanes
                    if (held >= 0) flush<B>(a, held, Y, ps, pc);
                    held = at;
                    ps = 0.0f; pc[0] = 0.0f; pc[1] = 0.0f; pc[2] = 0.0f;
                }
                const float wx = ex ? s.f[0] : 1.0f - s.f[0], wy = ey ? s.f[1] : 1.0f - s.f[1], wz = ez ? s.f[2] : 1.0f - s.f[2];
                const float w = (wx * wy) * wz;
                const float raw_s = group_sum(w * a.sigma[at]);
                const float sigma_s = fmaxf(raw_s, 0.0f);
                const float delta = (s.bk - s.ak) * L;
                const float alpha = 1.0f - expf(-(sigma_s * delta));
                const float wt = T * alpha;
                float wq[3], q[3], col[3];
                corner_colour<B>(a.coef, at, Y, w, wq);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    q[ch] = group_sum(wq[ch]);
                    col[ch] = fminf(fmaxf(q[ch], 0.0f), 1.0f);
                }
                const float sk = (((G[0] * col[0] + G[1] * col[1]) + G[2] * col[2]) + gap) + gd * s.mk;
                const float dsig = delta * (T * sk - (S - P));
                if (raw_s >= 0.0f) ps += w * dsig;             // nothing flows through the ReLU where the interpolation is negative; 0 keeps the one-sided value
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float gq = (q[ch] >= 0.0f && q[ch] <= 1.0f) ? wt * G[ch] : 0.0f;
                    pc[ch] += w * gq;
                }
                P += wt * sk;
                T = T * (1.0f - alpha);
                if (T < a.T_min) break;
            }
            if (held >= 0) flush<B>(a, held, Y, ps, pc);
        }
    }
    if (e == 0) {
        const float rest = 1.0f - sw;
        if (a.rgb) {
            a.rgb[ray * 3 + 0] = sr + rest * a.bg[0];
            a.rgb[ray * 3 + 1] = sg + rest * a.bg[1];
            a.rgb[ray * 3 + 2] = sb + rest * a.bg[2];
        }
        if (a.acc) a.acc[ray] = sw;
        if (a.depth) a.depth[ray] = sd;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: checks, launch
// ------------------------------------------------------------------------------------------------
// vox_rule.h's checks under this library's status values
static int check_grid(const char* who, const mi_voxgrad_grid* grid, Lattice* out) {
    return grid_ok(set_error, MI_VOXGRAD_MAX_RES, who, grid, out) ? MI_VOXGRAD_OK : MI_VOXGRAD_EINVAL;
}
static int check_basis(const char* who, int B) { return basis_ok(set_error, who, B) ? MI_VOXGRAD_OK : MI_VOXGRAD_EINVAL; }
static int check_march(const char* who, const mi_voxgrad_grid* grid, const mi_voxgrad_render_cfg* cfg, int64_t n, int64_t* steps) {
    return march_ok(set_error, MI_VOXGRAD_MAX_STEPS, who, grid, cfg, n, steps) ? MI_VOXGRAD_OK : MI_VOXGRAD_EINVAL;
}

}  // namespace mivoxgrad

using namespace mivoxgrad;

extern "C" {

int mi_voxgrad_abi_version(void) { return MI_VOXGRAD_ABI_VERSION; }
const char* mi_voxgrad_last_error(void) { return g_err; }

int mi_voxgrad_render_backward(const mi_voxgrad_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev,
                               const float* rays_dev, int64_t n, const mi_voxgrad_render_cfg* cfg, const float* g_rgb_dev, const float* g_acc_dev,
                               const float* g_depth_dev, float* d_sigma_dev, float* d_coef_dev, float* rgb_check_dev, float* acc_check_dev,
                               float* depth_check_dev, void* stream) {
    const char* who = "mi_voxgrad_render_backward";
    BackArgs a{};
    if (int rc = check_grid(who, grid, &a.g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    int64_t steps;
    if (int rc = check_march(who, grid, cfg, n, &steps)) return rc;
    if (n == 0) return MI_VOXGRAD_OK;                                  // no work: the arrays of an empty ray set may be NULL
    VG_CHECK_ARG(sigma_dev && coef_dev && rays_dev && g_rgb_dev && d_sigma_dev && d_coef_dev, "%s: NULL pointer", who);
    VG_CHECK_ARG(aligned(coef_dev, 16) && aligned(d_coef_dev, 16), "%s: coef and d_coef must be 16-byte aligned", who);
    VG_CHECK_ARG(skip_dev || !cfg->use_skip, "%s: use_skip needs the skip plane", who);
    VG_CHECK_ARG(aligned(sigma_dev, 4) && aligned(rays_dev, 4) && aligned(g_rgb_dev, 4) && aligned(g_acc_dev, 4) && aligned(g_depth_dev, 4) &&
                     aligned(d_sigma_dev, 4) && aligned(rgb_check_dev, 4) && aligned(acc_check_dev, 4) && aligned(depth_check_dev, 4),
                 "%s: a float array is not 4-byte aligned", who);
    a.sigma = sigma_dev; a.coef = reinterpret_cast<const float4*>(coef_dev); a.skip = skip_dev; a.rays = rays_dev; a.n = n;
    a.step = cfg->step; a.t_near = cfg->t_near; a.t_far = cfg->t_far; a.T_min = cfg->T_min;
    a.bg[0] = cfg->bg[0]; a.bg[1] = cfg->bg[1]; a.bg[2] = cfg->bg[2];
    a.use_skip = cfg->use_skip; a.max_steps = (int)steps;
    a.g_rgb = g_rgb_dev; a.g_acc = g_acc_dev; a.g_depth = g_depth_dev; a.d_sigma = d_sigma_dev; a.d_coef = d_coef_dev;
    a.rgb = rgb_check_dev; a.acc = acc_check_dev; a.depth = depth_check_dev;
    const dim3 blocks((unsigned)((n + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK));
    hipStream_t st = (hipStream_t)stream;
    if (B == 1) hipLaunchKernelGGL(backward_kernel<1>, blocks, dim3(THREADS), 0, st, a);
    else if (B == 4) hipLaunchKernelGGL(backward_kernel<4>, blocks, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(backward_kernel<9>, blocks, dim3(THREADS), 0, st, a);
    VG_LAUNCH_CHECK("backward_kernel");
    return MI_VOXGRAD_OK;
}

}  // extern "C"
