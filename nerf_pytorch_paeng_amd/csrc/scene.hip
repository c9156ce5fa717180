// scene.hip -- libmi_nerf_scene.so (include/mi_nerf_scene.h): procedural solid-object scenes.  A short list of spheres, boxes and cylinders
// answers what a network answers -- raw (r, g, b, sigma) at a point -- in closed form (THE FIELD RULE of the header), and a fused kernel forms
// the ground-truth image of it through post_process.  A library of its own: no other header of the project, no other library.
//
// scene_field_kernel    one thread per sample: THE FIELD RULE, one 16-byte store (the shapes of mi_nerf_mlp_rays)
// scene_render_kernel   one ray per lane, its S bin-centre samples in sequence: field rule, alpha, running transmittance, five running sums;
//                       rays in, four outputs out, nothing else through device memory
//
// The primitives are kernel arguments (1 KiB by value): every lane of a launch tests the same primitive at the same time, so the loop over
// them is wave-uniform -- scalar loads from the argument segment, scalar branches on kind / axis / freq, SGPR operands of the vector
// compares -- and a lane owns nothing but its point.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_scene.h"
#include "abi_error.h"

namespace miscene {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_SCENE_EHIP)
#define SCENE_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::miscene, MI_SCENE_EINVAL, cond, __VA_ARGS__)
#define SCENE_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::miscene, name)

constexpr long long MAX_POINTS = 1LL << 39;      // 2^31 blocks of 256 threads

// ---- the scene as the kernels see it ---------------------------------------------------------------
// h as the tests of the field rule read it: sphere h[0] = r*r; cylinder h[0] = r*r, h[1] = half-height; box: the half-extents.  The squares
// are fp32 products rounded once on the host, the numbers the rule names.
struct PrimDev {
    int kind, axis;
    float c[3], h[3];
    float sigma;
    float rgb[6];
    float freq;
};
struct SceneDev {
    PrimDev p[MI_SCENE_MAX_PRIMS];
    int n;
};

static const char* const KIND_NAMES[3] = {"sphere", "box", "cylinder"};

static int resolve_scene(const mi_scene_prim* prims, int n_prims, SceneDev* out) {
    SCENE_CHECK_ARG(prims != nullptr, "prims is NULL");
    SCENE_CHECK_ARG(n_prims >= 1 && n_prims <= MI_SCENE_MAX_PRIMS, "n_prims=%d: 1..%d", n_prims, MI_SCENE_MAX_PRIMS);
    for (int i = 0; i < n_prims; ++i) {
        const mi_scene_prim& P = prims[i];
        SCENE_CHECK_ARG(P.kind >= MI_SCENE_SPHERE && P.kind <= MI_SCENE_CYLINDER, "prim %d: kind=%d is not a sphere (0), a box (1) or a cylinder (2)", i, P.kind);
        SCENE_CHECK_ARG(P.axis >= 0 && P.axis <= 2, "prim %d: axis=%d: 0, 1 or 2", i, P.axis);
        const int used = P.kind == MI_SCENE_BOX ? 3 : P.kind == MI_SCENE_SPHERE ? 1 : 2;
        PrimDev D;
        D.kind = P.kind;
        D.axis = P.axis;
        for (int j = 0; j < 3; ++j) {
            SCENE_CHECK_ARG(isfinite(P.c[j]), "prim %d (%s): centre c[%d]=%g is not finite", i, KIND_NAMES[P.kind], j, (double)P.c[j]);
            D.c[j] = P.c[j];
            D.h[j] = 0.0f;
        }
        for (int j = 0; j < used; ++j) {
            SCENE_CHECK_ARG(isfinite(P.h[j]) && P.h[j] > 0.0f, "prim %d (%s): extent h[%d]=%g must be finite and > 0", i, KIND_NAMES[P.kind], j, (double)P.h[j]);
            D.h[j] = P.h[j];
        }
        if (P.kind != MI_SCENE_BOX) {
            D.h[0] = P.h[0] * P.h[0];
            SCENE_CHECK_ARG(isfinite(D.h[0]) && D.h[0] > 0.0f, "prim %d (%s): the square of radius h[0]=%g is not a positive finite fp32 number", i, KIND_NAMES[P.kind],
                            (double)P.h[0]);
        }
        SCENE_CHECK_ARG(isfinite(P.sigma) && P.sigma > 0.0f, "prim %d (%s): sigma=%g must be finite and > 0", i, KIND_NAMES[P.kind], (double)P.sigma);
        D.sigma = P.sigma;
        for (int j = 0; j < 6; ++j) {
            SCENE_CHECK_ARG(isfinite(P.rgb_raw[j / 3][j % 3]), "prim %d (%s): rgb_raw[%d][%d]=%g is not finite", i, KIND_NAMES[P.kind], j / 3, j % 3,
                            (double)P.rgb_raw[j / 3][j % 3]);
            D.rgb[j] = P.rgb_raw[j / 3][j % 3];
        }
        SCENE_CHECK_ARG(isfinite(P.freq) && P.freq >= 0.0f, "prim %d (%s): freq=%g must be finite and >= 0", i, KIND_NAMES[P.kind], (double)P.freq);
        D.freq = P.freq;
        if (out) out->p[i] = D;
    }
    if (out) {
        for (int i = n_prims; i < MI_SCENE_MAX_PRIMS; ++i) out->p[i] = out->p[0];      // never read; defined bytes in the argument segment
        out->n = n_prims;
    }
    return MI_SCENE_OK;
}

// THE FIELD RULE, first half: the first primitive in list order that contains p (-1: none) and its colour index.  The list is walked from
// its end so that an earlier primitive overwrites a later one: no lane leaves the loop early, and everything but q is wave-uniform.
// -ffp-contract=off: every product and every sum is rounded on its own.
__device__ __forceinline__ int scene_hit(const SceneDev& sc, float px, float py, float pz, int& colour) {
    int hit = -1, col = 0;
    for (int i = sc.n - 1; i >= 0; --i) {
        const PrimDev& P = sc.p[i];
        const float q0 = px - P.c[0], q1 = py - P.c[1], q2 = pz - P.c[2];
        bool in;
        if (P.kind == MI_SCENE_BOX) {
            in = __builtin_fabsf(q0) <= P.h[0] && __builtin_fabsf(q1) <= P.h[1] && __builtin_fabsf(q2) <= P.h[2];
        } else if (P.kind == MI_SCENE_SPHERE) {
            in = (q0 * q0 + q1 * q1) + q2 * q2 <= P.h[0];
        } else {
            const float qa = P.axis == 0 ? q0 : P.axis == 1 ? q1 : q2;
            const float qb = P.axis == 0 ? q1 : q0;                       // b < c: the two other axes in order
            const float qc = P.axis == 2 ? q1 : q2;
            in = __builtin_fabsf(qa) <= P.h[1] && qb * qb + qc * qc <= P.h[0];
        }
        int c = 0;
        if (P.freq > 0.0f) c = ((int)floorf(q0 * P.freq) + (int)floorf(q1 * P.freq) + (int)floorf(q2 * P.freq)) & 1;
        hit = in ? i : hit;
        col = in ? c : col;
    }
    colour = col;
    return hit;
}

// second half: the raw output of primitive `hit` (>= 0), colour `col`.  hit differs from lane to lane, the argument segment is read with
// scalar loads: one more uniform walk with selects, taken only by waves that hit something.
__device__ __forceinline__ void scene_raw(const SceneDev& sc, int hit, int col, float& r, float& g, float& b, float& sigma) {
    r = g = b = sigma = 0.0f;
    for (int i = 0; i < sc.n; ++i) {
        const PrimDev& P = sc.p[i];
        const bool me = hit == i;
        r = me ? (col ? P.rgb[3] : P.rgb[0]) : r;
        g = me ? (col ? P.rgb[4] : P.rgb[1]) : g;
        b = me ? (col ? P.rgb[5] : P.rgb[2]) : b;
        sigma = me ? P.sigma : sigma;
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void scene_field_kernel(SceneDev sc, const float* __restrict__ rays, const float* __restrict__ z, long long n_pts, int S,
                                                          f32x4* __restrict__ raw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;
    const float* rp = rays + (i / S) * 6;
    const float zz = z[i];
    const float px = rp[0] + rp[3] * zz, py = rp[1] + rp[4] * zz, pz = rp[2] + rp[5] * zz;      // nerf_process.py:69-70
    int col;
    const int hit = scene_hit(sc, px, py, pz, col);
    float r = 0.0f, g = 0.0f, b = 0.0f, s = 0.0f;
    if (hit >= 0) scene_raw(sc, hit, col, r, g, b, s);
    const f32x4 v = {r, g, b, s};
    raw[i] = v;
}

// One ray per lane.  An empty sample has alpha = 1 - expf(-0 * dist) = 0 exactly, weight 0 and leaves T as it is (1 - 0 + 1e-10 rounds to 1):
// it is skipped without a trace in any sum.  Once T is exactly 0 (a few samples into an opaque solid) every later weight is exactly 0 too, and
// the lane stops.  Both shortcuts leave the sums the numbers the full loop gives.
__global__ __launch_bounds__(256) void scene_render_kernel(SceneDev sc, const float* __restrict__ rays, long long n, float near_, float step, int S,
                                                           float* __restrict__ rgb_o, float* __restrict__ disp_o, float* __restrict__ acc_o,
                                                           float* __restrict__ depth_o) {
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= n) return;
    const float* rp = rays + ray * 6;
    const float ox = rp[0], oy = rp[1], oz = rp[2], dx = rp[3], dy = rp[4], dz = rp[5];
    const float dnorm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);                          // nerf_process.py:101
    float T = 1.0f, sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f;
    float zk = near_ + 0.5f * step;
    if (S > 1) {                                                                               // S == 1: the reference leaves no sample at all
        for (int k = 0; k < S; ++k) {
            const float zn = near_ + ((float)(k + 1) + 0.5f) * step;
            const float px = ox + dx * zk, py = oy + dy * zk, pz = oz + dz * zk;               // :69-70
            int col;
            const int hit = scene_hit(sc, px, py, pz, col);
            if (hit >= 0) {
                float vr, vg, vb, vs;
                scene_raw(sc, hit, col, vr, vg, vb, vs);
                float dist = (k + 1 < S) ? (zn - zk) : 1e10f;                                  // :93-97
                dist = dist * dnorm;                                                           // :101
                const float sig = __builtin_fmaxf(vs, 0.0f);                                   // relu, :91
                const float a = 1.0f - expf(-sig * dist);                                      // :92
                const float w = a * T;                                                         // :111
                sw += w;
                sr += w * (1.0f / (1.0f + expf(-vr)));                                         // sigmoid, :104
                sg += w * (1.0f / (1.0f + expf(-vg)));
                sb += w * (1.0f / (1.0f + expf(-vb)));
                sd += w * zk;
                T *= (1.0f - a + 1e-10f);                                                      // :110
                if (T == 0.0f) break;
            }
            zk = zn;
        }
    }
    const float q = sd / sw;                                                                   // depth / acc
    const float m = (q != q) ? q : __builtin_fmaxf(1e-10f, q);                                 // torch.max propagates NaN (:124)
    float disp = 1.0f / m;
    if (disp != disp) disp = 0.0f;                                                             // :126
    if (disp > 5.0f) disp = 5.0f;                                                              // :132-134
    const float bg = 1.0f - sw;                                                                // :138 white background, always
    rgb_o[ray * 3 + 0] = sr + bg;
    rgb_o[ray * 3 + 1] = sg + bg;
    rgb_o[ray * 3 + 2] = sb + bg;
    if (disp_o) disp_o[ray] = disp;
    if (acc_o) acc_o[ray] = sw;
    if (depth_o) depth_o[ray] = sd;
}

}  // namespace miscene

using namespace miscene;

extern "C" {

int mi_scene_abi_version(void) { return MI_SCENE_ABI_VERSION; }
const char* mi_scene_last_error(void) { return g_err; }

int mi_scene_check(const mi_scene_prim* prims, int n_prims) { return resolve_scene(prims, n_prims, nullptr); }

int mi_scene_field_rays(const mi_scene_prim* prims, int n_prims, const float* rays_dev, const float* z_dev, int64_t n_rays, int S, float* raw_dev,
                        void* stream) {
    SceneDev sc;
    const int rc = resolve_scene(prims, n_prims, &sc);
    if (rc != MI_SCENE_OK) return rc;
    SCENE_CHECK_ARG(n_rays >= 0, "mi_scene_field_rays: n_rays=%lld is negative", (long long)n_rays);
    SCENE_CHECK_ARG(n_rays == 0 || (rays_dev != nullptr && z_dev != nullptr && raw_dev != nullptr), "mi_scene_field_rays: rays / z / raw is NULL");
    SCENE_CHECK_ARG(((uintptr_t)raw_dev & 15) == 0, "mi_scene_field_rays: raw must be 16-byte aligned");
    SCENE_CHECK_ARG(S >= 1, "mi_scene_field_rays: S=%d must be >= 1", S);
    SCENE_CHECK_ARG(n_rays < MAX_POINTS / S, "mi_scene_field_rays: n_rays * S = %lld * %d: below 2^39", (long long)n_rays, S);
    if (n_rays == 0) return MI_SCENE_OK;
    const long long n_pts = (long long)n_rays * S;
    hipLaunchKernelGGL(scene_field_kernel, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sc, rays_dev, z_dev, n_pts, S,
                       (f32x4*)raw_dev);
    SCENE_LAUNCH_CHECK("scene_field_kernel");
    return MI_SCENE_OK;
}

int mi_scene_render(const mi_scene_prim* prims, int n_prims, const float* rays_dev, int64_t n_rays, float near_, float far_, int S, float* rgb_dev,
                    float* disp_dev, float* acc_dev, float* depth_dev, void* stream) {
    SceneDev sc;
    const int rc = resolve_scene(prims, n_prims, &sc);
    if (rc != MI_SCENE_OK) return rc;
    SCENE_CHECK_ARG(n_rays >= 0 && n_rays < MAX_POINTS, "mi_scene_render: n_rays=%lld: 0 .. 2^39 - 1", (long long)n_rays);
    SCENE_CHECK_ARG(n_rays == 0 || (rays_dev != nullptr && rgb_dev != nullptr), "mi_scene_render: rays / rgb is NULL");
    SCENE_CHECK_ARG(S >= 1 && S <= MI_SCENE_MAX_SAMPLES, "mi_scene_render: S=%d: 1..%d", S, MI_SCENE_MAX_SAMPLES);
    SCENE_CHECK_ARG(isfinite(near_) && isfinite(far_) && near_ < far_, "mi_scene_render: near=%g must be below far=%g, both finite", (double)near_, (double)far_);
    const float step = (far_ - near_) / (float)S;
    SCENE_CHECK_ARG(isfinite(step) && step > 0.0f, "mi_scene_render: (far - near) / S = %g is not a positive finite fp32 step", (double)step);
    if (n_rays == 0) return MI_SCENE_OK;
    hipLaunchKernelGGL(scene_render_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sc, rays_dev, (long long)n_rays, near_,
                       step, S, rgb_dev, disp_dev, acc_dev, depth_dev);
    SCENE_LAUNCH_CHECK("scene_render_kernel");
    return MI_SCENE_OK;
}

}  // extern "C"
