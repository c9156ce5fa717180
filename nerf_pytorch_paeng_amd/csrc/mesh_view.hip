// mesh_view.hip -- THE VIEW of include/mi_nerf_mesh.h, the second translation unit of libmi_nerf_mesh.so: a rasteriser for micro-triangles
// (a 256^3 lattice seen at 800 x 800 gives triangles of a few pixels).  No MFMA, no ray march, no call into libmi_nerf.so.
//
// view_project_kernel  one thread per vertex: camera, snap to 24.8 fixed point, validity
// view_clear_kernel    the visibility words to all ones, the six counter words to 0
// view_small_kernel    one lane per triangle: set-up, then its clipped bounding box pixel by pixel; a box above large_box pixels goes to the
//                      queue instead (wave ballot + prefix count, one atomic add per wave)
// view_large_kernel    one wave per queued triangle, the lanes striding over its box
// view_resolve_kernel  one thread per pixel: visibility word -> tri, depth
// view_shade_kernel    one thread per pixel: the winner's edge functions again, then colour, normal, disp, acc, depth
//
// Visibility is a 64-bit unsigned atomic minimum on depth bits << 32 | triangle number: the minimum of a set does not depend on the order
// its members arrive in, so every output is the same bit for bit from run to run whatever the scheduling.  Both size classes evaluate the
// same int64 edge functions and the same fp32 expression, so the class a triangle lands in (and a full queue) changes no output either.
//
// MI_MESH_VIEW_LARGE_BOX = 32, from tools/mesh_view_probe.py on the MI355X (profiles/r19_mesh_view.txt; raster ms of an 800 x 800 frame, medians of 7):
//     large_box                     4       8      16      32      64     128     256    1024
//     16^3 lattice (3 360 tris)  0.107   0.100   0.099   0.101   0.144   0.232   0.275   0.431      triangles span ~40 pixels: a wave each is 4x a lane each
//     128^3 (415 080 tris)       0.441   0.409   0.257   0.257   0.256   0.256   0.257   0.257      boxes of up to 16 pixels: a wave each costs 1.7x
//     256^3 (1 681 608 tris)     0.942   0.934   0.934   0.934   0.934   0.934   0.935   0.935      boxes of a few pixels: the threshold is never met
// 16 and 32 are level on all three; 32 keeps a margin above the micro-triangles' boxes.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_mesh.h"
#include "abi_error.h"

namespace mimesh {

// the library's one message buffer lives in mesh.hip (ABI_ERROR_STATE of abi_error.h)
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
#define VIEW_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mimesh, MI_MESH_EINVAL, cond, __VA_ARGS__)
#define VIEW_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mimesh, name)

namespace view {

constexpr int GUARD = MI_MESH_VIEW_GUARD;
constexpr int QUEUE = MI_MESH_VIEW_QUEUE;
constexpr int LARGE_BLOCKS = 1024;                    // view_large_kernel: 4096 waves stride over the queue

struct CamArgs {
    float fx, fy, cx, cy;
    float c2w[12];
};

// ---- project -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void view_project_kernel(CamArgs c, float near, const float* __restrict__ verts, int V, int32_t* __restrict__ X,
                                                           int32_t* __restrict__ Y, float* __restrict__ z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float d0 = verts[3 * (long long)i + 0] - c.c2w[3], d1 = verts[3 * (long long)i + 1] - c.c2w[7], d2 = verts[3 * (long long)i + 2] - c.c2w[11];
    const float px = (c.c2w[0] * d0 + c.c2w[4] * d1) + c.c2w[8] * d2;
    const float py = (c.c2w[1] * d0 + c.c2w[5] * d1) + c.c2w[9] * d2;
    const float pz = (c.c2w[2] * d0 + c.c2w[6] * d1) + c.c2w[10] * d2;
    const float zz = -pz;
    const float sx = c.cx + (c.fx * px) / zz;
    const float sy = c.cy - (c.fy * py) / zz;
    const float fx8 = 256.0f * sx, fy8 = 256.0f * sy;
    const bool ok = zz > near && zz < INFINITY && fabsf(fx8) <= (float)GUARD && fabsf(fy8) <= (float)GUARD;      // a NaN fails
    X[i] = ok ? (int32_t)rintf(fx8) : INT32_MIN;
    Y[i] = ok ? (int32_t)rintf(fy8) : INT32_MIN;
    z[i] = ok ? zz : 0.0f;
}

// ---- a triangle as the pixel walk sees it --------------------------------------------------------------
struct Setup {
    long long e[3];          // e_k at pixel (x0, y0)
    long long ex[3], ey[3];  // e_k(i + 1, j) - e_k(i, j) and e_k(i, j + 1) - e_k(i, j)
    int bias[3];             // 0 on a top-left edge, -1 elsewhere: covered iff e_k + bias_k >= 0 for every k
    float a2, z[3];
    int x0, y0, x1, y1;      // the bounding box clipped to the frame, in pixels (inclusive)
};

__device__ __forceinline__ bool vertex_ok(int x, int y, float zz) {
    return zz > 0.0f && zz < INFINITY && x >= -GUARD && x <= GUARD && y >= -GUARD && y <= GUARD;
}

// Set-up of triangle t from (x0, y0) = the top-left pixel of its clipped box, or of pixel (px, py) when clip is false (shade).  False: the
// triangle is not drawn (a vertex number outside [0, V), an invalid vertex, A2 == 0, culled, or a box that holds no pixel).
__device__ __forceinline__ bool tri_setup(const int32_t* __restrict__ X, const int32_t* __restrict__ Y, const float* __restrict__ z, int V,
                                          const int32_t* __restrict__ tris, long long t, int H, int W, int cull, bool clip, int px, int py, Setup& S) {
    int vx[3], vy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = tris[3 * t + k];
        if ((unsigned)v >= (unsigned)V) return false;
        vx[k] = X[v];
        vy[k] = Y[v];
        S.z[k] = z[v];
        if (!vertex_ok(vx[k], vy[k], S.z[k])) return false;
    }
    const long long A2 = (long long)(vx[1] - vx[0]) * (vy[2] - vy[0]) - (long long)(vy[1] - vy[0]) * (vx[2] - vx[0]);
    if (A2 == 0 || (cull == 1 && A2 > 0) || (cull == 2 && A2 < 0)) return false;
    const int s = A2 < 0 ? -1 : 1;
    if (clip) {
        const int lox = min(vx[0], min(vx[1], vx[2])), hix = max(vx[0], max(vx[1], vx[2]));
        const int loy = min(vy[0], min(vy[1], vy[2])), hiy = max(vy[0], max(vy[1], vy[2]));
        S.x0 = max(0, (lox + 255) >> 8);                                   // the first pixel centre at or right of lox (>> floors)
        S.y0 = max(0, (loy + 255) >> 8);
        S.x1 = min(W - 1, hix >> 8);
        S.y1 = min(H - 1, hiy >> 8);
        if (S.x0 > S.x1 || S.y0 > S.y1) return false;
    } else {
        S.x0 = S.x1 = px;
        S.y0 = S.y1 = py;
    }
    const long long Px = 256LL * S.x0, Py = 256LL * S.y0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                          // e_k: the edge from a = v(k+1) to b = v(k+2)
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const long long dx = (long long)s * (vx[b] - vx[a]), dy = (long long)s * (vy[b] - vy[a]);
        S.e[k] = dx * (Py - vy[a]) - dy * (Px - vx[a]);
        S.ex[k] = -256 * dy;
        S.ey[k] = 256 * dx;
        S.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
    }
    S.a2 = (float)(s * A2);
    return true;
}

__device__ __forceinline__ bool covered(const Setup& S, long long e0, long long e1, long long e2) {
    return (e0 + S.bias[0]) >= 0 && (e1 + S.bias[1]) >= 0 && (e2 + S.bias[2]) >= 0;
}

// w_k = b_k / z_k and the depth: Depth of THE VIEW
__device__ __forceinline__ float depth_of(const Setup& S, long long e0, long long e1, long long e2, float w[3]) {
    w[0] = ((float)e0 / S.a2) / S.z[0];
    w[1] = ((float)e1 / S.a2) / S.z[1];
    w[2] = ((float)e2 / S.a2) / S.z[2];
    return 1.0f / ((w[0] + w[1]) + w[2]);
}

// One sample: true when it lowered the word.  The returning form of the atomic is used ON PURPOSE: the lane waits for the old value before it
// goes on, so the registers that hold the sample are not rewritten while the update is in flight.  The form without a return, inside the
// lane's pixel loop, gave words whose depth half was not the sample's (docs/design/16_mesh.md 16.7, "The atomic's operands").
__device__ __forceinline__ bool sample(const Setup& S, long long e0, long long e1, long long e2, long long t, unsigned long long* word) {
    float w[3];
    const float depth = depth_of(S, e0, e1, e2, w);
    const unsigned long long v = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(unsigned)t;
    return __hip_atomic_fetch_min(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v;
}

// ---- visibility ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void view_clear_kernel(long long n, unsigned long long* __restrict__ word, unsigned* __restrict__ counters) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) word[i] = ~0ull;
    if (i < 6) counters[i] = 0u;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void view_small_kernel(int H, int W, int cull, int large_box, const int32_t* __restrict__ X,
                                                         const int32_t* __restrict__ Y, const float* __restrict__ z, int V,
                                                         const int32_t* __restrict__ tris, int T, unsigned long long* __restrict__ word,
                                                         unsigned* __restrict__ counters, int32_t* __restrict__ queue) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    Setup S;
    bool live = t < T && tri_setup(X, Y, z, V, tris, t, H, W, cull, true, 0, 0, S);
    const bool large = live && (long long)(S.x1 - S.x0 + 1) * (S.y1 - S.y0 + 1) > large_box;
    const unsigned long long m = __ballot(large);
    if (m != 0ull) {                                                        // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&counters[0], (unsigned)__popcll(m));
        base = __shfl(base, leader, 64);
        if (large) {
            const unsigned long long slot = (unsigned long long)base + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < (unsigned long long)QUEUE) {                        // a full queue: the lane walks the box itself
                queue[slot] = (int32_t)t;
                live = false;
            }
        }
    }
    unsigned issued = 0, lowered = 0;
    if (live) {
        long long r0 = S.e[0], r1 = S.e[1], r2 = S.e[2];
        for (int y = S.y0; y <= S.y1; ++y) {
            long long e0 = r0, e1 = r1, e2 = r2;
            for (int x = S.x0; x <= S.x1; ++x) {
                if (covered(S, e0, e1, e2)) {
                    lowered += sample(S, e0, e1, e2, t, word + ((long long)y * W + x)) ? 1u : 0u;
                    ++issued;
                }
                e0 += S.ex[0]; e1 += S.ex[1]; e2 += S.ex[2];
            }
            r0 += S.ey[0]; r1 += S.ey[1]; r2 += S.ey[2];
        }
    }
    const unsigned drawn = wave_sum(live ? 1u : 0u), total = wave_sum(issued), won = wave_sum(lowered);
    if (lane == 0) {
        if (drawn) atomicAdd(&counters[1], drawn);
        if (total) atomicAdd((unsigned long long*)(counters + 2), (unsigned long long)total);
        if (won) atomicAdd((unsigned long long*)(counters + 4), (unsigned long long)won);
    }
}

__global__ __launch_bounds__(256) void view_large_kernel(int H, int W, int cull, const int32_t* __restrict__ X, const int32_t* __restrict__ Y,
                                                         const float* __restrict__ z, int V, const int32_t* __restrict__ tris,
                                                         unsigned long long* __restrict__ word, unsigned* __restrict__ counters,
                                                         const int32_t* __restrict__ queue) {
    const unsigned met = counters[0];
    const int n = (int)(met < (unsigned)QUEUE ? met : (unsigned)QUEUE);
    const int lane = threadIdx.x & 63, wave = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), waves = (int)(gridDim.x * 4);
    unsigned issued = 0, lowered = 0;
    for (int q = wave; q < n; q += waves) {
        const long long t = queue[q];
        Setup S;
        if (!tri_setup(X, Y, z, V, tris, t, H, W, cull, true, 0, 0, S)) continue;     // wave-uniform: it was drawable when it was queued
        const int bw = S.x1 - S.x0 + 1;
        const long long box = (long long)bw * (S.y1 - S.y0 + 1);
        for (long long p = lane; p < box; p += 64) {
            const long long dy = p / bw, dx = p - dy * bw;
            const long long e0 = S.e[0] + dx * S.ex[0] + dy * S.ey[0], e1 = S.e[1] + dx * S.ex[1] + dy * S.ey[1],
                            e2 = S.e[2] + dx * S.ex[2] + dy * S.ey[2];
            if (covered(S, e0, e1, e2)) {
                lowered += sample(S, e0, e1, e2, t, word + ((S.y0 + dy) * W + (S.x0 + dx))) ? 1u : 0u;
                ++issued;
            }
        }
    }
    const unsigned total = wave_sum(issued), won = wave_sum(lowered);
    if (lane == 0 && total) atomicAdd((unsigned long long*)(counters + 2), (unsigned long long)total);
    if (lane == 0 && won) atomicAdd((unsigned long long*)(counters + 4), (unsigned long long)won);
}

__global__ __launch_bounds__(256) void view_resolve_kernel(long long n, const unsigned long long* __restrict__ word, int32_t* __restrict__ tri,
                                                           float* __restrict__ depth) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long w = word[i];
    const unsigned lo = (unsigned)w;
    if (tri) tri[i] = (int32_t)lo;                                          // all ones: -1
    if (depth) depth[i] = lo == 0xffffffffu ? 0.0f : __uint_as_float((unsigned)(w >> 32));
}

// ---- shade ---------------------------------------------------------------------------------------------
struct Bg {
    float c[3];
};

__global__ __launch_bounds__(256) void view_shade_kernel(int H, int W, const int32_t* __restrict__ X, const int32_t* __restrict__ Y,
                                                         const float* __restrict__ z, int V, const int32_t* __restrict__ tris, int T,
                                                         const int32_t* __restrict__ tri_in, const float* __restrict__ colors,
                                                         const float* __restrict__ normals, Bg bg, float* __restrict__ rgb, float* __restrict__ disp,
                                                         float* __restrict__ acc, float* __restrict__ depth_out, float* __restrict__ normal) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int t = tri_in[i];
    const int py = (int)(i / W), px = (int)(i - (long long)py * W);
    Setup S;
    const bool hit = t >= 0 && t < T && tri_setup(X, Y, z, V, tris, t, H, W, 0, false, px, py, S);
    float w[3] = {0.0f, 0.0f, 0.0f};
    const float depth = hit ? depth_of(S, S.e[0], S.e[1], S.e[2], w) : 0.0f;
    if (depth_out) depth_out[i] = depth;
    if (acc) acc[i] = hit ? 1.0f : 0.0f;
    if (disp) disp[i] = hit ? 1.0f / depth : 0.0f;
    if (!rgb && !normal) return;
    int v[3] = {0, 0, 0};
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = tris[3 * (long long)t + k];
    }
    if (rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float c = bg.c[ch];
            if (hit) {
                c = ((w[0] * colors[3 * (long long)v[0] + ch] + w[1] * colors[3 * (long long)v[1] + ch]) + w[2] * colors[3 * (long long)v[2] + ch]) * depth;
                c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);                 // a NaN stays a NaN
            }
            rgb[3 * i + ch] = c;
        }
    }
    if (normal) {
        float n[3] = {0.0f, 0.0f, 0.0f};
        if (hit) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                n[ch] = ((w[0] * normals[3 * (long long)v[0] + ch] + w[1] * normals[3 * (long long)v[1] + ch]) + w[2] * normals[3 * (long long)v[2] + ch]) * depth;
            const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const bool ok = len > 0.0f && len < INFINITY;                   // a NaN fails the first
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) n[ch] = ok ? n[ch] / len : 0.0f;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) normal[3 * i + ch] = n[ch];
    }
}

// ---- host side -----------------------------------------------------------------------------------------
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

static int check_frame(int H, int W) {
    VIEW_CHECK_ARG(H >= 1 && H <= MI_MESH_VIEW_MAX_DIM && W >= 1 && W <= MI_MESH_VIEW_MAX_DIM, "H=%d, W=%d: 1..%d each (MI_MESH_VIEW_MAX_DIM)", H, W,
                   MI_MESH_VIEW_MAX_DIM);
    return MI_MESH_OK;
}

static int check_counts(int64_t V, int64_t T) {
    VIEW_CHECK_ARG(V >= 0 && V <= 0x7fffffffLL && T >= 0 && T <= 0x7fffffffLL, "V=%lld, T=%lld: 0..2^31 - 1 each (int32 vertex and triangle numbers)",
                   (long long)V, (long long)T);
    return MI_MESH_OK;
}

static int check_mesh(const int32_t* X, const int32_t* Y, const float* z, int64_t V, const int32_t* tris, int64_t T) {
    if (int rc = check_counts(V, T)) return rc;
    VIEW_CHECK_ARG(V == 0 || (X && Y && z), "NULL pointer (X, Y and z are required where V is not 0)");
    VIEW_CHECK_ARG(T == 0 || tris, "NULL pointer (tris is required where T is not 0)");
    VIEW_CHECK_ARG(aligned4(X) && aligned4(Y) && aligned4(z) && aligned4(tris), "X, Y, z and tris must be 4-byte aligned");
    return MI_MESH_OK;
}

static size_t words_bytes(int H, int W) { return align256((size_t)8 * H * W); }
static size_t raster_bytes(int H, int W) { return words_bytes(H, W) + align256(24 + (size_t)4 * QUEUE); }

static int project(const mi_mesh_camera* cam, float near, const float* verts, int64_t V, int32_t* X, int32_t* Y, float* z, hipStream_t st) {
    VIEW_CHECK_ARG(cam != nullptr, "cam is NULL");
    if (int rc = check_frame(cam->H, cam->W)) return rc;
    VIEW_CHECK_ARG(isfinite(cam->fx) && isfinite(cam->fy) && cam->fx != 0.0f && cam->fy != 0.0f && isfinite(cam->cx) && isfinite(cam->cy),
                   "camera: fx=%g, fy=%g, cx=%g, cy=%g must be finite, fx and fy not 0", (double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy);
    CamArgs c;
    c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
    for (int i = 0; i < 12; ++i) {
        VIEW_CHECK_ARG(isfinite(cam->c2w[i]), "camera: c2w[%d] is not finite", i);
        c.c2w[i] = cam->c2w[i];
    }
    VIEW_CHECK_ARG(near > 0.0f, "near=%g must be above 0", (double)near);                      // a NaN fails
    if (int rc = check_counts(V, 0)) return rc;
    VIEW_CHECK_ARG(V == 0 || (verts && X && Y && z), "NULL pointer (verts, X, Y and z are required where V is not 0)");
    VIEW_CHECK_ARG(aligned4(verts) && aligned4(X) && aligned4(Y) && aligned4(z), "verts, X, Y and z must be 4-byte aligned");
    if (V == 0) return MI_MESH_OK;
    hipLaunchKernelGGL(view_project_kernel, dim3(blocks_for(V, 256)), dim3(256), 0, st, c, near, verts, (int)V, X, Y, z);
    VIEW_LAUNCH_CHECK("view_project_kernel");
    return MI_MESH_OK;
}

static int raster(int H, int W, int cull, int large_box, const int32_t* X, const int32_t* Y, const float* z, int64_t V, const int32_t* tris, int64_t T,
                  void* scratch, size_t scratch_bytes, int32_t* tri_out, float* depth_out, hipStream_t st) {
    if (int rc = check_frame(H, W)) return rc;
    VIEW_CHECK_ARG(cull >= 0 && cull <= 2, "cull=%d: 0 (both), 1 (drop back faces) or 2 (drop front faces)", cull);
    VIEW_CHECK_ARG(large_box >= 0, "large_box=%d: 0 (MI_MESH_VIEW_LARGE_BOX) or a pixel count above 0", large_box);
    if (int rc = check_mesh(X, Y, z, V, tris, T)) return rc;
    VIEW_CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 255) == 0, "scratch must be given and 256-byte aligned");
    VIEW_CHECK_ARG(scratch_bytes >= raster_bytes(H, W), "scratch too small: %zu < %zu (mi_mesh_raster_scratch_bytes)", scratch_bytes, raster_bytes(H, W));
    VIEW_CHECK_ARG(tri_out || depth_out, "no output: tri_out and depth_out are both NULL");
    VIEW_CHECK_ARG(aligned4(tri_out) && aligned4(depth_out), "tri_out and depth_out must be 4-byte aligned");
    const long long n = (long long)H * W;
    unsigned long long* word = (unsigned long long*)scratch;
    unsigned* counters = (unsigned*)((char*)scratch + words_bytes(H, W));
    int32_t* queue = (int32_t*)(counters + 6);
    hipLaunchKernelGGL(view_clear_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, word, counters);
    VIEW_LAUNCH_CHECK("view_clear_kernel");
    if (T > 0 && V > 0) {
        hipLaunchKernelGGL(view_small_kernel, dim3(blocks_for(T, 256)), dim3(256), 0, st, H, W, cull, large_box ? large_box : MI_MESH_VIEW_LARGE_BOX, X, Y,
                           z, (int)V, tris, (int)T, word, counters, queue);
        VIEW_LAUNCH_CHECK("view_small_kernel");
        hipLaunchKernelGGL(view_large_kernel, dim3(LARGE_BLOCKS), dim3(256), 0, st, H, W, cull, X, Y, z, (int)V, tris, word, counters, queue);
        VIEW_LAUNCH_CHECK("view_large_kernel");
    }
    hipLaunchKernelGGL(view_resolve_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, word, tri_out, depth_out);
    VIEW_LAUNCH_CHECK("view_resolve_kernel");
    return MI_MESH_OK;
}

static int shade(int H, int W, const int32_t* X, const int32_t* Y, const float* z, int64_t V, const int32_t* tris, int64_t T, const int32_t* tri_in,
                 const float* colors, const float* normals, const float* bg, float* rgb, float* disp, float* acc, float* depth, float* normal,
                 hipStream_t st) {
    if (int rc = check_frame(H, W)) return rc;
    if (int rc = check_mesh(X, Y, z, V, tris, T)) return rc;
    VIEW_CHECK_ARG(tri_in != nullptr && aligned4(tri_in), "tri_in must be given and 4-byte aligned");
    VIEW_CHECK_ARG(rgb || disp || acc || depth || normal, "no output: rgb, disp, acc, depth and normal are all NULL");
    VIEW_CHECK_ARG(aligned4(rgb) && aligned4(disp) && aligned4(acc) && aligned4(depth) && aligned4(normal) && aligned4(colors) && aligned4(normals),
                   "colors, normals and the outputs must be 4-byte aligned");
    VIEW_CHECK_ARG(!rgb || bg, "bg is NULL (required with rgb)");
    VIEW_CHECK_ARG(!rgb || V == 0 || colors, "colors is NULL (required with rgb where V is not 0)");
    VIEW_CHECK_ARG(!normal || V == 0 || normals, "normals is NULL (required with normal where V is not 0)");
    Bg b = {{0.0f, 0.0f, 0.0f}};
    if (rgb)
        for (int i = 0; i < 3; ++i) b.c[i] = bg[i];
    hipLaunchKernelGGL(view_shade_kernel, dim3(blocks_for((long long)H * W, 256)), dim3(256), 0, st, H, W, X, Y, z, (int)V, tris, (int)T, tri_in, colors, normals,
                       b, rgb, disp, acc, depth, normal);
    VIEW_LAUNCH_CHECK("view_shade_kernel");
    return MI_MESH_OK;
}

}  // namespace view
}  // namespace mimesh

using namespace mimesh;

extern "C" {

int mi_mesh_project(const mi_mesh_camera* cam, float near, const float* verts, int64_t V, int32_t* X, int32_t* Y, float* z, void* stream) {
    return view::project(cam, near, verts, V, X, Y, z, (hipStream_t)stream);
}

size_t mi_mesh_raster_scratch_bytes(int H, int W) { return view::check_frame(H, W) == MI_MESH_OK ? view::raster_bytes(H, W) : 0; }

int mi_mesh_raster(int H, int W, int cull, int large_box, const int32_t* X, const int32_t* Y, const float* z, int64_t V, const int32_t* tris, int64_t T,
                   void* scratch, size_t scratch_bytes, int32_t* tri_out, float* depth_out, void* stream) {
    return view::raster(H, W, cull, large_box, X, Y, z, V, tris, T, scratch, scratch_bytes, tri_out, depth_out, (hipStream_t)stream);
}

int mi_mesh_shade(int H, int W, const int32_t* X, const int32_t* Y, const float* z, int64_t V, const int32_t* tris, int64_t T, const int32_t* tri_in,
                  const float* colors, const float* normals, const float* bg, float* rgb, float* disp, float* acc, float* depth, float* normal,
                  void* stream) {
    return view::shade(H, W, X, Y, z, V, tris, T, tri_in, colors, normals, bg, rgb, disp, acc, depth, normal, (hipStream_t)stream);
}

}  // extern "C"
