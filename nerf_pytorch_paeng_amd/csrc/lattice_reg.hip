// lattice_reg.hip -- the second translation unit of libmi_nerf_geo.so (include/mi_nerf_geo.h, THE LATTICE REGULARISERS): total variation
// and a Cauchy sparsity prior over a channel-last lattice array, value and gradient.  It shares abi_error.h with the rest of the project
// and nothing else; the error text lives in geo.hip (one buffer per library) and is reached through the two declarations below.
//
//   lattice_tv_kernel<VEC, GRAD, VALUE>        one workgroup per (block row of the mask: b_z, b_y, a run of WX blocks along x).  Lanes run
//                                              along the contiguous direction (x, channel) in units of VEC floats (float4 for R > 1), four
//                                              rows of y per pass, the workgroup marches in z.  Each thread OWNS its elements of d_v: it
//                                              gathers the 13-point stencil and adds the gradient -- no atomic, no LDS tile.  The halo is
//                                              left to the caches: a tile is 9 x 9 x 288 floats at most, three z-planes of it live at a time.
//   lattice_sparsity_kernel<GRAD, VALUE>       the same geometry over a plane with R = C = 1, pointwise
//   lattice_finish_kernel                      one workgroup: the partials in index order per thread, then a fixed tree
//
// A workgroup whose own blocks and (for the gradient) backward neighbour blocks are all masked out loads nothing of v or d_v and stores
// nothing but its zero partial.  Values: each thread adds its terms in double in loop order, the 64 lanes by a butterfly, the four waves in
// order: one double per workgroup.  Compiled with -ffp-contract=off like geo.hip; sqrtf and / are correctly rounded (hipcc's default).
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_geo.h"
#include "abi_error.h"

namespace migeo {
void set_error(const char* fmt, ...);            // geo.hip
int hip_fail(hipError_t e, const char* what);    // geo.hip
}  // namespace migeo

namespace milat {

#define LAT_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::migeo, MI_GEO_EINVAL, cond, __VA_ARGS__)
#define LAT_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::migeo, name)

constexpr int THREADS = 256;     // 64 lanes along (x, channel) times 4 rows of y
constexpr int BLOCK = 8;         // cells per mask block and axis (the skip plane of include/mi_nerf_vox.h)
constexpr int MAX_P = 513, MIN_P = 2;

struct Args {
    const float* v;
    float* d_v;
    const unsigned char* mask;
    double* partial;
    int Pz, Py, Px, R, C;
    int nBz, nBy, nBx, WX;       // mask blocks per axis; blocks along x per workgroup
    float eps, scale;
};

// blocks along x per workgroup: a row of the tile is at least 256 floats wide
static int run_of(int R) { return R >= 32 ? 1 : R == 16 ? 2 : R == 4 ? 8 : 32; }

struct Geometry { int nBz, nBy, nBx, WX, nSX; };
static Geometry geometry_of(const int32_t* P, int R) {
    Geometry g;
    g.nBz = (P[0] - 1 + BLOCK - 1) / BLOCK;
    g.nBy = (P[1] - 1 + BLOCK - 1) / BLOCK;
    g.nBx = (P[2] - 1 + BLOCK - 1) / BLOCK;
    g.WX = run_of(R);
    g.nSX = (g.nBx + g.WX - 1) / g.WX;
    return g;
}

template <int VEC> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<4> { using type = float4; };
__device__ __forceinline__ float comp(float a, int) { return a; }
__device__ __forceinline__ float comp(const float4& a, int j) { return j == 0 ? a.x : j == 1 ? a.y : j == 2 ? a.z : a.w; }

// t(p, c) of THE LATTICE REGULARISERS from the three forward differences (an absent one is exactly 0)
__device__ __forceinline__ float tv_norm(float eps, float dx, float dy, float dz) {
    return sqrtf(((eps + dx * dx) + dy * dy) + dz * dz);
}

// one double per workgroup from one double per thread, in a fixed order
__device__ __forceinline__ void write_partial(double s, double* partial) {
    __shared__ double red[THREADS / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Is any block this workgroup needs set?  Its own run, and with BACK the block before the run and the runs of the rows b_y - 1 and b_z - 1.
template <bool BACK>
__device__ __forceinline__ bool any_block_set(const Args& a, int bz, int by, int bx0, int n) {
    const int i = threadIdx.x;
    const unsigned char* own = a.mask + ((size_t)bz * a.nBy + by) * a.nBx;
    int any = 0;
    if (i < n) any = own[bx0 + i];
    if (BACK) {
        if (i == n && bx0 > 0) any = own[bx0 - 1];
        if (i >= 64 && i < 64 + n && by > 0) any = own[bx0 + (i - 64) - a.nBx];
        if (i >= 128 && i < 128 + n && bz > 0) any = own[bx0 + (i - 128) - (ptrdiff_t)a.nBy * a.nBx];
    }
    return __syncthreads_or(any) != 0;
}

// ------------------------------------------------------------------------------------------------
// total variation
// ------------------------------------------------------------------------------------------------
template <int VEC, bool GRAD, bool VALUE>
__global__ __launch_bounds__(THREADS) void lattice_tv_kernel(const Args a) {
    using V = typename Vec<VEC>::type;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int bz = blockIdx.z, by = blockIdx.y, bx0 = blockIdx.x * a.WX;
    const int bx1 = bx0 + a.WX < a.nBx ? bx0 + a.WX : a.nBx;
    if (a.mask && !any_block_set<GRAD>(a, bz, by, bx0, bx1 - bx0)) {              // workgroup-uniform
        if (VALUE && threadIdx.x == 0) a.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    // the points of the tile: 8 per block and axis, and the last block of an axis also holds the lattice's last point
    const int z0 = bz * BLOCK, z1 = bz == a.nBz - 1 ? a.Pz : z0 + BLOCK;
    const int y0 = by * BLOCK, y1 = by == a.nBy - 1 ? a.Py : y0 + BLOCK;
    const int x0 = bx0 * BLOCK, x1 = bx1 == a.nBx ? a.Px : bx1 * BLOCK;
    const int U = a.R / VEC;                          // units of VEC floats per point: 1, 4 or 8
    const int UC = (a.C + VEC - 1) / VEC;             // ... that hold a counted channel
    const int logU = U == 8 ? 3 : U == 4 ? 2 : 0;
    const int sx = a.R, sy = a.Px * a.R, sz = a.Py * sy;            // at most 513 * 513 * 32 floats
    const unsigned char* m_own = a.mask ? a.mask + ((size_t)bz * a.nBy + by) * a.nBx : nullptr;
    double acc = 0.0;

    for (int z = z0; z < z1; ++z) {
        const bool hasz = z + 1 < a.Pz;
        // the mask row of p - e_z: this block row inside the tile, the row of b_z - 1 at its first plane
        const unsigned char* m_z = !a.mask ? nullptr : z > z0 ? m_own : m_own - (ptrdiff_t)a.nBy * a.nBx;
        for (int y = y0 + ty; y < y1; y += THREADS / 64) {
            const bool hasy = y + 1 < a.Py;
            const unsigned char* m_y = !a.mask ? nullptr : y > y0 ? m_own : m_own - a.nBx;
            for (int u = x0 * U + tx; u < x1 * U; u += 64) {
                const int x = u >> logU, cg = u & (U - 1);
                if (cg >= UC) continue;                                         // a unit of padding alone
                const int nc = a.C - cg * VEC < VEC ? a.C - cg * VEC : VEC;     // counted channels of this unit
                const bool hasx = x + 1 < a.Px;
                const int bxp = (x < a.Px - 2 ? x : a.Px - 2) >> 3;
                const bool c0 = !a.mask || m_own[bxp] != 0;
                const bool cx = GRAD && x >= 1 && (!a.mask || m_own[(x - 1) >> 3] != 0);
                const bool cy = GRAD && y >= 1 && (!a.mask || m_y[bxp] != 0);
                const bool cz = GRAD && z >= 1 && (!a.mask || m_z[bxp] != 0);
                if (!(c0 || cx || cy || cz)) continue;
                const long long at = (((long long)z * a.Py + y) * a.Px + x) * a.R + cg * VEC;
                auto ld = [&](int off) { return *reinterpret_cast<const V*>(a.v + at + off); };
                // An absent forward neighbour is read at the point itself and its difference set to exactly 0; a backward term that is not
                // counted is formed at the point itself and dropped.  Straight-line code: thirteen loads, four norms, four divisions.
                const int ox = hasx ? sx : 0, oy = hasy ? sy : 0, oz = hasz ? sz : 0;
                const int mx = cx ? -sx : 0, my = cy ? -sy : 0, mz = cz ? -sz : 0;
                const V v0 = ld(0), vxp = ld(ox), vyp = ld(oy), vzp = ld(oz);
                const V xm = ld(mx), xm_y = ld(mx + oy), xm_z = ld(mx + oz);
                const V ym = ld(my), ym_x = ld(my + ox), ym_z = ld(my + oz);
                const V zm = ld(mz), zm_x = ld(mz + ox), zm_y = ld(mz + oy);
                float g[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float w = comp(v0, j);
                    float own, b_x = 0.0f, b_y = 0.0f, b_z = 0.0f;
                    {
                        const float dx = hasx ? comp(vxp, j) - w : 0.0f, dy = hasy ? comp(vyp, j) - w : 0.0f, dz = hasz ? comp(vzp, j) - w : 0.0f;
                        const float t = tv_norm(a.eps, dx, dy, dz);
                        own = c0 ? -(((dx + dy) + dz) / t) : 0.0f;
                        if (VALUE) acc += (c0 && j < nc) ? (double)t : 0.0;
                    }
                    if (GRAD) {
                        const float qx = comp(xm, j), qy = comp(ym, j), qz = comp(zm, j);
                        const float dxx = w - qx, dxy = hasy ? comp(xm_y, j) - qx : 0.0f, dxz = hasz ? comp(xm_z, j) - qx : 0.0f;
                        const float dyx = hasx ? comp(ym_x, j) - qy : 0.0f, dyy = w - qy, dyz = hasz ? comp(ym_z, j) - qy : 0.0f;
                        const float dzx = hasx ? comp(zm_x, j) - qz : 0.0f, dzy = hasy ? comp(zm_y, j) - qz : 0.0f, dzz = w - qz;
                        b_x = cx ? dxx / tv_norm(a.eps, dxx, dxy, dxz) : 0.0f;
                        b_y = cy ? dyy / tv_norm(a.eps, dyx, dyy, dyz) : 0.0f;
                        b_z = cz ? dzz / tv_norm(a.eps, dzx, dzy, dzz) : 0.0f;
                    }
                    g[j] = ((own + b_x) + b_y) + b_z;
                }
                if (GRAD) {
                    float* o = a.d_v + at;
                    if (VEC == 4 && nc == 4) {
                        float4 d = *reinterpret_cast<const float4*>(o);
                        d.x = d.x + a.scale * g[0];
                        d.y = d.y + a.scale * g[VEC > 1 ? 1 : 0];
                        d.z = d.z + a.scale * g[VEC > 2 ? 2 : 0];
                        d.w = d.w + a.scale * g[VEC > 3 ? 3 : 0];
                        *reinterpret_cast<float4*>(o) = d;
                    } else {                                                     // the padding of a partly counted unit is not touched
#pragma unroll
                        for (int j = 0; j < VEC; ++j)
                            if (j < nc) o[j] = o[j] + a.scale * g[j];
                    }
                }
            }
        }
    }
    if (VALUE) write_partial(acc, a.partial);
}

// ------------------------------------------------------------------------------------------------
// sparsity (Cauchy) on a plane
// ------------------------------------------------------------------------------------------------
template <bool GRAD, bool VALUE>
__global__ __launch_bounds__(THREADS) void lattice_sparsity_kernel(const Args a) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int bz = blockIdx.z, by = blockIdx.y, bx0 = blockIdx.x * a.WX;
    const int bx1 = bx0 + a.WX < a.nBx ? bx0 + a.WX : a.nBx;
    if (a.mask && !any_block_set<false>(a, bz, by, bx0, bx1 - bx0)) {
        if (VALUE && threadIdx.x == 0) a.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    const int z0 = bz * BLOCK, z1 = bz == a.nBz - 1 ? a.Pz : z0 + BLOCK;
    const int y0 = by * BLOCK, y1 = by == a.nBy - 1 ? a.Py : y0 + BLOCK;
    const int x0 = bx0 * BLOCK, x1 = bx1 == a.nBx ? a.Px : bx1 * BLOCK;
    const unsigned char* m_own = a.mask ? a.mask + ((size_t)bz * a.nBy + by) * a.nBx : nullptr;
    double acc = 0.0;
    for (int z = z0; z < z1; ++z)
        for (int y = y0 + ty; y < y1; y += THREADS / 64)
            for (int x = x0 + tx; x < x1; x += 64) {
                if (a.mask && m_own[(x < a.Px - 2 ? x : a.Px - 2) >> 3] == 0) continue;
                const long long at = ((long long)z * a.Py + y) * a.Px + x;
                const float s = a.v[at];
                if (GRAD) {
                    const float g = (4.0f * s) / (1.0f + (2.0f * s) * s);
                    a.d_v[at] = a.d_v[at] + a.scale * g;
                }
                if (VALUE) {
                    const double sd = (double)s;
                    acc += log1p((2.0 * sd) * sd);
                }
            }
    if (VALUE) write_partial(acc, a.partial);
}

// the partials in index order, THREADS runs of consecutive ones, then a fixed tree
__global__ __launch_bounds__(THREADS) void lattice_finish_kernel(const double* __restrict__ partial, int n, double* __restrict__ value) {
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const int per = (n + THREADS - 1) / THREADS;
    const int lo = tid * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += partial[i];
    red[tid] = s;
    __syncthreads();
    for (int w = THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) *value = red[0];
}

static bool shape_ok(const int32_t* P, int R, int C) {
    if (!P) return false;
    for (int i = 0; i < 3; ++i)
        if (P[i] < MIN_P || P[i] > MAX_P) return false;
    return (R == 1 || R == 4 || R == 16 || R == 32) && C >= 1 && C <= R;
}

static size_t array_bytes(const int32_t* P, int R) { return (size_t)P[0] * P[1] * P[2] * R * sizeof(float); }

static bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

// what both entries check before any HIP call
static int check_common(const char* who, const int32_t* P, int R, int C, const float* v, float scale, const float* d_v, const double* value_dev,
                        const void* scratch, size_t scratch_bytes) {
    LAT_CHECK_ARG(P != nullptr, "%s: P is NULL", who);
    LAT_CHECK_ARG(P[0] >= MIN_P && P[0] <= MAX_P && P[1] >= MIN_P && P[1] <= MAX_P && P[2] >= MIN_P && P[2] <= MAX_P,
                  "%s: P=(%d, %d, %d): every axis holds %d..%d points", who, (int)P[0], (int)P[1], (int)P[2], MIN_P, MAX_P);
    LAT_CHECK_ARG(R == 1 || R == 4 || R == 16 || R == 32, "%s: R=%d must be 1, 4, 16 or 32", who, R);
    LAT_CHECK_ARG(C >= 1 && C <= R, "%s: C=%d: 1..R=%d", who, C, R);
    LAT_CHECK_ARG(isfinite(scale), "%s: scale=%g is not finite", who, (double)scale);
    LAT_CHECK_ARG(v != nullptr, "%s: the array is NULL", who);
    const uintptr_t need = R > 1 ? 15 : 3;
    LAT_CHECK_ARG(((uintptr_t)v & need) == 0, "%s: the array must be %d-byte aligned", who, (int)need + 1);
    LAT_CHECK_ARG(((uintptr_t)d_v & need) == 0, "%s: the gradient array must be %d-byte aligned", who, (int)need + 1);
    LAT_CHECK_ARG(d_v == nullptr || !overlap(v, d_v, array_bytes(P, R)), "%s: the gradient array overlaps the array it is the gradient of", who);
    LAT_CHECK_ARG(((uintptr_t)value_dev & 7) == 0, "%s: value_dev must be 8-byte aligned", who);
    if (value_dev) {
        const size_t want = mi_geo_lattice_scratch_bytes(P, R, C);
        LAT_CHECK_ARG(scratch != nullptr && scratch_bytes >= want, "%s: scratch of %zu bytes given, %zu needed (mi_geo_lattice_scratch_bytes)", who,
                      scratch ? scratch_bytes : (size_t)0, want);
        LAT_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "%s: scratch must be 8-byte aligned", who);
    }
    return MI_GEO_OK;
}

static Args args_of(const int32_t* P, int R, int C, const float* v, const uint8_t* mask, float eps, float scale, float* d_v, void* scratch,
                    const Geometry& g) {
    Args a;
    a.v = v; a.d_v = d_v; a.mask = mask; a.partial = (double*)scratch;
    a.Pz = P[0]; a.Py = P[1]; a.Px = P[2]; a.R = R; a.C = C;
    a.nBz = g.nBz; a.nBy = g.nBy; a.nBx = g.nBx; a.WX = g.WX;
    a.eps = eps; a.scale = scale;
    return a;
}

}  // namespace milat

using namespace milat;

extern "C" {

size_t mi_geo_lattice_scratch_bytes(const int32_t P[3], int R, int C) {
    if (!shape_ok(P, R, C)) return 0;
    const Geometry g = geometry_of(P, R);
    return (size_t)g.nBz * g.nBy * g.nSX * sizeof(double);
}

int mi_geo_lattice_tv(const int32_t P[3], int R, int C, const float* v, const uint8_t* mask, float eps, float scale, float* d_v, double* value_dev,
                      void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "mi_geo_lattice_tv";
    const int rc = check_common(who, P, R, C, v, scale, d_v, value_dev, scratch, scratch_bytes);
    if (rc != MI_GEO_OK) return rc;
    LAT_CHECK_ARG(isfinite(eps) && eps > 0.0f, "%s: eps=%g must be positive and finite", who, (double)eps);
    if (!d_v && !value_dev) return MI_GEO_OK;
    const Geometry g = geometry_of(P, R);
    const Args a = args_of(P, R, C, v, mask, eps, scale, d_v, scratch, g);
    const dim3 grid(g.nSX, g.nBy, g.nBz), block(THREADS);
    hipStream_t s = (hipStream_t)stream;
#define LAT_TV(VV)                                                                                              \
    do {                                                                                                        \
        if (d_v && value_dev) hipLaunchKernelGGL((lattice_tv_kernel<VV, true, true>), grid, block, 0, s, a);    \
        else if (d_v) hipLaunchKernelGGL((lattice_tv_kernel<VV, true, false>), grid, block, 0, s, a);           \
        else hipLaunchKernelGGL((lattice_tv_kernel<VV, false, true>), grid, block, 0, s, a);                    \
    } while (0)
    if (R == 1) LAT_TV(1); else LAT_TV(4);
#undef LAT_TV
    LAT_LAUNCH_CHECK("lattice_tv_kernel");
    if (value_dev) {
        hipLaunchKernelGGL(lattice_finish_kernel, dim3(1), block, 0, s, (const double*)scratch, g.nBz * g.nBy * g.nSX, value_dev);
        LAT_LAUNCH_CHECK("lattice_finish_kernel");
    }
    return MI_GEO_OK;
}

int mi_geo_lattice_sparsity(const int32_t P[3], const float* sigma, const uint8_t* mask, float scale, float* d_sigma, double* value_dev,
                            void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "mi_geo_lattice_sparsity";
    const int rc = check_common(who, P, 1, 1, sigma, scale, d_sigma, value_dev, scratch, scratch_bytes);
    if (rc != MI_GEO_OK) return rc;
    if (!d_sigma && !value_dev) return MI_GEO_OK;
    const Geometry g = geometry_of(P, 1);
    const Args a = args_of(P, 1, 1, sigma, mask, 0.0f, scale, d_sigma, scratch, g);
    const dim3 grid(g.nSX, g.nBy, g.nBz), block(THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (d_sigma && value_dev) hipLaunchKernelGGL((lattice_sparsity_kernel<true, true>), grid, block, 0, s, a);
    else if (d_sigma) hipLaunchKernelGGL((lattice_sparsity_kernel<true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((lattice_sparsity_kernel<false, true>), grid, block, 0, s, a);
    LAT_LAUNCH_CHECK("lattice_sparsity_kernel");
    if (value_dev) {
        hipLaunchKernelGGL(lattice_finish_kernel, dim3(1), block, 0, s, (const double*)scratch, g.nBz * g.nBy * g.nSX, value_dev);
        LAT_LAUNCH_CHECK("lattice_finish_kernel");
    }
    return MI_GEO_OK;
}

}  // extern "C"
