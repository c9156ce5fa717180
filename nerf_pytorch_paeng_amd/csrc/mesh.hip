// mesh.hip -- libmi_nerf_mesh.so (include/mi_nerf_mesh.h): triangle meshes from a density lattice by marching tetrahedra on the Kuhn split of
// each cell.  A library of its own: it links against libmi_nerf.so and reaches the networks through the three public fused entries only.
//
// mesh_rows_kernel     a slab of lattice rows along x as rays (origin on the box face, direction +x) with depths
// mesh_density_kernel  channel 3 of raw [rows, P_x, 4] -> f (the slab loop around the two: row_slab.h)
// mesh_mark_kernel     one thread per lattice point: the crossed-edge mask (7 bits) and its popcount
// mesh_cells_kernel    one thread per cell: the number of triangles of its six tetrahedra
// scan_*_kernel        exclusive prefix sum of a uint32 array in place: block sums | one block over the block sums (+ the total) | apply
//                      (the bodies of block_scan.h)
// mesh_verts_kernel    one thread per lattice point: the vertices (and normals) of its crossed edges
// mesh_tris_kernel     one thread per cell: its triangles, vertex numbers looked up through mask + vfirst
//
// The case table (6 tetrahedra x 16 inside patterns) is computed at compile time FROM THE RULE of the header (tet_entry below); the
// numpy restatement in tests/test_mesh_cpu.py computes the rule a second time, from the header, without a table.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_mesh.h"
#include "abi_error.h"
#include "block_scan.h"
#include "row_slab.h"

namespace mimesh {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(, MI_MESH_EHIP)          // external linkage: mesh_view.hip declares the two functions and writes the same buffer
ABI_NERF_FAIL(MI_MESH_EINVAL, MI_MESH_EHIP)
#define MESH_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mimesh, MI_MESH_EINVAL, cond, __VA_ARGS__)
#define MESH_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mimesh, name)
#define MESH_NERF(call) ABI_NERF(::mimesh, call, #call)

constexpr int SCAN_TILE = MI_MESH_SCAN_TILE;          // 256 threads x 4 elements
static_assert(SCAN_TILE == miblock::SCAN_TILE, "block_scan.h and mi_nerf_mesh.h disagree on the scan's block");

// ---- the lattice as the kernels see it ---------------------------------------------------------------
struct Lattice {
    float lo[3], step[3];
    int P[3], res[3];
    long long N, C;             // points, cells: N <= 513^3 < 2^31
};

static int resolve_grid(const mi_mesh_grid* g, Lattice* out) {
    MESH_CHECK_ARG(g != nullptr, "grid is NULL");
    Lattice L;
    L.N = L.C = 1;
    for (int i = 0; i < 3; ++i) {
        MESH_CHECK_ARG(g->res[i] >= 1 && g->res[i] <= MI_MESH_MAX_RES, "grid res[%d]=%d: 1..%d", i, g->res[i], MI_MESH_MAX_RES);
        MESH_CHECK_ARG(isfinite(g->lo[i]) && isfinite(g->hi[i]) && g->lo[i] < g->hi[i], "grid box: lo[%d]=%g must be below hi[%d]=%g, both finite", i,
                       (double)g->lo[i], i, (double)g->hi[i]);
        const float ext = g->hi[i] - g->lo[i];
        L.lo[i] = g->lo[i];
        L.step[i] = ext / (float)g->res[i];
        MESH_CHECK_ARG(isfinite(ext) && L.step[i] > 0.0f, "grid box: extent %g of axis %d has no finite fp32 step above 0", (double)ext, i);
        L.res[i] = g->res[i];
        L.P[i] = g->res[i] + 1;
        L.N *= L.P[i];
        L.C *= L.res[i];
    }
    *out = L;
    return MI_MESH_OK;
}

// ---- the case table, from the rule -------------------------------------------------------------------
// corner k of tetrahedron q as a 3-bit offset code (bit i: +1 along axis i); entry (q, pattern): triangles << 24 | 2 x 3 edges of 4 bits
// (lower corner << 2 | higher corner), winding applied.  Pattern bit k: corner k is inside.
struct CaseTable {
    uint32_t entry[6 * 16];
    uint8_t code[6 * 4];
};

constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr int corner_code(int q, int k) { return k == 0 ? 0 : k == 1 ? (1 << PERM[q][0]) : k == 2 ? ((1 << PERM[q][0]) | (1 << PERM[q][1])) : 7; }

constexpr uint32_t tet_entry(int q, int pat) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
    for (int k = 0; k < 4; ++k) {
        if ((pat >> k) & 1) in[n_in++] = k;
        else out[n_out++] = k;
    }
    if (n_in == 0 || n_in == 4) return 0;
    int tri[2][3][2] = {};
    int nt = 1;
    if (n_in == 2) {
        const int A = in[0], B = in[1], Cc = out[0], D = out[1];
        const int t0[3][2] = {{A, Cc}, {A, D}, {B, D}}, t1[3][2] = {{A, Cc}, {B, D}, {B, Cc}};
        for (int k = 0; k < 3; ++k)
            for (int s = 0; s < 2; ++s) { tri[0][k][s] = t0[k][s]; tri[1][k][s] = t1[k][s]; }
        nt = 2;
    } else {
        const int A = n_in == 1 ? in[0] : out[0];
        const int* rest = n_in == 1 ? out : in;
        for (int k = 0; k < 3; ++k) { tri[0][k][0] = A; tri[0][k][1] = rest[k]; }
    }
    // centroid of the outside corners minus centroid of the inside corners, times n_in * n_out
    int d[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) {
        int s_in = 0, s_out = 0;
        for (int k = 0; k < n_in; ++k) s_in += (corner_code(q, in[k]) >> i) & 1;
        for (int k = 0; k < n_out; ++k) s_out += (corner_code(q, out[k]) >> i) & 1;
        d[i] = s_out * n_in - s_in * n_out;
    }
    uint32_t e = (uint32_t)nt << 24;
    for (int t = 0; t < nt; ++t) {
        int m[3][3] = {};
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) m[k][i] = ((corner_code(q, tri[t][k][0]) >> i) & 1) + ((corner_code(q, tri[t][k][1]) >> i) & 1);
        const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]}, v[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
        const int dot = (u[1] * v[2] - u[2] * v[1]) * d[0] + (u[2] * v[0] - u[0] * v[2]) * d[1] + (u[0] * v[1] - u[1] * v[0]) * d[2];
        const int order[3] = {0, dot < 0 ? 2 : 1, dot < 0 ? 1 : 2};
        for (int k = 0; k < 3; ++k) {
            const int a = tri[t][order[k]][0], b = tri[t][order[k]][1];
            e |= (uint32_t)(((a < b ? a : b) << 2) | (a < b ? b : a)) << (12 * t + 4 * k);
        }
    }
    return e;
}

constexpr CaseTable make_table() {
    CaseTable T{};
    for (int q = 0; q < 6; ++q) {
        for (int p = 0; p < 16; ++p) T.entry[q * 16 + p] = tet_entry(q, p);
        for (int k = 0; k < 4; ++k) T.code[q * 4 + k] = (uint8_t)corner_code(q, k);
    }
    return T;
}

__constant__ const CaseTable k_table = make_table();

// ---- network -> lattice ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_rows_kernel(Lattice L, long long row0, long long n_rows, float* __restrict__ rays, float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int Px = L.P[0];
    if (i >= n_rows * Px) return;
    const long long r = i / Px;
    const int jx = (int)(i - r * Px);
    z[i] = (float)jx * L.step[0];
    if (jx == 0) {
        const long long row = row0 + r;
        const int jz = (int)(row / L.P[1]), jy = (int)(row - (long long)jz * L.P[1]);
        float* rp = rays + r * 6;
        rp[0] = L.lo[0];
        rp[1] = L.lo[1] + (float)jy * L.step[1];
        rp[2] = L.lo[2] + (float)jz * L.step[2];
        rp[3] = 1.0f;
        rp[4] = 0.0f;
        rp[5] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void mesh_density_kernel(long long n_pts, const float* __restrict__ raw, float* __restrict__ f) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pts) f[i] = raw[i * 4 + 3];
}

// ---- count -------------------------------------------------------------------------------------------
__device__ __forceinline__ void point_of(const Lattice& L, int i, int j[3]) {
    const int row = i / L.P[0];
    j[0] = i - row * L.P[0];
    j[2] = row / L.P[1];
    j[1] = row - j[2] * L.P[1];
}

__global__ __launch_bounds__(256) void mesh_mark_kernel(Lattice L, const float* __restrict__ f, float iso, uint8_t* __restrict__ mask,
                                                        uint32_t* __restrict__ vcount) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.N) return;
    int j[3];
    point_of(L, (int)i, j);
    const bool in = f[i] > iso;                                         // a NaN is outside
    const int sy = L.P[0], sz = L.P[0] * L.P[1];
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const int dx = (e + 1) & 1, dy = ((e + 1) >> 1) & 1, dz = ((e + 1) >> 2) & 1;
        if (j[0] + dx < L.P[0] && j[1] + dy < L.P[1] && j[2] + dz < L.P[2]) {
            const bool in_b = f[i + dx + dy * sy + dz * sz] > iso;
            if (in != in_b) m |= 1u << e;
        }
    }
    mask[i] = (uint8_t)m;
    vcount[i] = __popc(m);
}

__global__ __launch_bounds__(256) void mesh_cells_kernel(Lattice L, const float* __restrict__ f, float iso, uint32_t* __restrict__ tcount) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= L.C) return;
    const int row = (int)(c / L.res[0]);
    const int cx = (int)(c - (long long)row * L.res[0]), cz = row / L.res[1], cy = row - cz * L.res[1];
    const int sy = L.P[0], sz = L.P[0] * L.P[1];
    const long long p0 = ((long long)cz * L.P[1] + cy) * L.P[0] + cx;
    unsigned in = 0;                                                     // bit code: corner c + code is inside
#pragma unroll
    for (int code = 0; code < 8; ++code)
        if (f[p0 + (code & 1) + ((code >> 1) & 1) * sy + ((code >> 2) & 1) * sz] > iso) in |= 1u << code;
    unsigned n = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        unsigned pat = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) pat |= ((in >> k_table.code[q * 4 + k]) & 1u) << k;
        n += k_table.entry[q * 16 + pat] >> 24;
    }
    tcount[c] = n;
}

// the scan's three launches (block_scan.h), on uint32
__global__ __launch_bounds__(256) void scan_reduce_kernel(const uint32_t* __restrict__ data, long long n, uint32_t* __restrict__ bsum) {
    miblock::scan_reduce(data, n, bsum);
}

// one block: block sums -> their exclusive prefix sums in place, the grand total to *total (the totals stay below 2^32: at most 7 vertices
// per point and 12 triangles per cell of a 513^3 lattice)
__global__ __launch_bounds__(1024) void scan_sums_kernel(uint32_t* __restrict__ bsum, int nb, unsigned long long* __restrict__ total) {
    const uint32_t carry = miblock::scan_sums(bsum, nb);
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* __restrict__ data, long long n, const uint32_t* __restrict__ bsum) {
    miblock::scan_apply(data, n, bsum);
}

// ---- emit --------------------------------------------------------------------------------------------
// gradient of f at lattice point i = flat(j): central differences, one-sided at the lattice boundary
__device__ __forceinline__ void gradient(const Lattice& L, const float* __restrict__ f, long long i, const int j[3], float g[3]) {
    const int stride[3] = {1, L.P[0], L.P[0] * L.P[1]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int s = stride[a];
        if (j[a] == 0) g[a] = (f[i + s] - f[i]) / L.step[a];
        else if (j[a] == L.P[a] - 1) g[a] = (f[i] - f[i - s]) / L.step[a];
        else g[a] = (f[i + s] - f[i - s]) / (2.0f * L.step[a]);
    }
}

__global__ __launch_bounds__(256) void mesh_verts_kernel(Lattice L, const float* __restrict__ f, float iso, const uint8_t* __restrict__ mask,
                                                         const uint32_t* __restrict__ vfirst, unsigned long long n_verts, float* __restrict__ verts,
                                                         float* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.N) return;
    const unsigned m = mask[i];
    if (!m) return;
    int j[3];
    point_of(L, (int)i, j);
    const float fa = f[i];
    float xa[3], ga[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 3; ++a) xa[a] = L.lo[a] + (float)j[a] * L.step[a];
    if (normals) gradient(L, f, i, j, ga);
    const int sy = L.P[0], sz = L.P[0] * L.P[1];
    unsigned long long v = vfirst[i];
    for (int e = 0; e < 7; ++e) {
        if (!((m >> e) & 1u)) continue;
        const int d[3] = {(e + 1) & 1, ((e + 1) >> 1) & 1, ((e + 1) >> 2) & 1};
        const long long ib = i + d[0] + d[1] * sy + d[2] * sz;
        float t = (iso - fa) / (f[ib] - fa);
        t = t > 0.0f ? t : 0.0f;                                          // fmaxf(t, 0.f): a NaN becomes 0
        t = t < 1.0f ? t : 1.0f;                                          // fminf(t, 1.f)
        if (v < n_verts) {
            const int jb[3] = {j[0] + d[0], j[1] + d[1], j[2] + d[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float xb = L.lo[a] + (float)jb[a] * L.step[a];
                verts[v * 3 + a] = xa[a] + t * (xb - xa[a]);
            }
            if (normals) {
                float gb[3], g[3];
                gradient(L, f, ib, jb, gb);
#pragma unroll
                for (int a = 0; a < 3; ++a) g[a] = ga[a] + t * (gb[a] - ga[a]);
                const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
                const bool ok = len > 0.0f && len < INFINITY;             // a NaN fails the first
#pragma unroll
                for (int a = 0; a < 3; ++a) normals[v * 3 + a] = ok ? -g[a] / len : 0.0f;
            }
        }
        ++v;
    }
}

__global__ __launch_bounds__(256) void mesh_tris_kernel(Lattice L, const float* __restrict__ f, float iso, const uint8_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ vfirst, const uint32_t* __restrict__ tfirst,
                                                        unsigned long long n_tris, int32_t* __restrict__ tris) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= L.C) return;
    const int row = (int)(c / L.res[0]);
    const int cx = (int)(c - (long long)row * L.res[0]), cz = row / L.res[1], cy = row - cz * L.res[1];
    const int sy = L.P[0], sz = L.P[0] * L.P[1];
    const long long p0 = ((long long)cz * L.P[1] + cy) * L.P[0] + cx;
    unsigned in = 0;
#pragma unroll
    for (int code = 0; code < 8; ++code)
        if (f[p0 + (code & 1) + ((code >> 1) & 1) * sy + ((code >> 2) & 1) * sz] > iso) in |= 1u << code;
    if (in == 0u || in == 255u) return;
    unsigned long long t_out = tfirst[c];
    for (int q = 0; q < 6; ++q) {
        unsigned pat = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) pat |= ((in >> k_table.code[q * 4 + k]) & 1u) << k;
        const uint32_t entry = k_table.entry[q * 16 + pat];
        const int nt = (int)(entry >> 24);
        for (int t = 0; t < nt; ++t, ++t_out) {
            if (t_out >= n_tris) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned nib = (entry >> (12 * t + 4 * k)) & 15u;
                const int ca = k_table.code[q * 4 + (nib >> 2)], cb = k_table.code[q * 4 + (nib & 3u)];
                const long long pa = p0 + (ca & 1) + ((ca >> 1) & 1) * sy + ((ca >> 2) & 1) * sz;
                const int e = (cb - ca) - 1;                                 // the corners of a tetrahedron grow: cb contains ca
                tris[t_out * 3 + k] = (int32_t)(vfirst[pa] + __popc(mask[pa] & ((1u << e) - 1u)));
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------
// the lattice's rows along x through a network, slab by slab (row_slab.h): P_x points a row, P_y P_z rows
static inline long long lattice_rows(const Lattice& L) { return (long long)L.P[1] * L.P[2]; }
static inline size_t density_scratch_bytes(const Lattice& L) {
    return rowslab::slab_bytes(rowslab::min_rows(lattice_rows(L), L.P[0], MI_MESH_MIN_SLAB_POINTS), L.P[0]);
}

static int density(const mi_mesh_grid* grid, const mi_nerf_net* net, const void* packed, int mode, float* f, void* scratch, size_t scratch_bytes,
                   hipStream_t st) {
    Lattice L;
    if (int rc = resolve_grid(grid, &L)) return rc;
    rowslab::mlp_rays_fn fn;
    if (!rowslab::mlp_entry(set_error, "the density lattice", mode, &fn)) return MI_MESH_EINVAL;
    MESH_CHECK_ARG(net && packed && f && scratch, "NULL pointer (net, packed, f and scratch are required)");
    const int Px = L.P[0];
    rowslab::Slab slab;
    if (!rowslab::plan(set_error, "mi_mesh_density_scratch_bytes", Px, lattice_rows(L), MI_MESH_MIN_SLAB_POINTS, scratch, scratch_bytes, &slab)) return MI_MESH_EINVAL;
    float *rays = slab.rays, *z = slab.z, *raw = slab.raw;
    return rowslab::for_each(slab, [&](long long r0, long long nr) {
        hipLaunchKernelGGL(mesh_rows_kernel, dim3(blocks_for(nr * Px, 256)), dim3(256), 0, st, L, r0, nr, rays, z);
        MESH_LAUNCH_CHECK("mesh_rows_kernel");
        MESH_NERF(fn(net, packed, rays, z, nr, Px, raw, (void*)st));
        hipLaunchKernelGGL(mesh_density_kernel, dim3(blocks_for(nr * Px, 256)), dim3(256), 0, st, nr * Px, raw, f + r0 * Px);
        MESH_LAUNCH_CHECK("mesh_density_kernel");
        return MI_MESH_OK;
    });
}

struct Scratch {
    size_t mask, vfirst, tfirst, sums, total;
};
static Scratch extract_layout(const Lattice& L) {
    Scratch S;
    size_t off = 0;
    S.mask = off;   off += align256((size_t)L.N);
    S.vfirst = off; off += align256((size_t)L.N * 4);
    S.tfirst = off; off += align256((size_t)L.C * 4);
    S.sums = off;   off += align256((size_t)((L.N + SCAN_TILE - 1) / SCAN_TILE) * 4);
    S.total = off;
    return S;
}

static int scan_in_place(uint32_t* data, long long n, uint32_t* sums, unsigned long long* total, hipStream_t st) {
    const unsigned nb = blocks_for(n, SCAN_TILE);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(256), 0, st, data, n, sums);
    MESH_LAUNCH_CHECK("scan_reduce_kernel");
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, (int)nb, total);
    MESH_LAUNCH_CHECK("scan_sums_kernel");
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(256), 0, st, data, n, sums);
    MESH_LAUNCH_CHECK("scan_apply_kernel");
    return MI_MESH_OK;
}

static int extract_args(const mi_mesh_grid* grid, const float* f, float iso, const void* scratch, size_t scratch_bytes, Lattice* L, Scratch* S) {
    if (int rc = resolve_grid(grid, L)) return rc;
    MESH_CHECK_ARG(f && scratch, "NULL pointer (f and scratch are required)");
    MESH_CHECK_ARG(!isnan(iso), "iso is NaN");
    MESH_CHECK_ARG(((uintptr_t)scratch & 255) == 0, "scratch must be 256-byte aligned");
    *S = extract_layout(*L);
    MESH_CHECK_ARG(scratch_bytes >= S->total, "scratch too small: %zu < %zu (mi_mesh_extract_scratch_bytes)", scratch_bytes, S->total);
    return MI_MESH_OK;
}

static int count(const mi_mesh_grid* grid, const float* f, float iso, void* scratch, size_t scratch_bytes, uint64_t* counts, hipStream_t st) {
    Lattice L;
    Scratch S;
    if (int rc = extract_args(grid, f, iso, scratch, scratch_bytes, &L, &S)) return rc;
    MESH_CHECK_ARG(counts != nullptr, "counts is NULL");
    MESH_CHECK_ARG(((uintptr_t)counts & 7) == 0, "counts must be 8-byte aligned");
    char* w = (char*)scratch;
    uint8_t* mask = (uint8_t*)(w + S.mask);
    uint32_t* vfirst = (uint32_t*)(w + S.vfirst);
    uint32_t* tfirst = (uint32_t*)(w + S.tfirst);
    uint32_t* sums = (uint32_t*)(w + S.sums);
    hipLaunchKernelGGL(mesh_mark_kernel, dim3(blocks_for(L.N, 256)), dim3(256), 0, st, L, f, iso, mask, vfirst);
    MESH_LAUNCH_CHECK("mesh_mark_kernel");
    if (int rc = scan_in_place(vfirst, L.N, sums, (unsigned long long*)counts, st)) return rc;
    hipLaunchKernelGGL(mesh_cells_kernel, dim3(blocks_for(L.C, 256)), dim3(256), 0, st, L, f, iso, tfirst);
    MESH_LAUNCH_CHECK("mesh_cells_kernel");
    return scan_in_place(tfirst, L.C, sums, (unsigned long long*)counts + 1, st);
}

static int emit(const mi_mesh_grid* grid, const float* f, float iso, const void* scratch, size_t scratch_bytes, uint64_t n_verts, uint64_t n_tris,
                float* verts, int32_t* tris, float* normals, hipStream_t st) {
    Lattice L;
    Scratch S;
    if (int rc = extract_args(grid, f, iso, scratch, scratch_bytes, &L, &S)) return rc;
    MESH_CHECK_ARG(n_verts <= 0x7fffffffull && n_tris <= 0x7fffffffull, "n_verts=%llu, n_tris=%llu: at most 2^31 - 1 each (int32 vertex numbers)",
                   (unsigned long long)n_verts, (unsigned long long)n_tris);
    MESH_CHECK_ARG((n_verts == 0 || verts) && (n_tris == 0 || tris), "NULL pointer (verts and tris are required where their count is not 0)");
    const char* w = (const char*)scratch;
    const uint8_t* mask = (const uint8_t*)(w + S.mask);
    const uint32_t* vfirst = (const uint32_t*)(w + S.vfirst);
    const uint32_t* tfirst = (const uint32_t*)(w + S.tfirst);
    if (n_verts > 0) {
        hipLaunchKernelGGL(mesh_verts_kernel, dim3(blocks_for(L.N, 256)), dim3(256), 0, st, L, f, iso, mask, vfirst, (unsigned long long)n_verts, verts, normals);
        MESH_LAUNCH_CHECK("mesh_verts_kernel");
    }
    if (n_tris > 0) {
        hipLaunchKernelGGL(mesh_tris_kernel, dim3(blocks_for(L.C, 256)), dim3(256), 0, st, L, f, iso, mask, vfirst, tfirst, (unsigned long long)n_tris, tris);
        MESH_LAUNCH_CHECK("mesh_tris_kernel");
    }
    return MI_MESH_OK;
}

}  // namespace mimesh

using namespace mimesh;

extern "C" {

int mi_mesh_abi_version(void) { return MI_MESH_ABI_VERSION; }
const char* mi_mesh_last_error(void) { return g_err; }

size_t mi_mesh_density_scratch_bytes(const mi_mesh_grid* grid) {
    Lattice L;
    return resolve_grid(grid, &L) == MI_MESH_OK ? density_scratch_bytes(L) : 0;
}

int mi_mesh_density(const mi_mesh_grid* grid, const mi_nerf_net* net, const void* packed, int mode, float* f, void* scratch, size_t scratch_bytes,
                    void* stream) {
    return density(grid, net, packed, mode, f, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t mi_mesh_extract_scratch_bytes(const mi_mesh_grid* grid) {
    Lattice L;
    return resolve_grid(grid, &L) == MI_MESH_OK ? extract_layout(L).total : 0;
}

int mi_mesh_count(const mi_mesh_grid* grid, const float* f, float iso, void* scratch, size_t scratch_bytes, uint64_t* counts, void* stream) {
    return count(grid, f, iso, scratch, scratch_bytes, counts, (hipStream_t)stream);
}

int mi_mesh_emit(const mi_mesh_grid* grid, const float* f, float iso, const void* scratch, size_t scratch_bytes, uint64_t n_verts, uint64_t n_tris,
                 float* verts, int32_t* tris, float* normals, void* stream) {
    return emit(grid, f, iso, scratch, scratch_bytes, n_verts, n_tris, verts, tris, normals, (hipStream_t)stream);
}

}  // extern "C"
