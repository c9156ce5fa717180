// occ.hip -- libmi_nerf_occ.so (include/mi_nerf_occ.h): occupancy-grid rendering.  The networks of an object scene are evaluated only at the
// samples a baked one-bit-per-cell density grid marks occupied; a skipped sample's raw output is (0,0,0,0), which post_process turns into
// weight 0 exactly.  A library of its own: it links against libmi_nerf.so and reaches the networks and the stages through public entries only.
//
// occ_mark_kernel      one thread per sample: THE CELL RULE of the header, as a uint8 mask
// occ_cull_kernel      one wave per ray: lookup per lane, ballot + prefix count -> compacted 32-sample tiles (pseudo-rays with S = 32), padded
//                      with the ray's last survivor; tiles are reserved with one atomic add per ray (tile ORDER varies from run to run, a
//                      sample's value does not: each lane of the network kernels evaluates its own point)
// occ_scatter_kernel   one thread per sample: raw[ray, sample] = tile value of a survivor, zeros otherwise (every element written)
// occ_compact_*_kernel the same compaction WITHOUT an atomic (mi_occ_compact): count per ray | exclusive scan of the tile counts | emit, so
//                      the tile order is a function of the input; cscan_*_kernel is the scan (block sums | one block over them | apply:
//                      the bodies of block_scan.h on 64-bit words)
// occ_gather_kernel    one thread per tile lane: the inverse of the scatter (d_raw of the training path), zeros on padding lanes
// occ_bake_gen_kernel  sub-lattice rows along x as rays (origin on the box face, direction +x) with depths (the slab loop: row_slab.h)
// occ_bake_reduce_kernel   OR of (density > sigma_min) over a cell's samples of one row, atomically ORed into the cell's bit
// occ_dilate_kernel    one thread per cell, neighbourhood OR, words assembled by ballot
// occ_count_kernel     popcount of the grid's cells
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_occ.h"
#include "abi_error.h"
#include "block_scan.h"
#include "row_slab.h"

namespace miocc {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_OCC_EHIP)
ABI_NERF_FAIL(MI_OCC_EINVAL, MI_OCC_EHIP)
#define OCC_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::miocc, MI_OCC_EINVAL, cond, __VA_ARGS__)
#define OCC_HIP(call) ABI_HIP(::miocc, call, #call)
#define OCC_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::miocc, name)
#define OCC_NERF(call) ABI_NERF(::miocc, call, #call)

constexpr int TILE = MI_OCC_TILE;

// ---- the grid as the kernels see it ----------------------------------------------------------------
struct GridDev {
    float lo[3], scale[3], fres[3];
    int res[3];
    int outside;
    long long cells;
};

static int resolve_grid(const mi_occ_grid* g, GridDev* out) {
    OCC_CHECK_ARG(g != nullptr, "grid is NULL");
    GridDev G;
    G.cells = 1;
    for (int i = 0; i < 3; ++i) {
        OCC_CHECK_ARG(g->res[i] >= 1 && g->res[i] <= MI_OCC_MAX_RES, "grid res[%d]=%d: 1..%d", i, g->res[i], MI_OCC_MAX_RES);
        OCC_CHECK_ARG(isfinite(g->lo[i]) && isfinite(g->hi[i]) && g->lo[i] < g->hi[i], "grid box: lo[%d]=%g must be below hi[%d]=%g, both finite", i,
                      (double)g->lo[i], i, (double)g->hi[i]);
        const float ext = g->hi[i] - g->lo[i];
        G.lo[i] = g->lo[i];
        G.scale[i] = (float)g->res[i] / ext;
        OCC_CHECK_ARG(isfinite(ext) && isfinite(G.scale[i]) && G.scale[i] > 0.0f, "grid box: extent %g of axis %d has no finite fp32 cell scale", (double)ext, i);
        G.fres[i] = (float)g->res[i];
        G.res[i] = g->res[i];
        G.cells *= g->res[i];
    }
    G.outside = g->outside_occupied != 0;
    *out = G;
    return MI_OCC_OK;
}

static inline size_t grid_words(const GridDev& G) { return (size_t)((G.cells + 31) / 32); }

// THE CELL RULE.  -ffp-contract=off: the product is rounded, then the sum (nerf_process.py:69-70).
__device__ __forceinline__ bool occ_lookup(const GridDev& G, const uint32_t* __restrict__ bits, const float o[3], const float d[3], float z) {
    float c[3];
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float p = o[i] + d[i] * z;
        c[i] = floorf((p - G.lo[i]) * G.scale[i]);
        inside = inside && c[i] >= 0.0f && c[i] < G.fres[i];          // a NaN fails both
    }
    if (!inside) return G.outside != 0;
    const int b = ((int)c[2] * G.res[1] + (int)c[1]) * G.res[0] + (int)c[0];
    return (bits[b >> 5] >> (b & 31)) & 1u;
}

__global__ __launch_bounds__(256) void occ_mark_kernel(GridDev G, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                                       const float* __restrict__ z, long long n_pts, int S, uint8_t* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;
    const float* rp = rays + (i / S) * 6;
    const float o[3] = {rp[0], rp[1], rp[2]}, d[3] = {rp[3], rp[4], rp[5]};
    mask[i] = occ_lookup(G, bits, o, d, z[i]) ? 1 : 0;
}

// ---- cull + compact --------------------------------------------------------------------------------
// One wave = one ray (4 per workgroup; no workgroup barrier).  The per-ray compaction is spelled once, for the atomic path
// (occ_cull_kernel) and the deterministic one (occ_compact_*_kernel): ray_survivors counts, ray_emit repeats the lookups and writes.
struct WaveRay {
    long long ray;
    const float* rp;            // its six floats
    const float* zr;            // its S depths
    float o[3], d[3];
    int lane;
};

__device__ __forceinline__ WaveRay wave_ray(const float* __restrict__ rays, const float* __restrict__ z, long long ray, int S) {
    const float* rp = rays + ray * 6;
    return WaveRay{ray, rp, z + ray * S, {rp[0], rp[1], rp[2]}, {rp[3], rp[4], rp[5]}, (int)(threadIdx.x & 63)};
}

// the ray's survivor count, the same in every lane: 64 lookups a round, ballot + popcount
__device__ __forceinline__ int ray_survivors(const GridDev& G, const uint32_t* __restrict__ bits, const WaveRay& w, int S) {
    int cnt = 0;
    for (int c = 0; c < S; c += 64) {
        const int s = c + w.lane;
        const bool occ = s < S && occ_lookup(G, bits, w.o, w.d, w.zr[s]);
        cnt += __popcll(__ballot(occ));
    }
    return cnt;
}

// the ray's tiles from tile `base` on: slot of every sample, tile_z / tile_src of the survivors in order, the last tile padded with the
// last survivor's depth, the ray copied once per tile.
__device__ __forceinline__ void ray_emit(const GridDev& G, const uint32_t* __restrict__ bits, const WaveRay& w, int S, long long base,
                                         float* __restrict__ tile_rays, float* __restrict__ tile_z, int* __restrict__ tile_src, int* __restrict__ slot) {
    const int lane = w.lane;
    const int j0 = (int)base * TILE;                                  // first flat tile lane of this ray
    int run = 0;
    float last_z = 0.0f;
    for (int c = 0; c < S; c += 64) {
        const int s = c + lane;
        const float zv = s < S ? w.zr[s] : 0.0f;
        const bool occ = s < S && occ_lookup(G, bits, w.o, w.d, zv);
        const unsigned long long m = __ballot(occ);
        const int j = j0 + run + __popcll(m & ((1ull << lane) - 1ull));
        if (s < S) slot[w.ray * S + s] = occ ? j : -1;
        if (occ) {
            tile_z[j] = zv;
            tile_src[j] = (int)(w.ray * S + s);
        }
        run += __popcll(m);
        if (m) last_z = __shfl(zv, 63 - __clzll((long long)m), 64);
    }
    const int ntiles = (run + TILE - 1) / TILE;
    const int pad = ntiles * TILE - run;                              // < 32
    if (lane < pad) {
        tile_z[j0 + run + lane] = last_z;
        tile_src[j0 + run + lane] = -1;
    }
    for (int i = lane; i < ntiles * 6; i += 64) tile_rays[base * 6 + i] = w.rp[i % 6];
}

// count, lane 0 reserves ceil(count / 32) tiles (counters[0] += tiles, counters[1] += survivors), emit
__global__ __launch_bounds__(256) void occ_cull_kernel(GridDev G, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                                       const float* __restrict__ z, long long n, int S, float* __restrict__ tile_rays,
                                                       float* __restrict__ tile_z, int* __restrict__ tile_src, int* __restrict__ slot,
                                                       unsigned* __restrict__ counters) {
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n) return;
    const WaveRay w = wave_ray(rays, z, ray, S);
    const int cnt = ray_survivors(G, bits, w, S);
    const int ntiles = (cnt + TILE - 1) / TILE;
    unsigned base = 0;
    if (w.lane == 0 && ntiles > 0) {
        base = atomicAdd(&counters[0], (unsigned)ntiles);
        atomicAdd(&counters[1], (unsigned)cnt);
    }
    base = __shfl(base, 0, 64);
    ray_emit(G, bits, w, S, (long long)base, tile_rays, tile_z, tile_src, slot);
}

__global__ __launch_bounds__(256) void occ_scatter_kernel(const int* __restrict__ slot, const float4* __restrict__ tile_raw, long long n_pts,
                                                          float4* __restrict__ raw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;
    const int j = slot[i];
    raw[i] = j >= 0 ? tile_raw[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- deterministic compaction ------------------------------------------------------------------------
// count | exclusive scan | emit.  One 64-bit word per ray carries both counts through ONE scan: tiles t_r in the low half, survivors k_r in
// the high half (sum t < 2^26 and sum k < 2^31 under the entry's size limit, so neither half carries into the other).
constexpr int CSCAN_TILE = miblock::SCAN_TILE;                         // 256 threads x 4 rays

__global__ __launch_bounds__(256) void occ_compact_count_kernel(GridDev G, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                                                const float* __restrict__ z, long long n, int S, unsigned long long* __restrict__ per_ray) {
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n) return;
    const WaveRay w = wave_ray(rays, z, ray, S);
    const int cnt = ray_survivors(G, bits, w, S);
    if (w.lane == 0) per_ray[ray] = ((unsigned long long)cnt << 32) | (unsigned long long)((cnt + TILE - 1) / TILE);
}

// the scan's three launches (block_scan.h), on the packed words
__global__ __launch_bounds__(256) void cscan_reduce_kernel(const unsigned long long* __restrict__ data, long long n, unsigned long long* __restrict__ bsum) {
    miblock::scan_reduce(data, n, bsum);
}

// one block: block sums -> their exclusive prefix sums in place; counts[0] = tiles, counts[1] = survivors of the whole batch
__global__ __launch_bounds__(1024) void cscan_sums_kernel(unsigned long long* __restrict__ bsum, int nb, unsigned* __restrict__ counts) {
    const unsigned long long carry = miblock::scan_sums(bsum, nb);
    if (threadIdx.x == 0) {
        counts[0] = (unsigned)(carry & 0xffffffffull);
        counts[1] = (unsigned)(carry >> 32);
    }
}

__global__ __launch_bounds__(256) void cscan_apply_kernel(unsigned long long* __restrict__ data, long long n, const unsigned long long* __restrict__ bsum) {
    miblock::scan_apply(data, n, bsum);
}

// the ray's first tile comes from the scan (low half of first[ray])
__global__ __launch_bounds__(256) void occ_compact_emit_kernel(GridDev G, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                                               const float* __restrict__ z, long long n, int S,
                                                               const unsigned long long* __restrict__ first, float* __restrict__ tile_rays,
                                                               float* __restrict__ tile_z, int* __restrict__ tile_src, int* __restrict__ slot) {
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n) return;
    const WaveRay w = wave_ray(rays, z, ray, S);
    ray_emit(G, bits, w, S, (long long)(first[ray] & 0xffffffffull), tile_rays, tile_z, tile_src, slot);
}

__global__ __launch_bounds__(256) void occ_gather_kernel(const int* __restrict__ tile_src, const float4* __restrict__ src, long long n_lanes,
                                                         float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lanes) return;
    const int j = tile_src[i];
    out[i] = j >= 0 ? src[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- bake ------------------------------------------------------------------------------------------
struct BakeGeom {
    float lo[3], step[3];
    int rx, ry, rz, sub;        // cells per axis
    int S;                      // rx * sub: lattice points of a row = depths of a ray
    long long rows;             // ry * sub * rz * sub
};

__global__ __launch_bounds__(256) void occ_bake_gen_kernel(BakeGeom B, long long row0, long long n_rows, float* __restrict__ rays, float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * B.S) return;
    const long long r = i / B.S;
    const int jx = (int)(i - r * B.S);
    z[i] = ((float)jx + 0.5f) * B.step[0];
    if (jx == 0) {
        const long long row = row0 + r;
        const int ny = B.ry * B.sub;
        const int jz = (int)(row / ny), jy = (int)(row - (long long)jz * ny);
        float* rp = rays + r * 6;
        rp[0] = B.lo[0];
        rp[1] = B.lo[1] + ((float)jy + 0.5f) * B.step[1];
        rp[2] = B.lo[2] + ((float)jz + 0.5f) * B.step[2];
        rp[3] = 1.0f;
        rp[4] = 0.0f;
        rp[5] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void occ_bake_reduce_kernel(BakeGeom B, long long row0, long long n_rows, const float* __restrict__ raw, float sigma_min,
                                                              uint32_t* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * B.rx) return;
    const long long r = i / B.rx;
    const int ix = (int)(i - r * B.rx);
    const float* p = raw + (r * B.S + (long long)ix * B.sub) * 4 + 3;
    bool any = false;
    for (int a = 0; a < B.sub; ++a) any = any || p[a * 4] > sigma_min;      // a NaN density is not above the threshold
    if (!any) return;
    const long long row = row0 + r;
    const int ny = B.ry * B.sub;
    const int jz = (int)(row / ny), jy = (int)(row - (long long)jz * ny);
    const int b = ((jz / B.sub) * B.ry + jy / B.sub) * B.rx + ix;
    atomicOr(&bits[b >> 5], 1u << (b & 31));
}

// ---- dilate, count ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void occ_dilate_kernel(GridDev G, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int radius) {
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    bool any = false;
    if (cell < G.cells) {
        const int rx = G.res[0], ry = G.res[1], rz = G.res[2];
        const int cx = (int)(cell % rx), cy = (int)((cell / rx) % ry), cz = (int)(cell / ((long long)rx * ry));
        for (int dz = -radius; dz <= radius; ++dz)
            for (int dy = -radius; dy <= radius; ++dy)
                for (int dx = -radius; dx <= radius; ++dx) {
                    const int x = cx + dx, y = cy + dy, zz = cz + dz;
                    if (x < 0 || x >= rx || y < 0 || y >= ry || zz < 0 || zz >= rz) continue;
                    const int b = (zz * ry + y) * rx + x;
                    any = any || ((in[b >> 5] >> (b & 31)) & 1u);
                }
    }
    const unsigned long long m = __ballot(any);                        // 64 consecutive cells: two words
    const int lane = threadIdx.x & 63;
    const long long w0 = (cell - lane) >> 5;                           // cell - lane is a multiple of 64
    const long long words = (G.cells + 31) >> 5;
    if (lane == 0 && w0 < words) out[w0] = (uint32_t)m;
    if (lane == 32 && w0 + 1 < words) out[w0 + 1] = (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(256) void occ_count_kernel(GridDev G, const uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    const long long words = (G.cells + 31) >> 5;
    unsigned long long c = 0;
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long long)gridDim.x * 256) {
        uint32_t v = bits[w];
        const long long left = G.cells - w * 32;                       // cells this word holds; the bits beyond them are not cells
        if (left < 32) v &= (1u << left) - 1u;
        c += __popc(v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// ---- host side -------------------------------------------------------------------------------------
static int resolve_bake(const mi_occ_grid* grid, int sub, GridDev* G, BakeGeom* B) {
    if (int rc = resolve_grid(grid, G)) return rc;
    OCC_CHECK_ARG(sub >= 1 && sub <= MI_OCC_MAX_SUB, "sub=%d: 1..%d lattice points per cell and axis", sub, MI_OCC_MAX_SUB);
    for (int i = 0; i < 3; ++i) {
        B->lo[i] = grid->lo[i];
        B->step[i] = (grid->hi[i] - grid->lo[i]) / (float)(grid->res[i] * sub);
    }
    B->rx = grid->res[0]; B->ry = grid->res[1]; B->rz = grid->res[2]; B->sub = sub;
    B->S = B->rx * sub;
    B->rows = (long long)B->ry * sub * B->rz * sub;
    return MI_OCC_OK;
}

// the sub-lattice's rows along x through a network, slab by slab (row_slab.h); the smallest slab holds 2^22 points
constexpr long long BAKE_MIN_SLAB_POINTS = 1LL << 22;
static inline size_t bake_scratch_bytes(const BakeGeom& B) { return rowslab::slab_bytes(rowslab::min_rows(B.rows, B.S, BAKE_MIN_SLAB_POINTS), B.S); }

using rowslab::mlp_rays_fn;
static int mlp_entry(int mode, mlp_rays_fn* fn) { return rowslab::mlp_entry(set_error, "the occupancy path", mode, fn) ? MI_OCC_OK : MI_OCC_EINVAL; }

static int bake(const mi_occ_grid* grid, uint32_t* bits, const mi_nerf_net* net, const void* packed, int mode, int sub, float sigma_min, int accumulate,
                void* scratch, size_t scratch_bytes, hipStream_t st) {
    GridDev G;
    BakeGeom B;
    if (int rc = resolve_bake(grid, sub, &G, &B)) return rc;
    mlp_rays_fn fn;
    if (int rc = mlp_entry(mode, &fn)) return rc;
    OCC_CHECK_ARG(bits && net && packed && scratch, "NULL pointer (bits, net, packed and scratch are required)");
    OCC_CHECK_ARG(!isnan(sigma_min), "sigma_min is NaN");
    rowslab::Slab slab;
    if (!rowslab::plan(set_error, "mi_occ_bake_scratch_bytes", B.S, B.rows, BAKE_MIN_SLAB_POINTS, scratch, scratch_bytes, &slab)) return MI_OCC_EINVAL;
    if (!accumulate) OCC_HIP(hipMemsetAsync(bits, 0, grid_words(G) * 4, st));
    float *rays = slab.rays, *z = slab.z, *raw = slab.raw;
    return rowslab::for_each(slab, [&](long long r0, long long nr) {
        hipLaunchKernelGGL(occ_bake_gen_kernel, dim3(blocks_for(nr * B.S, 256)), dim3(256), 0, st, B, r0, nr, rays, z);
        OCC_LAUNCH_CHECK("occ_bake_gen_kernel");
        OCC_NERF(fn(net, packed, rays, z, nr, B.S, raw, (void*)st));
        hipLaunchKernelGGL(occ_bake_reduce_kernel, dim3(blocks_for(nr * B.rx, 256)), dim3(256), 0, st, B, r0, nr, raw, sigma_min, bits);
        OCC_LAUNCH_CHECK("occ_bake_reduce_kernel");
        return MI_OCC_OK;
    });
}

// ---- render ----------------------------------------------------------------------------------------
static int render_layout(const mi_nerf_render_cfg* cfg, int64_t n, mi_occ_workspace_layout* L) {
    OCC_CHECK_ARG(cfg && L, "NULL cfg/layout");
    OCC_CHECK_ARG(n >= 0 && cfg->Sc >= 1 && cfg->Nf >= 0, "bad sizes n=%lld Sc=%d Nf=%d", (long long)n, cfg->Sc, cfg->Nf);
    OCC_CHECK_ARG(cfg->Nf == 0 || cfg->Sc >= 3, "hierarchical sampling needs at least 3 coarse samples");
    OCC_CHECK_ARG((long long)cfg->Sc + cfg->Nf <= 1024, "Sc + Nf = %lld: at most 1024 samples per ray (mi_nerf_composite)", (long long)cfg->Sc + cfg->Nf);
    const size_t nn = (size_t)n, Sc = (size_t)cfg->Sc, Nf = (size_t)cfg->Nf, St = Sc + Nf;
    OCC_CHECK_ARG((long long)n * (long long)(St + 31) < (1LL << 31), "n_rays=%lld x %zu samples: n_rays * (Sc + Nf + 31) must stay below 2^31", (long long)n, St);
    const size_t T = nn * ((St + TILE - 1) / TILE);
    size_t off = 0;
    L->z_c = off;       off += align256(nn * Sc * 4);
    L->raw_c = off;     off += align256(nn * Sc * 16);
    L->weights_c = off; off += align256(nn * Sc * 4);
    L->z_f = off;       off += Nf > 0 ? align256(nn * St * 4) : 0;
    L->raw_f = off;     off += Nf > 0 ? align256(nn * St * 16) : 0;
    L->t_rand = off;    off += align256(nn * Sc * 4);
    L->u = off;         off += Nf > 0 ? align256(nn * Nf * 4) : 0;
    L->slot = off;      off += align256(nn * St * 4);
    L->tile_rays = off; off += align256(T * 6 * 4);
    L->tile_z = off;    off += align256(T * TILE * 4);
    L->tile_src = off;  off += align256(T * TILE * 4);
    L->tile_raw = off;  off += align256(T * TILE * 16);
    L->counters = off;  off += 256;
    L->total = off;
    return MI_OCC_OK;
}

struct Pass {
    float* tile_rays; float* tile_z; int* tile_src; float* tile_raw; int* slot; unsigned* counters;
};

// cull -> count to the host -> network over the tiles -> scatter into raw [n,S,4]
static int network_pass(const GridDev& G, const uint32_t* bits, mlp_rays_fn fn, const mi_nerf_net* net, const void* packed, const float* rays, const float* z,
                        int64_t n, int S, const Pass& P, float* raw, int64_t* evaluated, int64_t* padded, hipStream_t st) {
    static thread_local unsigned* pinned = nullptr;                    // 8 bytes of pinned host memory per calling thread, kept
    if (!pinned) OCC_HIP(hipHostMalloc((void**)&pinned, 8, hipHostMallocPortable));       // portable: the thread may render on any device later; never freed
    OCC_HIP(hipMemsetAsync(P.counters, 0, 8, st));
    hipLaunchKernelGGL(occ_cull_kernel, dim3(blocks_for(n, 4)), dim3(256), 0, st, G, bits, rays, z, (long long)n, S, P.tile_rays, P.tile_z, P.tile_src, P.slot,
                       P.counters);
    OCC_LAUNCH_CHECK("occ_cull_kernel");
    OCC_HIP(hipMemcpyAsync(pinned, P.counters, 8, hipMemcpyDeviceToHost, st));
    OCC_HIP(hipStreamSynchronize(st));
    const int64_t tiles = pinned[0], survivors = pinned[1];
    *evaluated = survivors;
    *padded = tiles * TILE - survivors;
    if (tiles > 0) OCC_NERF(fn(net, packed, P.tile_rays, P.tile_z, tiles, TILE, P.tile_raw, (void*)st));
    hipLaunchKernelGGL(occ_scatter_kernel, dim3(blocks_for((long long)n * S, 256)), dim3(256), 0, st, P.slot, (const float4*)P.tile_raw, (long long)n * S,
                       (float4*)raw);
    OCC_LAUNCH_CHECK("occ_scatter_kernel");
    return MI_OCC_OK;
}

static int render(const mi_nerf_net* net, const void* packed_c, const void* packed_f, const mi_nerf_render_cfg* cfg, const mi_occ_grid* grid,
                  const uint32_t* bits_c, const uint32_t* bits_f, const float* rays, int64_t n, const float* t_rand, const float* u, void* ws, size_t ws_bytes,
                  float* rgb_c, float* disp_c, float* rgb_f, float* disp_f, mi_occ_stats* stats, hipStream_t st) {
    mi_occ_workspace_layout L;
    if (int rc = render_layout(cfg, n, &L)) return rc;
    GridDev G;
    if (int rc = resolve_grid(grid, &G)) return rc;
    mlp_rays_fn fn;
    if (int rc = mlp_entry(cfg->mode, &fn)) return rc;
    OCC_CHECK_ARG(cfg->reserved == 0, "mi_nerf_render_cfg.reserved must be 0");
    OCC_CHECK_ARG(net != nullptr, "net is NULL");
    OCC_CHECK_ARG(rays && rgb_c && disp_c && packed_c && bits_c && ws, "NULL pointer (rays, rgb_c, disp_c, packed_coarse, bits_coarse and workspace are required)");
    OCC_CHECK_ARG(cfg->Nf == 0 || (packed_f && bits_f && rgb_f && disp_f), "the fine pass needs packed_fine, bits_fine and its outputs");
    OCC_CHECK_ARG(ws_bytes >= L.total, "workspace too small: %zu < %zu", ws_bytes, L.total);
    OCC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
    if (stats) *stats = mi_occ_stats{0, 0, 0, 0, 0, 0};
    if (n == 0) return MI_OCC_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    OCC_HIP(hipStreamIsCapturing(st, &cap));
    OCC_CHECK_ARG(cap == hipStreamCaptureStatusNone, "the stream is being captured: mi_occ_render_rays synchronises it once per network pass and cannot be recorded into a graph");
    char* w = (char*)ws;
    float* z_c = (float*)(w + L.z_c);
    float* raw_c = (float*)(w + L.raw_c);
    float* wts_c = (float*)(w + L.weights_c);
    const Pass P{(float*)(w + L.tile_rays), (float*)(w + L.tile_z), (int*)(w + L.tile_src), (float*)(w + L.tile_raw), (int*)(w + L.slot), (unsigned*)(w + L.counters)};
    const int Sc = cfg->Sc, St = cfg->Sc + cfg->Nf;
    mi_occ_stats s{0, 0, 0, 0, 0, 0};
    if (!t_rand) {
        float* tr = (float*)(w + L.t_rand);
        OCC_NERF(mi_nerf_fill_uniform(cfg->seed, 0, cfg->ray_offset, n, Sc, tr, (void*)st));
        t_rand = tr;
    }
    OCC_NERF(mi_nerf_stratified_z(n, Sc, cfg->near_, cfg->far_, t_rand, z_c, (void*)st));
    s.total_c = n * Sc;
    if (int rc = network_pass(G, bits_c, fn, net, packed_c, rays, z_c, n, Sc, P, raw_c, &s.evaluated_c, &s.padded_c, st)) return rc;
    OCC_NERF(mi_nerf_composite(raw_c, z_c, rays, 6, n, Sc, rgb_c, disp_c, nullptr, wts_c, nullptr, (void*)st));
    if (cfg->Nf > 0) {
        float* z_f = (float*)(w + L.z_f);
        float* raw_f = (float*)(w + L.raw_f);
        if (!cfg->det && !u) {
            float* ub = (float*)(w + L.u);
            OCC_NERF(mi_nerf_fill_uniform(cfg->seed, 1, cfg->ray_offset, n, cfg->Nf, ub, (void*)st));
            u = ub;
        }
        OCC_NERF(mi_nerf_fine_z(z_c, wts_c, n, Sc, cfg->Nf, cfg->det, cfg->det ? nullptr : u, z_f, nullptr, (void*)st));
        s.total_f = n * St;
        if (int rc = network_pass(G, bits_f, fn, net, packed_f, rays, z_f, n, St, P, raw_f, &s.evaluated_f, &s.padded_f, st)) return rc;
        OCC_NERF(mi_nerf_composite(raw_f, z_f, rays, 6, n, St, rgb_f, disp_f, nullptr, nullptr, nullptr, (void*)st));
    }
    if (stats) *stats = s;
    return MI_OCC_OK;
}

// ---- deterministic compaction, scatter, gather (host side) -------------------------------------------
static inline size_t compact_scratch_bytes(int64_t n) {
    const size_t nb = ((size_t)n + CSCAN_TILE - 1) / CSCAN_TILE;
    return align256((size_t)n * 8) + align256(nb * 8) + 256;         // never 0: 0 is the refusal
}

// the sizes every entry of the training surface accepts: int32 tile lanes
static int check_tile_sizes(int64_t n, int S) {
    OCC_CHECK_ARG(n >= 0, "bad size n_rays=%lld", (long long)n);
    OCC_CHECK_ARG(S >= 1 && S <= 1024, "S=%d: 1..1024 samples per ray", S);
    OCC_CHECK_ARG((long long)n * ((S + TILE - 1) / TILE) * TILE < (1LL << 31), "n_rays=%lld x %d samples: n_rays * ceil(S / 32) * 32 must stay below 2^31",
                  (long long)n, S);
    return MI_OCC_OK;
}

static int compact(const mi_occ_grid* grid, const uint32_t* bits, const float* rays, const float* z, int64_t n, int S, float* tile_rays, float* tile_z,
                   int* tile_src, int* slot, unsigned* counts, void* scratch, size_t scratch_bytes, hipStream_t st) {
    GridDev G;
    if (int rc = resolve_grid(grid, &G)) return rc;
    if (int rc = check_tile_sizes(n, S)) return rc;
    OCC_CHECK_ARG(counts != nullptr, "counts is NULL");
    OCC_CHECK_ARG(((uintptr_t)counts & 3) == 0, "counts must be 4-byte aligned");
    if (n == 0) {
        OCC_HIP(hipMemsetAsync(counts, 0, 8, st));
        return MI_OCC_OK;
    }
    OCC_CHECK_ARG(bits && rays && z && tile_rays && tile_z && tile_src && slot && scratch,
                  "NULL pointer (bits, rays, z, tile_rays, tile_z, tile_src, slot, counts and scratch are required)");
    OCC_CHECK_ARG(((uintptr_t)scratch & 255) == 0, "scratch must be 256-byte aligned");
    const size_t need = compact_scratch_bytes(n);
    OCC_CHECK_ARG(scratch_bytes >= need, "scratch too small: %zu < %zu (mi_occ_compact_scratch_bytes)", scratch_bytes, need);
    unsigned long long* per_ray = (unsigned long long*)scratch;
    unsigned long long* sums = (unsigned long long*)((char*)scratch + align256((size_t)n * 8));
    const unsigned nb = blocks_for(n, CSCAN_TILE);
    hipLaunchKernelGGL(occ_compact_count_kernel, dim3(blocks_for(n, 4)), dim3(256), 0, st, G, bits, rays, z, (long long)n, S, per_ray);
    OCC_LAUNCH_CHECK("occ_compact_count_kernel");
    hipLaunchKernelGGL(cscan_reduce_kernel, dim3(nb), dim3(256), 0, st, per_ray, (long long)n, sums);
    OCC_LAUNCH_CHECK("cscan_reduce_kernel");
    hipLaunchKernelGGL(cscan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, (int)nb, counts);
    OCC_LAUNCH_CHECK("cscan_sums_kernel");
    hipLaunchKernelGGL(cscan_apply_kernel, dim3(nb), dim3(256), 0, st, per_ray, (long long)n, sums);
    OCC_LAUNCH_CHECK("cscan_apply_kernel");
    hipLaunchKernelGGL(occ_compact_emit_kernel, dim3(blocks_for(n, 4)), dim3(256), 0, st, G, bits, rays, z, (long long)n, S, per_ray, tile_rays, tile_z, tile_src,
                       slot);
    OCC_LAUNCH_CHECK("occ_compact_emit_kernel");
    return MI_OCC_OK;
}

}  // namespace miocc

using namespace miocc;

extern "C" {

int mi_occ_abi_version(void) { return MI_OCC_ABI_VERSION; }
const char* mi_occ_last_error(void) { return g_err; }

size_t mi_occ_grid_words(const mi_occ_grid* grid) {
    GridDev G;
    return resolve_grid(grid, &G) == MI_OCC_OK ? grid_words(G) : 0;
}

size_t mi_occ_bake_scratch_bytes(const mi_occ_grid* grid, int sub) {
    GridDev G;
    BakeGeom B;
    if (resolve_bake(grid, sub, &G, &B) != MI_OCC_OK) return 0;
    return bake_scratch_bytes(B);
}

int mi_occ_bake(const mi_occ_grid* grid, uint32_t* bits, const mi_nerf_net* net, const void* packed, int mode, int sub, float sigma_min, int accumulate,
                void* scratch, size_t scratch_bytes, void* stream) {
    return bake(grid, bits, net, packed, mode, sub, sigma_min, accumulate, scratch, scratch_bytes, (hipStream_t)stream);
}

int mi_occ_dilate(const mi_occ_grid* grid, const uint32_t* bits_in, uint32_t* bits_out, int radius, void* stream) {
    GridDev G;
    if (int rc = resolve_grid(grid, &G)) return rc;
    OCC_CHECK_ARG(radius >= 0 && radius <= MI_OCC_MAX_RADIUS, "radius=%d: 0..%d", radius, MI_OCC_MAX_RADIUS);
    OCC_CHECK_ARG(bits_in && bits_out, "NULL pointer");
    OCC_CHECK_ARG(bits_in != bits_out, "mi_occ_dilate works out of place: bits_out must not be bits_in");
    hipLaunchKernelGGL(occ_dilate_kernel, dim3(blocks_for(G.cells, 256)), dim3(256), 0, (hipStream_t)stream, G, bits_in, bits_out, radius);
    OCC_LAUNCH_CHECK("occ_dilate_kernel");
    return MI_OCC_OK;
}

int mi_occ_count(const mi_occ_grid* grid, const uint32_t* bits, uint64_t* count, void* stream) {
    GridDev G;
    if (int rc = resolve_grid(grid, &G)) return rc;
    OCC_CHECK_ARG(bits && count, "NULL pointer");
    OCC_CHECK_ARG(((uintptr_t)count & 7) == 0, "count must be 8-byte aligned");
    OCC_HIP(hipMemsetAsync(count, 0, 8, (hipStream_t)stream));
    const long long words = (long long)grid_words(G);
    const unsigned nb = blocks_for(words, 256) < 1024 ? blocks_for(words, 256) : 1024;
    hipLaunchKernelGGL(occ_count_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, G, bits, (unsigned long long*)count);
    OCC_LAUNCH_CHECK("occ_count_kernel");
    return MI_OCC_OK;
}

int mi_occ_mark(const mi_occ_grid* grid, const uint32_t* bits, const float* rays, const float* z, int64_t n_rays, int S, uint8_t* mask, void* stream) {
    GridDev G;
    if (int rc = resolve_grid(grid, &G)) return rc;
    OCC_CHECK_ARG(n_rays >= 0 && S >= 1 && (long long)n_rays * S < (1LL << 38), "bad sizes n_rays=%lld S=%d", (long long)n_rays, S);
    if (n_rays == 0) return MI_OCC_OK;
    OCC_CHECK_ARG(bits && rays && z && mask, "NULL pointer");
    hipLaunchKernelGGL(occ_mark_kernel, dim3(blocks_for((long long)n_rays * S, 256)), dim3(256), 0, (hipStream_t)stream, G, bits, rays, z, (long long)n_rays * S, S,
                       mask);
    OCC_LAUNCH_CHECK("occ_mark_kernel");
    return MI_OCC_OK;
}

size_t mi_occ_compact_scratch_bytes(int64_t n_rays) {
    if (n_rays < 0 || n_rays >= (1LL << 26)) {
        set_error("n_rays=%lld: 0 .. 2^26 - 1 rays (n_rays * 32 tile lanes stay below 2^31)", (long long)n_rays);
        return 0;
    }
    return compact_scratch_bytes(n_rays);
}

int mi_occ_compact(const mi_occ_grid* grid, const uint32_t* bits, const float* rays, const float* z, int64_t n_rays, int S, float* tile_rays, float* tile_z,
                   int32_t* tile_src, int32_t* slot, uint32_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
    return compact(grid, bits, rays, z, n_rays, S, tile_rays, tile_z, tile_src, slot, counts, scratch, scratch_bytes, (hipStream_t)stream);
}

int mi_occ_scatter_raw(const float* tile_vals, const int32_t* slot, int64_t n_rays, int S, float* out, void* stream) {
    if (int rc = check_tile_sizes(n_rays, S)) return rc;
    if (n_rays == 0) return MI_OCC_OK;
    OCC_CHECK_ARG(tile_vals && slot && out, "NULL pointer (tile_vals, slot and out are required)");
    OCC_CHECK_ARG((((uintptr_t)tile_vals | (uintptr_t)out) & 15) == 0, "tile_vals and out must be 16-byte aligned");
    const long long n_pts = (long long)n_rays * S;
    hipLaunchKernelGGL(occ_scatter_kernel, dim3(blocks_for(n_pts, 256)), dim3(256), 0, (hipStream_t)stream, slot, (const float4*)tile_vals, n_pts, (float4*)out);
    OCC_LAUNCH_CHECK("occ_scatter_kernel");
    return MI_OCC_OK;
}

int mi_occ_gather_raw(const float* src, const int32_t* tile_src, int64_t n_tiles, float* out, void* stream) {
    OCC_CHECK_ARG(n_tiles >= 0 && n_tiles * TILE < (1LL << 31), "n_tiles=%lld: n_tiles * 32 must stay below 2^31", (long long)n_tiles);
    if (n_tiles == 0) return MI_OCC_OK;
    OCC_CHECK_ARG(src && tile_src && out, "NULL pointer (src, tile_src and out are required)");
    OCC_CHECK_ARG((((uintptr_t)src | (uintptr_t)out) & 15) == 0, "src and out must be 16-byte aligned");
    const long long n_lanes = (long long)n_tiles * TILE;
    hipLaunchKernelGGL(occ_gather_kernel, dim3(blocks_for(n_lanes, 256)), dim3(256), 0, (hipStream_t)stream, tile_src, (const float4*)src, n_lanes, (float4*)out);
    OCC_LAUNCH_CHECK("occ_gather_kernel");
    return MI_OCC_OK;
}

size_t mi_occ_render_workspace_bytes(const mi_nerf_render_cfg* cfg, int64_t n_rays) {
    mi_occ_workspace_layout L;
    return render_layout(cfg, n_rays, &L) == MI_OCC_OK ? L.total : 0;
}

int mi_occ_render_workspace_layout(const mi_nerf_render_cfg* cfg, int64_t n_rays, mi_occ_workspace_layout* out) { return render_layout(cfg, n_rays, out); }

int mi_occ_render_rays(const mi_nerf_net* net, const void* packed_c, const void* packed_f, const mi_nerf_render_cfg* cfg, const mi_occ_grid* grid,
                       const uint32_t* bits_c, const uint32_t* bits_f, const float* rays, int64_t n_rays, const float* t_rand, const float* u, void* ws,
                       size_t ws_bytes, float* rgb_c, float* disp_c, float* rgb_f, float* disp_f, mi_occ_stats* stats, void* stream) {
    return render(net, packed_c, packed_f, cfg, grid, bits_c, bits_f, rays, n_rays, t_rand, u, ws, ws_bytes, rgb_c, disp_c, rgb_f, disp_f, stats,
                  (hipStream_t)stream);
}

}  // extern "C"
