// vox.hip -- libmi_nerf_vox.so (include/mi_nerf_vox.h): a radiance grid (density plus spherical-harmonic colour per lattice point), the
// projection of a network's answers onto it, its empty-space plane, and the renderer that marches rays through it with no network.  A
// library of its own: it shares abi_error.h with the others, and vox_rule.h (the rule's building blocks in device code, the grid and march
// checks) with voxgrad.hip, at compile time and nothing at link time.
//
//   project_kernel<B>      one thread per lattice point of the index list: fmaxf of the density, 3 B dot products of proj rows with the
//                          sigmoid of the D colours (increasing j), one record written with 16-byte stores, padding as zero.
//   skip_kernel            one wave per block of 8^3 cells: the lanes sweep the points of the block extended by one cell, a ballot decides
//                          the byte, lane 0 stores it.
//   render_kernel<B, ST>   a GROUP OF 8 LANES PER RAY, 32 rays per workgroup.  Every lane of a group carries the same ray state (origin,
//                          interval counter, transmittance, sums): all control flow is uniform within a group, so the eight lanes are
//                          always active together.  Lane e owns corner e of the sample's cell: it reads that corner's sigma (4 bytes; the
//                          eight lanes read 4 pairs of neighbours), and only when the group's sigma_s > 0 its record with 16-byte loads --
//                          one aligned 16 / 64 / 128-byte piece per lane, neighbouring corners in x adjacent -- evaluates the basis on it
//                          and scales by its trilinear weight.  The group adds with DPP row operations (x neighbours, y neighbours, the
//                          other half-row): no LDS, no bpermute.  A wave instruction whose 64 lanes read 64 unrelated rows runs ~17x below
//                          the rate of contiguous segments; here a wave's 64 lanes are 8 rays of neighbouring pixels in neighbouring cells.
//                          The skip byte and the sigma plane are read before any coefficient: in a baked scene most samples end there.
//                          ST names the storage: DENSE (mi_vox_render), SPARSE32 and SPARSE16 (mi_vox_render_sparse).  A sparse lane reads
//                          its corner's slot once sigma_s > 0, then one record of the table: dwordx4 loads for fp32, one 8-byte load (B = 1) or
//                          16-byte loads (B = 4, 9) for binary16, widened with v_cvt_f32_f16.  Active x neighbours have consecutive slots,
//                          so the records of a pair of lanes are still adjacent.
//   index_*_kernel         mi_vox_index: the active flag of 1024 points per workgroup into the slot plane and their count (ballots, wave
//                          sums through LDS) | one block scans the counts (block_scan.h) | flags become record numbers.  Deterministic: no atomic.
//   pack_kernel<F16>       one thread per 16-byte piece of an fp32 record: copied, or converted to four binary16 values, to table[slot].
//   resample_kernel<B>     THE RESAMPLING RULE, a gather: one thread per 16-byte piece of a destination record (1 / 4 / 8 threads per
//                          point, x fastest), so a wave stores 1 KiB of consecutive bytes.  A thread finds its point's source cell with
//                          vox_rule.h's cell_of (the renderer's), loads the same piece of the eight source records with 16-byte loads
//                          (12-byte ones for B = 1, whose fourth float is always padding) -- the lanes of one point read eight whole
//                          records between them -- and sums in the rule's order; piece 0's thread also interpolates sigma.  A piece
//                          that is all padding is stored as zeros without a load; a padding float beside counted ones is masked
//                          to zero after the sum, so that its load stays part of the 16 bytes.
//   prune_kernel<B>        THE PRUNING RULE, the same thread shape: a point's R4 lanes split the 27 sigma reads of the stencil between
//                          them and a ballot joins the answers; piece 0's thread writes sigma_out, and the record of a point that is
//                          not kept is zeroed piece by piece.  A kept record is not touched.
//   shadow_kernel          THE SHADOW RULE: the renderer's group of 8 lanes per pixel ray, 32 rays per workgroup -- sigma only, never a
//                          record.  tvol is ray-major [H, W, K] with K a multiple of 8 so that lane k & 7 holds od_k and a group stores
//                          eight consecutive floats as one aligned 32-byte piece every eight slices.  Unlike the renderer, lane e takes
//                          a SLICE, not a corner: it evaluates slice 8 c + e of chunk c whole (eight sigma loads, the rule's pairwise
//                          sum), and the running sum goes from lane to lane in the rule's order by seven DPP shifts.  With a lane per
//                          corner every lane repeated the cell arithmetic of every slice, and that arithmetic bounded the kernel.  A chunk of eight slices that lies wholly before the ray's entry into the box or
//                          behind its exit (the slab, widened by the fp32 error of a sample position) is stored without a sample.
//   seen_kernel            THE VISIBILITY RULE: one thread per lattice point, x fastest: it projects itself into the view, loads one
//                          float of tvol and folds it into its own element of the od plane (a coalesced read-modify-write).  No LDS.
//   prune_seen_kernel<B>   THE SEEN PRUNING RULE: prune_kernel with the seed's second condition, a kernel of its own so that
//                          prune_kernel's code stays what it was.
//   ray_grad_kernel<B, ST> THE RAY GRADIENT RULE: the renderer's group of 8 lanes per ray and its three storages.  March 1 is the renderer's loop
//                          operation by operation (the check outputs are its bits) plus S = sum w_k s_k.  March 2 walks the same samples with
//                          the prefix P and jumps over empty blocks as march 1 does (a sample without density adds exact zeros): per sample
//                          lane e forms h_e from its corner's sigma and colour, three more group sums give dL/dp, and the sums to o, d, t0,
//                          dt, t1, L and lane e's share of dL/dY_b stay in registers.  At the ray's end the shares are group-summed, the
//                          basis, dt, L and the slab's entry and exit are differentiated, and lane 0 stores six floats.  A struct of its own
//                          (RayGradArgs), so that RenderArgs and the renderer's code stay what they were.
//   skip_signed_kernel,    A SIGNED GRID: skip_kernel with the test sigma > 0, and render_kernel's march with sigma_s = fmaxf(the group's sum, 0) --
//   render_signed_kernel<B, ST>  one v_max_f32 per sample more, the same nine instantiations.  Kernels of their own, spelled out again,
//                          so that skip_kernel and render_kernel keep their names and their code (docs/design/29_signed_density.md).
//
// No atomic, no host synchronisation, no copy, no allocation.  Compiled with -ffp-contract=off: the rule is evaluated as it is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/mi_nerf_vox.h"
#include "abi_error.h"
#include "block_scan.h"
#define VOX_RULE_NAMESPACE mivox
#include "vox_rule.h"

namespace mivox {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_VOX_EHIP)
#define VOX_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mivox, MI_VOX_EINVAL, cond, __VA_ARGS__)
#define VOX_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mivox, name)

static_assert(BLK == MI_VOX_BLOCK, "vox_rule.h and mi_nerf_vox.h disagree on the block edge");

// ------------------------------------------------------------------------------------------------
// mi_vox_project
// ------------------------------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(THREADS) void project_kernel(const float4* __restrict__ raw, const float* __restrict__ proj,
                                                          const long long* __restrict__ index, long long M, int D, long long N,
                                                          float* __restrict__ sigma, float4* __restrict__ coef) {
    constexpr int R4 = record_floats(B) / 4;
    const long long m = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    const long long at = index[m];
    if (at < 0 || at >= N) return;
    float acc[R4 * 4];
#pragma unroll
    for (int i = 0; i < R4 * 4; ++i) acc[i] = 0.0f;
    const float4* row = raw + m * D;
    float dens = 0.0f;
    for (int j = 0; j < D; ++j) {
        const float4 v = row[j];
        if (j == 0) dens = v.w;
        const float s0 = 1.0f / (1.0f + expf(-v.x)), s1 = 1.0f / (1.0f + expf(-v.y)), s2 = 1.0f / (1.0f + expf(-v.z));
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const float p = proj[b * D + j];
            if (j == 0) {
                acc[3 * b + 0] = p * s0; acc[3 * b + 1] = p * s1; acc[3 * b + 2] = p * s2;
            } else {
                acc[3 * b + 0] += p * s0; acc[3 * b + 1] += p * s1; acc[3 * b + 2] += p * s2;
            }
        }
    }
    if (sigma) sigma[at] = fmaxf(dens, 0.0f);                          // fmaxf returns the other operand for a NaN
    float4* rec = coef + at * R4;
#pragma unroll
    for (int q = 0; q < R4; ++q) rec[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
}

// ------------------------------------------------------------------------------------------------
// mi_vox_build_skip
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void skip_kernel(const Lattice g, const float* __restrict__ sigma, uint8_t* __restrict__ skip) {
    const int blk = blockIdx.x;
    const int bx = blk % g.nb[0], by = (blk / g.nb[0]) % g.nb[1], bz = blk / (g.nb[0] * g.nb[1]);
    const int b[3] = {bx, by, bz};
    int p0[3], np[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c1 = min(BLK * b[i] + BLK, g.res[i]);
        p0[i] = max(BLK * b[i] - 1, 0);
        np[i] = min(c1 + 1, g.res[i]) - p0[i] + 1;
    }
    const int total = np[0] * np[1] * np[2];
    bool any = false;
    for (int t = threadIdx.x; t < total; t += 64) {
        const int x = p0[0] + t % np[0], y = p0[1] + (t / np[0]) % np[1], z = p0[2] + t / (np[0] * np[1]);
        any |= sigma[((long long)z * g.P[1] + y) * g.P[0] + x] != 0.0f;
    }
    const bool found = __ballot(any) != 0ull;
    if (threadIdx.x == 0) skip[blk] = found ? 1 : 0;
}

// skip_kernel with the signed plane's test: the byte is 0 iff sigma <= 0 at every point of the block extended by one cell
__global__ __launch_bounds__(64) void skip_signed_kernel(const Lattice g, const float* __restrict__ sigma, uint8_t* __restrict__ skip) {
    const int blk = blockIdx.x;
    const int bx = blk % g.nb[0], by = (blk / g.nb[0]) % g.nb[1], bz = blk / (g.nb[0] * g.nb[1]);
    const int b[3] = {bx, by, bz};
    int p0[3], np[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c1 = min(BLK * b[i] + BLK, g.res[i]);
        p0[i] = max(BLK * b[i] - 1, 0);
        np[i] = min(c1 + 1, g.res[i]) - p0[i] + 1;
    }
    const int total = np[0] * np[1] * np[2];
    bool any = false;
    for (int t = threadIdx.x; t < total; t += 64) {
        const int x = p0[0] + t % np[0], y = p0[1] + (t / np[0]) % np[1], z = p0[2] + t / (np[0] * np[1]);
        any |= sigma[((long long)z * g.P[1] + y) * g.P[0] + x] > 0.0f;
    }
    const bool found = __ballot(any) != 0ull;
    if (threadIdx.x == 0) skip[blk] = found ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// mi_vox_index: flag + count | exclusive scan of the counts | emit
// ------------------------------------------------------------------------------------------------
constexpr int IDX_ROWS = 4;                              // a workgroup owns IDX_ROWS rows of THREADS consecutive points
constexpr int IDX_CHUNK = THREADS * IDX_ROWS;
constexpr int WAVES = THREADS / 64;

// the active flag of every point goes into the slot plane (1 / 0), the chunk's count into counts[blockIdx.x]
__global__ __launch_bounds__(THREADS) void index_flag_kernel(const Lattice g, const float* __restrict__ sigma, int* __restrict__ slot,
                                                             unsigned* __restrict__ counts, long long N) {
    __shared__ unsigned lds[WAVES];
    const long long base = (long long)blockIdx.x * IDX_CHUNK;
    unsigned cnt = 0;                                                      // of this wave, the same in every lane
    for (int r = 0; r < IDX_ROWS; ++r) {
        const long long i = base + r * THREADS + threadIdx.x;
        bool act = false;
        if (i < N) {
            const int x = (int)(i % g.P[0]), y = (int)((i / g.P[0]) % g.P[1]), z = (int)(i / ((long long)g.P[0] * g.P[1]));
            for (int z1 = max(z - 1, 0); z1 <= min(z + 1, g.P[2] - 1); ++z1)
                for (int y1 = max(y - 1, 0); y1 <= min(y + 1, g.P[1] - 1); ++y1)
                    for (int x1 = max(x - 1, 0); x1 <= min(x + 1, g.P[0] - 1); ++x1)
                        act |= sigma[((long long)z1 * g.P[1] + y1) * g.P[0] + x1] > 0.0f;
            slot[i] = act ? 1 : 0;
        }
        cnt += (unsigned)__popcll(__ballot(act));
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// one block: the chunk counts -> their exclusive prefix sums in place; *total = M
__global__ __launch_bounds__(1024) void index_scan_kernel(unsigned* __restrict__ counts, int nb, long long* __restrict__ total) {
    const unsigned carry = miblock::scan_sums(counts, nb);
    if (threadIdx.x == 0) *total = (long long)carry;
}

// flags -> slots: the chunk's first record number from the scan, ranks within a row from a ballot, rows in order
__global__ __launch_bounds__(THREADS) void index_emit_kernel(int* __restrict__ slot, const unsigned* __restrict__ counts, long long N) {
    __shared__ unsigned lds[WAVES];
    const long long base = (long long)blockIdx.x * IDX_CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned run = counts[blockIdx.x];
    for (int r = 0; r < IDX_ROWS; ++r) {
        const long long i = base + r * THREADS + threadIdx.x;
        const bool act = i < N && slot[i] != 0;
        const unsigned long long m = __ballot(act);
        if (lane == 0) lds[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = 0, row = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const unsigned s = lds[w];
            if (w < wave) before += s;
            row += s;
        }
        if (i < N) slot[i] = act ? (int)(run + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull))) : -1;
        run += row;
        __syncthreads();                                                   // lds is rewritten by the next row
    }
}

// ------------------------------------------------------------------------------------------------
// mi_vox_pack: one thread per 16-byte piece of an fp32 record
// ------------------------------------------------------------------------------------------------
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

template <bool F16>
__global__ __launch_bounds__(THREADS) void pack_kernel(const float4* __restrict__ src, const int* __restrict__ slot, long long records, long long M,
                                                       int R4, void* __restrict__ table) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long rec = t / R4;
    const int q = (int)(t % R4);
    if (rec >= records) return;
    long long to = rec;
    if (slot) {
        to = slot[rec];
        if (to < 0 || to >= M) return;
    }
    const float4 v = src[rec * R4 + q];
    if constexpr (F16) {
        // the conversion rounds to nearest even and gives +-inf beyond the binary16 range
        const half4_t h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        reinterpret_cast<uint2*>(table)[to * R4 + q] = __builtin_bit_cast(uint2, h);
    } else {
        reinterpret_cast<float4*>(table)[to * R4 + q] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// mi_vox_resample, mi_vox_prune: one thread per 16-byte piece of a destination record, x fastest
// ------------------------------------------------------------------------------------------------
struct ResampleArgs {
    Lattice s, d;                                        // source, destination
    float step_d[3];                                     // (hi_d - lo_d) / (float)res_d, formed on the host in fp32
    const float* sigma_s;
    const float4* coef_s;
    float* sigma_d;
    float4* coef_d;
    long long pieces;                                    // destination points x R4
};

// the header's pairwise sum of eight weighted corners
__device__ __forceinline__ float interp8(const float (&w)[8], const float (&q)[8]) {
    return ((w[0] * q[0] + w[1] * q[1]) + (w[2] * q[2] + w[3] * q[3])) + ((w[4] * q[4] + w[5] * q[5]) + (w[6] * q[6] + w[7] * q[7]));
}

template <int B>
__global__ __launch_bounds__(THREADS) void resample_kernel(const ResampleArgs a) {
    constexpr int R4 = record_floats(B) / 4;               // pieces of a record
    constexpr int V4 = (3 * B + 3) / 4;                    // the pieces that hold coefficients
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= a.pieces) return;
    const unsigned j = (unsigned)(t / R4);                 // at most 513^3 points: 32-bit divisions below
    const int q = (int)(t % R4);
    float4* out = a.coef_d + t;                            // = coef_d[j * R4 + q]
    if (q >= V4) {                                         // all padding: no load
        *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const Lattice& s = a.s;
    const unsigned row = j / (unsigned)a.d.P[0];
    const int jd[3] = {(int)(j - row * (unsigned)a.d.P[0]), (int)(row % (unsigned)a.d.P[1]), (int)(row / (unsigned)a.d.P[1])};
    int c[3];
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float x = a.d.lo[i] + (float)jd[i] * a.step_d[i];
        cell_of((x - s.lo[i]) * s.inv[i], s.res[i], c[i], f[i]);
    }
    float w[8];
    long long at[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        const float wx = ex ? f[0] : 1.0f - f[0], wy = ey ? f[1] : 1.0f - f[1], wz = ez ? f[2] : 1.0f - f[2];
        w[e] = (wx * wy) * wz;
        at[e] = ((long long)(c[2] + ez) * s.P[1] + (c[1] + ey)) * s.P[0] + (c[0] + ex);
    }
    float4 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = a.coef_s[at[e] * R4 + q];
    float qx[8], qy[8], qz[8], qw[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { qx[e] = v[e].x; qy[e] = v[e].y; qz[e] = v[e].z; qw[e] = v[e].w; }
    float4 r;
    r.x = interp8(w, qx);
    r.y = interp8(w, qy);                                  // 3 B is a multiple of 3: the first three floats of a piece that holds any are counted
    r.z = interp8(w, qz);
    // the fourth may be padding (B = 1: always; B = 9: piece 6), written as zero whatever the source holds there.  The bits are masked
    // and not selected: a select lets the compiler split the 16-byte load into 12 bytes and a 4-byte load under a branch
    static_assert((3 * B) % 4 == 3 || (3 * B) % 4 == 0, "a piece holds 3 or 4 counted floats");
    const int keep = 4 * q + 3 < 3 * B ? -1 : 0;
    r.w = __int_as_float(__float_as_int(interp8(w, qw)) & keep);
    *out = r;
    if (q == 0) {
        float qs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qs[e] = a.sigma_s[at[e]];
        a.sigma_d[j] = interp8(w, qs);
    }
}

// kept: the point or one of its 26 neighbours (clipped) has sigma > tau.  The R4 lanes of a point share the 27 reads (lane q takes
// neighbours q, q + R4, ...) and a ballot joins them: R4 divides 64, so a point's lanes sit in one wave.
template <int B>
__global__ __launch_bounds__(THREADS) void prune_kernel(const Lattice g, float tau, const float* __restrict__ sigma_in, float* __restrict__ sigma_out,
                                                        float4* __restrict__ coef, long long pieces) {
    constexpr int R4 = record_floats(B) / 4;
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = t < pieces;                          // no lane leaves before the ballot
    const unsigned j = (unsigned)(t / R4);                 // used only when live: at most 513^3 points, 32-bit divisions below
    const int q = (int)(t % R4);
    bool hit = false;
    if (live) {
        const unsigned row = j / (unsigned)g.P[0];
        const int x = (int)(j - row * (unsigned)g.P[0]), y = (int)(row % (unsigned)g.P[1]), z = (int)(row / (unsigned)g.P[1]);
        for (int n = q; n < 27; n += R4) {
            const int x1 = x + n % 3 - 1, y1 = y + (n / 3) % 3 - 1, z1 = z + n / 9 - 1;
            if (x1 >= 0 && x1 < g.P[0] && y1 >= 0 && y1 < g.P[1] && z1 >= 0 && z1 < g.P[2])
                hit |= sigma_in[((long long)z1 * g.P[1] + y1) * g.P[0] + x1] > tau;
        }
    }
    const unsigned long long m = __ballot(hit);
    const int first = (threadIdx.x & 63) & ~(R4 - 1);      // the wave lane of this point's piece 0
    const bool kept = ((m >> first) & ((1ull << R4) - 1ull)) != 0ull;
    if (!live) return;
    if (q == 0) sigma_out[j] = kept ? sigma_in[j] : 0.0f;
    if (!kept) coef[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// a lane's value handed to the next lane of its row of 16 (row_shr:1); lane 0 of a row receives 0
__device__ __forceinline__ float dpp_row_shr1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true)); }

// THE SEEN PRUNING RULE: the same kernel with the seed's second condition (od <= od_max; a NaN fails).  od is loaded only where
// sigma_in > tau.
template <int B>
__global__ __launch_bounds__(THREADS) void prune_seen_kernel(const Lattice g, float tau, float od_max, const float* __restrict__ sigma_in,
                                                             const float* __restrict__ od, float* __restrict__ sigma_out, float4* __restrict__ coef,
                                                             long long pieces) {
    constexpr int R4 = record_floats(B) / 4;
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = t < pieces;                          // no lane leaves before the ballot
    const unsigned j = (unsigned)(t / R4);
    const int q = (int)(t % R4);
    bool hit = false;
    if (live) {
        const unsigned row = j / (unsigned)g.P[0];
        const int x = (int)(j - row * (unsigned)g.P[0]), y = (int)(row % (unsigned)g.P[1]), z = (int)(row / (unsigned)g.P[1]);
        for (int n = q; n < 27; n += R4) {
            const int x1 = x + n % 3 - 1, y1 = y + (n / 3) % 3 - 1, z1 = z + n / 9 - 1;
            if (x1 >= 0 && x1 < g.P[0] && y1 >= 0 && y1 < g.P[1] && z1 >= 0 && z1 < g.P[2]) {
                const long long at = ((long long)z1 * g.P[1] + y1) * g.P[0] + x1;
                if (sigma_in[at] > tau) hit |= od[at] <= od_max;
            }
        }
    }
    const unsigned long long m = __ballot(hit);
    const int first = (threadIdx.x & 63) & ~(R4 - 1);      // the wave lane of this point's piece 0
    const bool kept = ((m >> first) & ((1ull << R4) - 1ull)) != 0ull;
    if (!live) return;
    if (q == 0) sigma_out[j] = kept ? sigma_in[j] : 0.0f;
    if (!kept) coef[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ------------------------------------------------------------------------------------------------
// mi_vox_shadow, mi_vox_seen: one view
// ------------------------------------------------------------------------------------------------
struct ViewArgs {
    int H, W, K;
    float fx, fy, cx, cy;
    float R[9], t[3];                                    // c2w = (R | t): R[3 r + c]
    float depth_near, depth_step;
};

struct ShadowArgs {
    Lattice g;
    ViewArgs v;
    const float* sigma;
    const uint8_t* skip;                                 // NULL: no plane
    float* tvol;
};

__global__ __launch_bounds__(THREADS) void shadow_kernel(const ShadowArgs a) {
    const int e = threadIdx.x & (GROUP - 1);               // the slice of a chunk that this lane evaluates and whose od it stores
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 3);
    const ViewArgs& v = a.v;
    if (ray >= (long long)v.H * v.W) return;               // a whole group leaves together
    const Lattice& g = a.g;
    const int pj = (int)(ray / v.W), pi = (int)(ray - (long long)pj * v.W);
    const float ca = ((float)pi - v.cx) / v.fx, cb = -(((float)pj - v.cy) / v.fy);
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (v.R[3 * r] * ca + v.R[3 * r + 1] * cb) + v.R[3 * r + 2] * -1.0f;
    const float* o = v.t;
    const float L = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float delta = v.depth_step * L;
    // The ray's slab of the box in the parameter m, widened by more than the fp32 error of a sample position o + m d and of the slab's own
    // quotients: a sample with m outside (m_in, m_out) fails the rule's test lo <= p <= hi, so a chunk of eight slices on one side of it
    // needs no sample.  The samples that are evaluated make the rule's test themselves: the slab decides nothing but which are skipped.
    const float m_last = v.depth_near + ((float)(v.K - 1) + 0.5f) * v.depth_step;
    float m_in = -INFINITY, m_out = INFINITY;
    bool never = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (d[i] != 0.0f) {
            const float ta = (g.lo[i] - o[i]) / d[i], tb = (g.hi[i] - o[i]) / d[i];
            const float pad = 8.0f * EPS32 * ((fabsf(ta) + fabsf(tb)) + ((fabsf(o[i]) + fabsf(g.lo[i]) + fabsf(g.hi[i])) / fabsf(d[i]) + m_last));
            m_in = fmaxf(m_in, fminf(ta, tb) - pad);       // fmaxf / fminf drop a NaN: such an axis bounds nothing
            m_out = fminf(m_out, fmaxf(ta, tb) + pad);
        } else if (!(g.lo[i] <= o[i] && o[i] <= g.hi[i])) {
            never = true;                                  // p_i = o_i at every sample
        }
    }
    float* out = a.tvol + ray * v.K + e;
    float od = 0.0f;                                       // od before the chunk's first slice: the same in the group's eight lanes
    for (int kb = 0; kb < v.K; kb += GROUP) {
        float mine = od;                                   // od_(kb + e); of a chunk without a sample it is od itself
        const float m_first = v.depth_near + ((float)kb + 0.5f) * v.depth_step;
        const float m_end = v.depth_near + ((float)(kb + GROUP - 1) + 0.5f) * v.depth_step;
        if (!never && !(m_end < m_in) && !(m_first > m_out)) {                             // uniform in a group
            // lane e evaluates slice kb + e, all eight corners of its cell: x = sigma_s * delta, 0 where the rule fetches nothing
            const float mk = v.depth_near + ((float)(kb + e) + 0.5f) * v.depth_step;
            float p[3];
            bool inside = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[i] = o[i] + mk * d[i];
                inside = inside && g.lo[i] <= p[i] && p[i] <= g.hi[i];
            }
            float x = 0.0f;
            if (inside) {
                int c[3];
                float f[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) cell_of((p[i] - g.lo[i]) * g.inv[i], g.res[i], c[i], f[i]);
                if (a.skip == nullptr || a.skip[((c[2] >> 3) * g.nb[1] + (c[1] >> 3)) * g.nb[0] + (c[0] >> 3)] != 0) {
                    float w[8], q[8];
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        const int nx = n & 1, ny = (n >> 1) & 1, nz = n >> 2;
                        const float wx = nx ? f[0] : 1.0f - f[0], wy = ny ? f[1] : 1.0f - f[1], wz = nz ? f[2] : 1.0f - f[2];
                        w[n] = (wx * wy) * wz;
                        q[n] = a.sigma[((long long)(c[2] + nz) * g.P[1] + (c[1] + ny)) * g.P[0] + (c[0] + nx)];
                    }
                    x = interp8(w, q) * delta;
                }
            }
            // od_(k+1) = od_k + x_k in the rule's order: a chain handed from lane s to lane s + 1 (row_shr:1; lane 0 of a group starts
            // from od and never takes what the neighbouring group's lane 7 hands over).  All eight lanes are active together.
#pragma unroll
            for (int s2 = 0; s2 < GROUP - 1; ++s2) {
                const float handed = dpp_row_shr1(mine + x);
                if (e == s2 + 1) mine = handed;
            }
            od = group_sum(e == GROUP - 1 ? mine + x : 0.0f);                              // lane 7's sum plus seven zeros: exact
        }
        out[kb] = mine;                                    // the group's eight lanes: 32 consecutive, aligned bytes
    }
}

struct SeenArgs {
    Lattice g;
    ViewArgs v;
    float step[3];                                       // (hi - lo) / (float)res, formed on the host in fp32
    const float* tvol;
    float* od;
    int bias;
    long long N;
};

__global__ __launch_bounds__(THREADS) void seen_kernel(const SeenArgs a) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= a.N) return;
    const Lattice& g = a.g;
    const ViewArgs& v = a.v;
    const unsigned j = (unsigned)t;                        // at most 513^3 points: 32-bit divisions below
    const unsigned row = j / (unsigned)g.P[0];
    const int jd[3] = {(int)(j - row * (unsigned)g.P[0]), (int)(row % (unsigned)g.P[1]), (int)(row / (unsigned)g.P[1])};
    float ek[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ek[i] = (g.lo[i] + (float)jd[i] * a.step[i]) - v.t[i];
    float q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = (v.R[i] * ek[0] + v.R[3 + i] * ek[1]) + v.R[6 + i] * ek[2];
    const float z = -q[2];
    const float sx = v.cx + (v.fx * q[0]) / z, sy = v.cy - (v.fy * q[1]) / z;
    const float fi = rintf(sx), fj = rintf(sy);
    if (!(z > 0.0f && isfinite(z) && fi >= 0.0f && fi <= (float)(v.W - 1) && fj >= 0.0f && fj <= (float)(v.H - 1))) return;
    const float kf = fminf(fmaxf(floorf((z - v.depth_near) / v.depth_step), -1099511627776.0f), 1099511627776.0f);      // +-2^40
    const long long k = (long long)kf - a.bias;
    if (k >= v.K) return;
    float od = 0.0f;
    if (k >= 0) od = a.tvol[((long long)(int)fj * v.W + (int)fi) * v.K + k];
    a.od[t] = fminf(a.od[t], od);
}

// ------------------------------------------------------------------------------------------------
// mi_vox_render, mi_vox_render_sparse
// ------------------------------------------------------------------------------------------------
struct RenderArgs {
    Lattice g;
    const float* sigma;
    const float4* coef;                                  // the dense coef array, or the table of a compact grid (either format)
    const int* slot;                                     // compact grids only
    long long M;
    const uint8_t* skip;
    const float* rays;
    long long n;
    float step, t_near, t_far, T_min;
    float bg[3];
    int use_skip;
    int max_steps;
    float *rgb, *disp, *acc, *depth;
    unsigned* visited;
};

template <int B, int ST>
__global__ __launch_bounds__(THREADS) void render_kernel(const RenderArgs a) {
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
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    unsigned seen = 0;
    if (!miss) {
        const float dt = a.step / L;
        const float ux = d[0] / L, uy = d[1] / L, uz = d[2] / L;
        float Y[B];
        sh_basis<B>(ux, uy, uz, Y);
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
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        float T = 1.0f;
        int k = 0;
        while (k < a.max_steps) {
            const float ak = t0 + (float)k * dt;
            if (!(ak < t1)) break;
            const float bk = fminf(t0 + (float)(k + 1) * dt, t1);
            const float mk = 0.5f * (ak + bk);
            int c[3];
            float f[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float p = o[i] + mk * d[i];
                cell_of((p - g.lo[i]) * g.inv[i], g.res[i], c[i], f[i]);
            }
            if (a.use_skip) {
                const int bx = c[0] >> 3, by = c[1] >> 3, bz = c[2] >> 3;
                if (a.skip[(bz * g.nb[1] + by) * g.nb[0] + bx] == 0) {
                    int next = k + 1;
                    if (can_jump) {
                        // where the ray leaves the block extended by half a cell, in lattice units; the first sample that is evaluated
                        // again starts a whole interval before that
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
            // lane e: corner e
            const long long at = ((long long)(c[2] + ez) * g.P[1] + (c[1] + ey)) * g.P[0] + (c[0] + ex);
            const float wx = ex ? f[0] : 1.0f - f[0], wy = ey ? f[1] : 1.0f - f[1], wz = ez ? f[2] : 1.0f - f[2];
            const float w = (wx * wy) * wz;
            const float sigma_s = group_sum(w * a.sigma[at]);
            ++seen;
            const float delta = (bk - ak) * L;
            const float alpha = 1.0f - expf(-(sigma_s * delta));
            const float wt = T * alpha;
            if (sigma_s > 0.0f) {
                float kc[record_regs<B, ST>()];
                fetch_record<B, ST>(a.coef, a.slot, a.M, at, kc);
                float col[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float q = kc[ch] * Y[0];
#pragma unroll
                    for (int b = 1; b < B; ++b) q += kc[3 * b + ch] * Y[b];
                    col[ch] = fminf(fmaxf(group_sum(w * q), 0.0f), 1.0f);
                }
                sr += wt * col[0]; sg += wt * col[1]; sb += wt * col[2];
            }
            sw += wt;
            sd += wt * mk;
            T = T * (1.0f - alpha);
            ++k;
            if (T < a.T_min) break;
        }
    }
    if (e == 0) {
        const float rest = 1.0f - sw;
        a.rgb[ray * 3 + 0] = sr + rest * a.bg[0];
        a.rgb[ray * 3 + 1] = sg + rest * a.bg[1];
        a.rgb[ray * 3 + 2] = sb + rest * a.bg[2];
        if (a.disp) {
            const float q = sd / sw;
            const float m = (q != q) ? q : fmaxf(1e-10f, q);
            float disp = 1.0f / m;
            if (disp != disp) disp = 0.0f;
            if (disp > 5.0f) disp = 5.0f;
            a.disp[ray] = disp;
        }
        if (a.acc) a.acc[ray] = sw;
        if (a.depth) a.depth[ray] = sd;
        if (a.visited) a.visited[ray] = seen;
    }
}

// ------------------------------------------------------------------------------------------------
// mi_vox_render_signed, mi_vox_render_sparse_signed: A SIGNED GRID of the header (its skip builder stands beside skip_kernel)
// ------------------------------------------------------------------------------------------------
// render_kernel's march spelled again with step 3's sigma_s = fmaxf(interpolation, 0).  A kernel of its own and not a template flag on
// render_kernel: that kernel's names and code stay what they were (vox_rule.h on why the march is not shared through a function).
// On a plane that is >= 0 the fmaxf returns its argument, so every output equals render_kernel's bit for bit.  A sample in a block whose
// signed byte is 0 has eight corners <= 0 and weights >= 0: the interpolation is <= 0, sigma_s = 0, and it adds exactly nothing.
template <int B, int ST>
__global__ __launch_bounds__(THREADS) void render_signed_kernel(const RenderArgs a) {
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
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    unsigned seen = 0;
    if (!miss) {
        const float dt = a.step / L;
        const float ux = d[0] / L, uy = d[1] / L, uz = d[2] / L;
        float Y[B];
        sh_basis<B>(ux, uy, uz, Y);
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
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        float T = 1.0f;
        int k = 0;
        while (k < a.max_steps) {
            const float ak = t0 + (float)k * dt;
            if (!(ak < t1)) break;
            const float bk = fminf(t0 + (float)(k + 1) * dt, t1);
            const float mk = 0.5f * (ak + bk);
            int c[3];
            float f[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float p = o[i] + mk * d[i];
                cell_of((p - g.lo[i]) * g.inv[i], g.res[i], c[i], f[i]);
            }
            if (a.use_skip) {
                const int bx = c[0] >> 3, by = c[1] >> 3, bz = c[2] >> 3;
                if (a.skip[(bz * g.nb[1] + by) * g.nb[0] + bx] == 0) {
                    int next = k + 1;
                    if (can_jump) {
                        // where the ray leaves the block extended by half a cell, in lattice units; the first sample that is evaluated
                        // again starts a whole interval before that
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
            // lane e: corner e
            const long long at = ((long long)(c[2] + ez) * g.P[1] + (c[1] + ey)) * g.P[0] + (c[0] + ex);
            const float wx = ex ? f[0] : 1.0f - f[0], wy = ey ? f[1] : 1.0f - f[1], wz = ez ? f[2] : 1.0f - f[2];
            const float w = (wx * wy) * wz;
            const float sigma_s = fmaxf(group_sum(w * a.sigma[at]), 0.0f);   // the ReLU AFTER the interpolation: the one change
            ++seen;
            const float delta = (bk - ak) * L;
            const float alpha = 1.0f - expf(-(sigma_s * delta));
            const float wt = T * alpha;
            if (sigma_s > 0.0f) {
                float kc[record_regs<B, ST>()];
                fetch_record<B, ST>(a.coef, a.slot, a.M, at, kc);
                float col[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float q = kc[ch] * Y[0];
#pragma unroll
                    for (int b = 1; b < B; ++b) q += kc[3 * b + ch] * Y[b];
                    col[ch] = fminf(fmaxf(group_sum(w * q), 0.0f), 1.0f);
                }
                sr += wt * col[0]; sg += wt * col[1]; sb += wt * col[2];
            }
            sw += wt;
            sd += wt * mk;
            T = T * (1.0f - alpha);
            ++k;
            if (T < a.T_min) break;
        }
    }
    if (e == 0) {
        const float rest = 1.0f - sw;
        a.rgb[ray * 3 + 0] = sr + rest * a.bg[0];
        a.rgb[ray * 3 + 1] = sg + rest * a.bg[1];
        a.rgb[ray * 3 + 2] = sb + rest * a.bg[2];
        if (a.disp) {
            const float q = sd / sw;
            const float m = (q != q) ? q : fmaxf(1e-10f, q);
            float disp = 1.0f / m;
            if (disp != disp) disp = 0.0f;
            if (disp > 5.0f) disp = 5.0f;
            a.disp[ray] = disp;
        }
        if (a.acc) a.acc[ray] = sw;
        if (a.depth) a.depth[ray] = sd;
        if (a.visited) a.visited[ray] = seen;
    }
}

// ------------------------------------------------------------------------------------------------
// mi_vox_render_backward_rays, mi_vox_render_sparse_backward_rays
// ------------------------------------------------------------------------------------------------
struct RayGradArgs {
    Lattice g;
    const float* sigma;
    const float4* coef;                                  // the dense coef array, or the table of a compact grid (either format)
    const int* slot;                                     // compact grids only
    long long M;
    const uint8_t* skip;
    const float* rays;
    long long n;
    float step, t_near, t_far, T_min;
    float bg[3];
    int use_skip;
    int max_steps;
    const float *g_rgb, *g_acc, *g_depth;
    float* d_rays;
    float *rgb, *acc, *depth;                            // the check outputs
};

template <int B, int ST>
__global__ __launch_bounds__(THREADS) void ray_grad_kernel(const RayGradArgs a) {
    const int e = threadIdx.x & (GROUP - 1);               // this lane's corner
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 3);
    if (ray >= a.n) return;                                // a whole group leaves together
    const Lattice& g = a.g;
    const float* rp = a.rays + ray * 6;
    const float o[3] = {rp[0], rp[1], rp[2]}, d[3] = {rp[3], rp[4], rp[5]};
    const float L = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    bool miss = !(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(L)) || L == 0.0f;
    float entry = -INFINITY, exit_ = INFINITY;
    int ie = -1, ix = -1;                                  // the axes that give entry and exit
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (d[i] != 0.0f) {
            const float ta = (g.lo[i] - o[i]) / d[i], tb = (g.hi[i] - o[i]) / d[i];
            const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
            if (tn > entry) ie = i;
            if (tf < exit_) ix = i;
            entry = fmaxf(entry, tn);
            exit_ = fminf(exit_, tf);
        } else if (!(g.lo[i] <= o[i] && o[i] <= g.hi[i])) {
            miss = true;
        }
    }
    const float t0 = fmaxf(a.t_near, entry), t1 = fminf(a.t_far, exit_);
    if (!(t1 > t0)) miss = true;
    if (!(entry > a.t_near)) ie = -1;                      // t0 = t_near: fixed
    if (!(exit_ < a.t_far)) ix = -1;                       // t1 = t_far: fixed
    // upstream
    const float G[3] = {a.g_rgb[ray * 3 + 0], a.g_rgb[ray * 3 + 1], a.g_rgb[ray * 3 + 2]};
    const float ga = a.g_acc ? a.g_acc[ray] : 0.0f, gd = a.g_depth ? a.g_depth[ray] : 0.0f;
    const float gap = ga - ((G[0] * a.bg[0] + G[1] * a.bg[1]) + G[2] * a.bg[2]);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    float go[3] = {0.0f, 0.0f, 0.0f}, gdir[3] = {0.0f, 0.0f, 0.0f};
    if (!miss) {
        const float dt = a.step / L;
        const float ux = d[0] / L, uy = d[1] / L, uz = d[2] / L;
        float Y[B];
        sh_basis<B>(ux, uy, uz, Y);
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
        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        // ---- march 1: the renderer's loop, and S ----------------------------------------------------------
        float S = 0.0f;
        {
            float T = 1.0f;
            int k = 0;
            while (k < a.max_steps) {
                const float ak = t0 + (float)k * dt;
                if (!(ak < t1)) break;
                const float bk = fminf(t0 + (float)(k + 1) * dt, t1);
                const float mk = 0.5f * (ak + bk);
                int c[3];
                float f[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float p = o[i] + mk * d[i];
                    cell_of((p - g.lo[i]) * g.inv[i], g.res[i], c[i], f[i]);
                }
                if (a.use_skip) {
                    const int bx = c[0] >> 3, by = c[1] >> 3, bz = c[2] >> 3;
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
                const long long at = ((long long)(c[2] + ez) * g.P[1] + (c[1] + ey)) * g.P[0] + (c[0] + ex);
                const float wx = ex ? f[0] : 1.0f - f[0], wy = ey ? f[1] : 1.0f - f[1], wz = ez ? f[2] : 1.0f - f[2];
                const float w = (wx * wy) * wz;
                const float sigma_s = group_sum(w * a.sigma[at]);
                const float delta = (bk - ak) * L;
                const float alpha = 1.0f - expf(-(sigma_s * delta));
                const float wt = T * alpha;
                float col[3] = {0.0f, 0.0f, 0.0f};
                if (sigma_s > 0.0f) {
                    float kc[record_regs<B, ST>()];
                    fetch_record<B, ST>(a.coef, a.slot, a.M, at, kc);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float q = kc[ch] * Y[0];
#pragma unroll
                        for (int b = 1; b < B; ++b) q += kc[3 * b + ch] * Y[b];
                        col[ch] = fminf(fmaxf(group_sum(w * q), 0.0f), 1.0f);
                    }
                    sr += wt * col[0]; sg += wt * col[1]; sb += wt * col[2];
                }
                const float sk = (((G[0] * col[0] + G[1] * col[1]) + G[2] * col[2]) + gap) + gd * mk;
                S += wt * sk;
                sw += wt;
                sd += wt * mk;
                T = T * (1.0f - alpha);
                ++k;
                if (T < a.T_min) break;
            }
        }
        // ---- march 2: the same samples (it jumps as march 1 does), the prefix P, the sums of THE RAY GRADIENT RULE --------
        {
            float T = 1.0f, P = 0.0f;
            float gpo[3] = {0.0f, 0.0f, 0.0f}, gpd[3] = {0.0f, 0.0f, 0.0f};       // sum g_p, sum m_k g_p
            float gt0 = 0.0f, gdt = 0.0f, gt1 = 0.0f, gL = 0.0f;
            float gy[B];                                                       // this lane's share of dL/dY_b
#pragma unroll
            for (int b = 0; b < B; ++b) gy[b] = 0.0f;
            int k = 0;
            while (k < a.max_steps) {
                const float ak = t0 + (float)k * dt;
                if (!(ak < t1)) break;
                const float nk = t0 + (float)(k + 1) * dt;
                const float bk = fminf(nk, t1);
                const bool cut = t1 < nk;                                      // the truncated last interval
                const float mk = 0.5f * (ak + bk);
                int c[3];
                float f[3];
                bool moves[3];                                                 // the clamp of f_i is not active
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float p = o[i] + mk * d[i];
                    const float gi = (p - g.lo[i]) * g.inv[i];
                    cell_of(gi, g.res[i], c[i], f[i]);
                    const float r = gi - (float)c[i];
                    moves[i] = r >= 0.0f && r <= 1.0f;
                }
                if (a.use_skip) {
                    const int bx = c[0] >> 3, by = c[1] >> 3, bz = c[2] >> 3;
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
                const long long at = ((long long)(c[2] + ez) * g.P[1] + (c[1] + ey)) * g.P[0] + (c[0] + ex);
                const float wx = ex ? f[0] : 1.0f - f[0], wy = ey ? f[1] : 1.0f - f[1], wz = ez ? f[2] : 1.0f - f[2];
                const float w = (wx * wy) * wz;
                const float se = a.sigma[at];
                const float sigma_s = group_sum(w * se);
                const float delta = (bk - ak) * L;
                const float alpha = 1.0f - expf(-(sigma_s * delta));
                const float wt = T * alpha;
                float qe[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f}, Q[3] = {0.0f, 0.0f, 0.0f};
                float kc[record_regs<B, ST>()];
#pragma unroll
                for (int i = 0; i < record_regs<B, ST>(); ++i) kc[i] = 0.0f;
                if (sigma_s > 0.0f) {
                    fetch_record<B, ST>(a.coef, a.slot, a.M, at, kc);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float q = kc[ch] * Y[0];
#pragma unroll
                        for (int b = 1; b < B; ++b) q += kc[3 * b + ch] * Y[b];
                        qe[ch] = q;
                        const float qs = group_sum(w * q);
                        col[ch] = fminf(fmaxf(qs, 0.0f), 1.0f);
                        Q[ch] = (qs >= 0.0f && qs <= 1.0f) ? wt * G[ch] : 0.0f;
                    }
                }
                const float sk = (((G[0] * col[0] + G[1] * col[1]) + G[2] * col[2]) + gap) + gd * mk;
                const float E = T * sk - (S - P);
                const float Dk = delta * E, Lk = sigma_s * E;                    // dL/d sigma_s, dL/d delta_k
                const float h = Dk * se + ((Q[0] * qe[0] + Q[1] * qe[1]) + Q[2] * qe[2]);
                const float yz = wy * wz, xz = wx * wz, xy = wx * wy;
                const float dwx = moves[0] ? (ex ? yz : -yz) : 0.0f;
                const float dwy = moves[1] ? (ey ? xz : -xz) : 0.0f;
                const float dwz = moves[2] ? (ez ? xy : -xy) : 0.0f;
                const float gp[3] = {g.inv[0] * group_sum(dwx * h), g.inv[1] * group_sum(dwy * h), g.inv[2] * group_sum(dwz * h)};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    gpo[i] += gp[i];
                    gpd[i] += mk * gp[i];
                }
                const float Mk = ((d[0] * gp[0] + d[1] * gp[1]) + d[2] * gp[2]) + gd * wt;   // dL/dm_k
                if (!cut) {
                    gt0 += Mk;
                    gdt += ((float)k + 0.5f) * Mk;
                } else {
                    const float hm = 0.5f * Mk, ld = L * Lk;
                    const float lower = hm - ld;
                    gt0 += lower;
                    gdt += (float)k * lower;
                    gt1 += hm + ld;
                    gL += (t1 - ak) * Lk;
                }
#pragma unroll
                for (int b = 0; b < B; ++b) gy[b] += (Q[0] * (w * kc[3 * b]) + Q[1] * (w * kc[3 * b + 1])) + Q[2] * (w * kc[3 * b + 2]);
                P += wt * sk;
                T = T * (1.0f - alpha);
                ++k;
                if (T < a.T_min) break;
            }
            // ---- the ray's end: the basis, dt, L, entry and exit --------------------------------------------
            float du[3] = {0.0f, 0.0f, 0.0f};                                   // dL/du = sum over b of dL/dY_b grad Y_b(u), increasing b
            if constexpr (B >= 4) {
                const float y1 = group_sum(gy[1]), y2 = group_sum(gy[2]), y3 = group_sum(gy[3]);
                du[1] = -0.48860251f * y1;
                du[2] = 0.48860251f * y2;
                du[0] = -0.48860251f * y3;
            }
            if constexpr (B >= 9) {
                const float y4 = group_sum(gy[4]), y5 = group_sum(gy[5]), y6 = group_sum(gy[6]), y7 = group_sum(gy[7]), y8 = group_sum(gy[8]);
                du[0] += (1.0925484f * uy) * y4;   du[1] += (1.0925484f * ux) * y4;
                du[1] += (-1.0925484f * uz) * y5;  du[2] += (-1.0925484f * uy) * y5;
                du[0] += (-0.63078314f * ux) * y6; du[1] += (-0.63078314f * uy) * y6; du[2] += (1.26156628f * uz) * y6;
                du[0] += (-1.0925484f * uz) * y7;  du[2] += (-1.0925484f * ux) * y7;
                du[0] += (1.09254844f * ux) * y8;  du[1] += (-1.09254844f * uy) * y8;
            }
            const float u[3] = {ux, uy, uz};
            const float udu = (ux * du[0] + uy * du[1]) + uz * du[2];
            const float cdt = gdt * -(a.step / ((L * L) * L)), cl = gL / L;
            const float q0 = ie >= 0 ? gt0 / (ie == 0 ? d[0] : ie == 1 ? d[1] : d[2]) : 0.0f;
            const float q1 = ix >= 0 ? gt1 / (ix == 0 ? d[0] : ix == 1 ? d[1] : d[2]) : 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                go[i] = gpo[i];
                gdir[i] = ((gpd[i] + (du[i] - u[i] * udu) / L) + cdt * d[i]) + cl * d[i];
                if (i == ie) {
                    go[i] -= q0;
                    gdir[i] -= q0 * t0;
                }
                if (i == ix) {
                    go[i] -= q1;
                    gdir[i] -= q1 * t1;
                }
            }
        }
    }
    if (e == 0) {
        float* out = a.d_rays + ray * 6;
        out[0] = go[0]; out[1] = go[1]; out[2] = go[2];
        out[3] = gdir[0]; out[4] = gdir[1]; out[5] = gdir[2];
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
// host side: checks, launches
// ------------------------------------------------------------------------------------------------
// vox_rule.h's checks under this library's status values
static int check_grid(const char* who, const mi_vox_grid* grid, Lattice* out) { return grid_ok(set_error, MI_VOX_MAX_RES, who, grid, out) ? MI_VOX_OK : MI_VOX_EINVAL; }
static int check_basis(const char* who, int B) { return basis_ok(set_error, who, B) ? MI_VOX_OK : MI_VOX_EINVAL; }
static int check_march(const char* who, const mi_vox_grid* grid, const mi_vox_render_cfg* cfg, int64_t n, int64_t* steps) {
    return march_ok(set_error, MI_VOX_MAX_STEPS, who, grid, cfg, n, steps) ? MI_VOX_OK : MI_VOX_EINVAL;
}

__host__ __device__ constexpr int record_bytes(int B, int fmt) {
    return fmt == MI_VOX_FMT_F32 ? 4 * record_floats(B) : fmt == MI_VOX_FMT_F16 ? 2 * record_floats(B) : 0;
}

// two arrays share a byte (the same array included)
static inline bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

static inline long long index_chunks(const Lattice& g) { return ((long long)g.P[0] * g.P[1] * g.P[2] + IDX_CHUNK - 1) / IDX_CHUNK; }
static inline size_t index_scratch_bytes(const Lattice& g) { return ((size_t)index_chunks(g) * sizeof(unsigned) + 15) & ~(size_t)15; }

static constexpr int VIEW_MAX_DIM = 8192;

// a view, and the ViewArgs of it (out may be NULL)
static int check_view(const char* who, const mi_vox_view* view, ViewArgs* out) {
    VOX_CHECK_ARG(view != nullptr, "%s: view is NULL", who);
    VOX_CHECK_ARG(view->H >= 1 && view->H <= VIEW_MAX_DIM && view->W >= 1 && view->W <= VIEW_MAX_DIM, "%s: H=%d, W=%d: 1 .. %d", who, view->H, view->W,
                  VIEW_MAX_DIM);
    VOX_CHECK_ARG(isfinite(view->fx) && isfinite(view->fy) && isfinite(view->cx) && isfinite(view->cy) && view->fx != 0.0f && view->fy != 0.0f,
                  "%s: fx=%g, fy=%g, cx=%g, cy=%g must be finite, fx and fy not 0", who, (double)view->fx, (double)view->fy, (double)view->cx, (double)view->cy);
    for (int i = 0; i < 12; ++i) VOX_CHECK_ARG(isfinite(view->c2w[i]), "%s: c2w[%d]=%g is not finite", who, i, (double)view->c2w[i]);
    VOX_CHECK_ARG(isfinite(view->depth_near) && view->depth_near >= 0.0f, "%s: depth_near=%g must be a finite number >= 0", who, (double)view->depth_near);
    VOX_CHECK_ARG(isfinite(view->depth_step) && view->depth_step > 0.0f, "%s: depth_step=%g must be a positive finite number", who, (double)view->depth_step);
    VOX_CHECK_ARG(view->slices >= GROUP && view->slices <= MI_VOX_MAX_STEPS && view->slices % GROUP == 0, "%s: slices=%d: a multiple of %d, %d .. %d", who,
                  view->slices, GROUP, GROUP, MI_VOX_MAX_STEPS);
    if (out) {
        ViewArgs v{};
        v.H = view->H; v.W = view->W; v.K = view->slices;
        v.fx = view->fx; v.fy = view->fy; v.cx = view->cx; v.cy = view->cy;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) v.R[3 * r + c] = view->c2w[4 * r + c];
            v.t[r] = view->c2w[4 * r + 3];
        }
        v.depth_near = view->depth_near; v.depth_step = view->depth_step;
        *out = v;
    }
    return MI_VOX_OK;
}

static inline size_t shadow_bytes(const ViewArgs& v) { return (size_t)v.H * v.W * v.K * sizeof(float); }

template <int ST>
static void launch_render(int B, dim3 blocks, hipStream_t st, const RenderArgs& a) {
    if (B == 1) hipLaunchKernelGGL((render_kernel<1, ST>), blocks, dim3(THREADS), 0, st, a);
    else if (B == 4) hipLaunchKernelGGL((render_kernel<4, ST>), blocks, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((render_kernel<9, ST>), blocks, dim3(THREADS), 0, st, a);
}

template <int ST>
static void launch_render_signed(int B, dim3 blocks, hipStream_t st, const RenderArgs& a) {
    if (B == 1) hipLaunchKernelGGL((render_signed_kernel<1, ST>), blocks, dim3(THREADS), 0, st, a);
    else if (B == 4) hipLaunchKernelGGL((render_signed_kernel<4, ST>), blocks, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((render_signed_kernel<9, ST>), blocks, dim3(THREADS), 0, st, a);
}

// mi_vox_render (slot_dev NULL, fmt and M unused) and mi_vox_render_sparse: one set of checks, one kernel body; is_signed: the two entries
// of A SIGNED GRID, the same checks and the signed kernel
static int render(const char* who, bool sparse, bool is_signed, const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const void* coef_dev,
                  const int32_t* slot_dev, int64_t M, const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg,
                  float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev, uint32_t* visited_dev, void* stream) {
    RenderArgs a{};
    if (int rc = check_grid(who, grid, &a.g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    if (sparse) {
        VOX_CHECK_ARG(fmt == MI_VOX_FMT_F32 || fmt == MI_VOX_FMT_F16, "%s: fmt=%d: MI_VOX_FMT_F32 (0) or MI_VOX_FMT_F16 (1)", who, fmt);
        VOX_CHECK_ARG(M >= 0 && M <= (int64_t)a.g.P[0] * a.g.P[1] * a.g.P[2], "%s: M=%lld: 0 .. the lattice's points", who, (long long)M);
    }
    int64_t steps;
    if (int rc = check_march(who, grid, cfg, n, &steps)) return rc;
    if (n == 0) return MI_VOX_OK;                                      // no work: the arrays of an empty ray set may be NULL
    if (sparse) {
        VOX_CHECK_ARG(sigma_dev && slot_dev && rays_dev && rgb_dev && (coef_dev || M == 0), "%s: NULL pointer", who);
        VOX_CHECK_ARG(aligned(coef_dev, 16) && aligned(slot_dev, 4), "%s: the table must be 16-byte aligned, slot 4-byte aligned", who);
    } else {
        VOX_CHECK_ARG(sigma_dev && coef_dev && rays_dev && rgb_dev, "%s: NULL pointer", who);
        VOX_CHECK_ARG(aligned(coef_dev, 16), "%s: coef must be 16-byte aligned", who);
    }
    VOX_CHECK_ARG(skip_dev || !cfg->use_skip, "%s: use_skip needs the skip plane", who);
    VOX_CHECK_ARG(aligned(sigma_dev, 4) && aligned(rays_dev, 4) && aligned(rgb_dev, 4) && aligned(disp_dev, 4) && aligned(acc_dev, 4) &&
                      aligned(depth_dev, 4) && aligned(visited_dev, 4),
                  "%s: a float or uint32 array is not 4-byte aligned", who);
    a.sigma = sigma_dev; a.coef = reinterpret_cast<const float4*>(coef_dev); a.slot = slot_dev; a.M = M; a.skip = skip_dev; a.rays = rays_dev; a.n = n;
    a.step = cfg->step; a.t_near = cfg->t_near; a.t_far = cfg->t_far; a.T_min = cfg->T_min;
    a.bg[0] = cfg->bg[0]; a.bg[1] = cfg->bg[1]; a.bg[2] = cfg->bg[2];
    a.use_skip = cfg->use_skip; a.max_steps = (int)steps;
    a.rgb = rgb_dev; a.disp = disp_dev; a.acc = acc_dev; a.depth = depth_dev; a.visited = visited_dev;
    const dim3 blocks((unsigned)((n + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK));
    hipStream_t st = (hipStream_t)stream;
    if (is_signed) {
        if (!sparse) launch_render_signed<DENSE>(B, blocks, st, a);
        else if (fmt == MI_VOX_FMT_F32) launch_render_signed<SPARSE32>(B, blocks, st, a);
        else launch_render_signed<SPARSE16>(B, blocks, st, a);
        VOX_LAUNCH_CHECK("render_signed_kernel");
        return MI_VOX_OK;
    }
    if (!sparse) launch_render<DENSE>(B, blocks, st, a);
    else if (fmt == MI_VOX_FMT_F32) launch_render<SPARSE32>(B, blocks, st, a);
    else launch_render<SPARSE16>(B, blocks, st, a);
    VOX_LAUNCH_CHECK("render_kernel");
    return MI_VOX_OK;
}

template <int ST>
static void launch_ray_grad(int B, dim3 blocks, hipStream_t st, const RayGradArgs& a) {
    if (B == 1) hipLaunchKernelGGL((ray_grad_kernel<1, ST>), blocks, dim3(THREADS), 0, st, a);
    else if (B == 4) hipLaunchKernelGGL((ray_grad_kernel<4, ST>), blocks, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((ray_grad_kernel<9, ST>), blocks, dim3(THREADS), 0, st, a);
}

// mi_vox_render_backward_rays (slot_dev NULL, fmt and M unused) and mi_vox_render_sparse_backward_rays: render()'s checks and conventions
static int ray_grad(const char* who, bool sparse, const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const void* coef_dev,
                    const int32_t* slot_dev, int64_t M, const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg,
                    const float* g_rgb_dev, const float* g_acc_dev, const float* g_depth_dev, float* d_rays_dev, float* rgb_check_dev,
                    float* acc_check_dev, float* depth_check_dev, void* stream) {
    RayGradArgs a{};
    if (int rc = check_grid(who, grid, &a.g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    if (sparse) {
        VOX_CHECK_ARG(fmt == MI_VOX_FMT_F32 || fmt == MI_VOX_FMT_F16, "%s: fmt=%d: MI_VOX_FMT_F32 (0) or MI_VOX_FMT_F16 (1)", who, fmt);
        VOX_CHECK_ARG(M >= 0 && M <= (int64_t)a.g.P[0] * a.g.P[1] * a.g.P[2], "%s: M=%lld: 0 .. the lattice's points", who, (long long)M);
    }
    int64_t steps;
    if (int rc = check_march(who, grid, cfg, n, &steps)) return rc;
    if (n == 0) return MI_VOX_OK;                                      // no work: the arrays of an empty ray set may be NULL
    if (sparse) {
        VOX_CHECK_ARG(sigma_dev && slot_dev && rays_dev && g_rgb_dev && d_rays_dev && (coef_dev || M == 0), "%s: NULL pointer", who);
        VOX_CHECK_ARG(aligned(coef_dev, 16) && aligned(slot_dev, 4), "%s: the table must be 16-byte aligned, slot 4-byte aligned", who);
    } else {
        VOX_CHECK_ARG(sigma_dev && coef_dev && rays_dev && g_rgb_dev && d_rays_dev, "%s: NULL pointer", who);
        VOX_CHECK_ARG(aligned(coef_dev, 16), "%s: coef must be 16-byte aligned", who);
    }
    VOX_CHECK_ARG(skip_dev || !cfg->use_skip, "%s: use_skip needs the skip plane", who);
    VOX_CHECK_ARG(aligned(sigma_dev, 4) && aligned(rays_dev, 4) && aligned(g_rgb_dev, 4) && aligned(g_acc_dev, 4) && aligned(g_depth_dev, 4) &&
                      aligned(d_rays_dev, 4) && aligned(rgb_check_dev, 4) && aligned(acc_check_dev, 4) && aligned(depth_check_dev, 4),
                  "%s: a float array is not 4-byte aligned", who);
    VOX_CHECK_ARG(!overlap(d_rays_dev, 24 * (size_t)n, rays_dev, 24 * (size_t)n), "%s: d_rays overlaps rays: the rays are read while d_rays is written", who);
    a.sigma = sigma_dev; a.coef = reinterpret_cast<const float4*>(coef_dev); a.slot = slot_dev; a.M = M; a.skip = skip_dev; a.rays = rays_dev; a.n = n;
    a.step = cfg->step; a.t_near = cfg->t_near; a.t_far = cfg->t_far; a.T_min = cfg->T_min;
    a.bg[0] = cfg->bg[0]; a.bg[1] = cfg->bg[1]; a.bg[2] = cfg->bg[2];
    a.use_skip = cfg->use_skip; a.max_steps = (int)steps;
    a.g_rgb = g_rgb_dev; a.g_acc = g_acc_dev; a.g_depth = g_depth_dev; a.d_rays = d_rays_dev;
    a.rgb = rgb_check_dev; a.acc = acc_check_dev; a.depth = depth_check_dev;
    const dim3 blocks((unsigned)((n + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK));
    hipStream_t st = (hipStream_t)stream;
    if (!sparse) launch_ray_grad<DENSE>(B, blocks, st, a);
    else if (fmt == MI_VOX_FMT_F32) launch_ray_grad<SPARSE32>(B, blocks, st, a);
    else launch_ray_grad<SPARSE16>(B, blocks, st, a);
    VOX_LAUNCH_CHECK("ray_grad_kernel");
    return MI_VOX_OK;
}

}  // namespace mivox

using namespace mivox;

extern "C" {

int mi_vox_abi_version(void) { return MI_VOX_ABI_VERSION; }
const char* mi_vox_last_error(void) { return g_err; }

int mi_vox_record_floats(int B) { return record_floats(B); }

size_t mi_vox_skip_bytes(const mi_vox_grid* grid) {
    Lattice g;
    if (check_grid("mi_vox_skip_bytes", grid, &g)) return 0;
    return (size_t)g.nb[0] * g.nb[1] * g.nb[2];
}

int64_t mi_vox_max_steps(const mi_vox_grid* grid, float step) {
    if (check_grid("mi_vox_max_steps", grid, nullptr)) return 0;
    if (!(isfinite(step) && step > 0.0f)) {
        set_error("mi_vox_max_steps: step=%g must be a positive finite number", (double)step);
        return 0;
    }
    return max_steps_of(grid, step);
}

int mi_vox_project(const mi_vox_grid* grid, int B, int D, const float* raw_dev, const float* proj_dev, const int64_t* index_dev, int64_t M,
                   float* sigma_dev, float* coef_dev, void* stream) {
    const char* who = "mi_vox_project";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    VOX_CHECK_ARG(D >= B && D <= MI_VOX_MAX_DIRS, "%s: D=%d: B=%d .. %d directions", who, D, B, MI_VOX_MAX_DIRS);
    VOX_CHECK_ARG(M >= 0 && M <= ((int64_t)1 << 31) * THREADS - 1, "%s: M=%lld out of range", who, (long long)M);
    if (M == 0) return MI_VOX_OK;                                      // no work: the arrays of an empty list may be NULL
    VOX_CHECK_ARG(raw_dev && proj_dev && index_dev && coef_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(raw_dev, 16) && aligned(coef_dev, 16), "%s: raw and coef must be 16-byte aligned", who);
    VOX_CHECK_ARG(aligned(proj_dev, 4) && aligned(sigma_dev, 4) && aligned(index_dev, 8), "%s: proj, sigma (4 bytes) or index (8 bytes) is misaligned", who);
    const long long N = (long long)g.P[0] * g.P[1] * g.P[2];
    const dim3 blocks((unsigned)((M + THREADS - 1) / THREADS));
    hipStream_t st = (hipStream_t)stream;
    const float4* raw4 = reinterpret_cast<const float4*>(raw_dev);
    const long long* idx = reinterpret_cast<const long long*>(index_dev);
    float4* coef4 = reinterpret_cast<float4*>(coef_dev);
    if (B == 1) hipLaunchKernelGGL(project_kernel<1>, blocks, dim3(THREADS), 0, st, raw4, proj_dev, idx, (long long)M, D, N, sigma_dev, coef4);
    else if (B == 4) hipLaunchKernelGGL(project_kernel<4>, blocks, dim3(THREADS), 0, st, raw4, proj_dev, idx, (long long)M, D, N, sigma_dev, coef4);
    else hipLaunchKernelGGL(project_kernel<9>, blocks, dim3(THREADS), 0, st, raw4, proj_dev, idx, (long long)M, D, N, sigma_dev, coef4);
    VOX_LAUNCH_CHECK("project_kernel");
    return MI_VOX_OK;
}

int mi_vox_build_skip(const mi_vox_grid* grid, const float* sigma_dev, uint8_t* skip_dev, void* stream) {
    const char* who = "mi_vox_build_skip";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    VOX_CHECK_ARG(sigma_dev && skip_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(sigma_dev, 4), "%s: sigma must be 4-byte aligned", who);
    hipLaunchKernelGGL(skip_kernel, dim3((unsigned)(g.nb[0] * g.nb[1] * g.nb[2])), dim3(64), 0, (hipStream_t)stream, g, sigma_dev, skip_dev);
    VOX_LAUNCH_CHECK("skip_kernel");
    return MI_VOX_OK;
}

int mi_vox_render(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev, const float* rays_dev,
                  int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev,
                  uint32_t* visited_dev, void* stream) {
    return render("mi_vox_render", false, false, grid, B, MI_VOX_FMT_F32, sigma_dev, coef_dev, nullptr, 0, skip_dev, rays_dev, n, cfg, rgb_dev, disp_dev, acc_dev,
                  depth_dev, visited_dev, stream);
}

int mi_vox_render_sparse(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev, int64_t M,
                         const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev,
                         float* acc_dev, float* depth_dev, uint32_t* visited_dev, void* stream) {
    return render("mi_vox_render_sparse", true, false, grid, B, fmt, sigma_dev, table_dev, slot_dev, M, skip_dev, rays_dev, n, cfg, rgb_dev, disp_dev, acc_dev,
                  depth_dev, visited_dev, stream);
}

size_t mi_vox_record_bytes(int B, int fmt) { return (size_t)record_bytes(B, fmt); }

size_t mi_vox_index_scratch_bytes(const mi_vox_grid* grid) {
    Lattice g;
    if (check_grid("mi_vox_index_scratch_bytes", grid, &g)) return 0;
    return index_scratch_bytes(g);
}

int mi_vox_index(const mi_vox_grid* grid, const float* sigma_dev, int32_t* slot_dev, int64_t* count_dev, void* scratch_dev, size_t scratch_bytes,
                 void* stream) {
    const char* who = "mi_vox_index";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    VOX_CHECK_ARG(sigma_dev && slot_dev && count_dev && scratch_dev, "%s: NULL pointer", who);
    const size_t need = index_scratch_bytes(g);
    VOX_CHECK_ARG(scratch_bytes >= need, "%s: scratch too small: %zu < %zu (mi_vox_index_scratch_bytes)", who, scratch_bytes, need);
    VOX_CHECK_ARG(aligned(sigma_dev, 4) && aligned(slot_dev, 4) && aligned(count_dev, 8) && aligned(scratch_dev, 16),
                  "%s: sigma, slot (4 bytes), count (8 bytes) or scratch (16 bytes) is misaligned", who);
    const long long N = (long long)g.P[0] * g.P[1] * g.P[2];
    const int nb = (int)index_chunks(g);
    unsigned* counts = reinterpret_cast<unsigned*>(scratch_dev);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(index_flag_kernel, dim3((unsigned)nb), dim3(THREADS), 0, st, g, sigma_dev, slot_dev, counts, N);
    VOX_LAUNCH_CHECK("index_flag_kernel");
    hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(1024), 0, st, counts, nb, reinterpret_cast<long long*>(count_dev));
    VOX_LAUNCH_CHECK("index_scan_kernel");
    hipLaunchKernelGGL(index_emit_kernel, dim3((unsigned)nb), dim3(THREADS), 0, st, slot_dev, counts, N);
    VOX_LAUNCH_CHECK("index_emit_kernel");
    return MI_VOX_OK;
}

int mi_vox_pack(const mi_vox_grid* grid, int B, int fmt, const float* src_dev, const int32_t* slot_dev, int64_t M, void* table_dev, void* stream) {
    const char* who = "mi_vox_pack";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    VOX_CHECK_ARG(fmt == MI_VOX_FMT_F32 || fmt == MI_VOX_FMT_F16, "%s: fmt=%d: MI_VOX_FMT_F32 (0) or MI_VOX_FMT_F16 (1)", who, fmt);
    const long long N = (long long)g.P[0] * g.P[1] * g.P[2];
    VOX_CHECK_ARG(M >= 0 && M <= N, "%s: M=%lld: 0 .. the lattice's points", who, (long long)M);
    if (M == 0) return MI_VOX_OK;                                      // no work: the arrays of an empty table may be NULL
    VOX_CHECK_ARG(src_dev && table_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(src_dev, 16) && aligned(table_dev, 16) && aligned(slot_dev, 4), "%s: src and table must be 16-byte aligned, slot 4-byte aligned", who);
    const int R4 = record_floats(B) / 4;
    const long long records = slot_dev ? N : (long long)M;
    const dim3 blocks((unsigned)((records * R4 + THREADS - 1) / THREADS));
    hipStream_t st = (hipStream_t)stream;
    const float4* src4 = reinterpret_cast<const float4*>(src_dev);
    if (fmt == MI_VOX_FMT_F16) hipLaunchKernelGGL(pack_kernel<true>, blocks, dim3(THREADS), 0, st, src4, slot_dev, records, (long long)M, R4, table_dev);
    else hipLaunchKernelGGL(pack_kernel<false>, blocks, dim3(THREADS), 0, st, src4, slot_dev, records, (long long)M, R4, table_dev);
    VOX_LAUNCH_CHECK("pack_kernel");
    return MI_VOX_OK;
}

int mi_vox_resample(const mi_vox_grid* src, const mi_vox_grid* dst, int B, const float* sigma_src_dev, const float* coef_src_dev, float* sigma_dst_dev,
                    float* coef_dst_dev, void* stream) {
    const char* who = "mi_vox_resample";
    ResampleArgs a{};
    if (int rc = check_grid("mi_vox_resample: source", src, &a.s)) return rc;
    if (int rc = check_grid("mi_vox_resample: destination", dst, &a.d)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    VOX_CHECK_ARG(sigma_src_dev && coef_src_dev && sigma_dst_dev && coef_dst_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(coef_src_dev, 16) && aligned(coef_dst_dev, 16) && aligned(sigma_src_dev, 4) && aligned(sigma_dst_dev, 4),
                  "%s: coef must be 16-byte aligned, sigma 4-byte aligned", who);
    const int R4 = record_floats(B) / 4;
    const size_t Ns = (size_t)a.s.P[0] * a.s.P[1] * a.s.P[2], Nd = (size_t)a.d.P[0] * a.d.P[1] * a.d.P[2];
    VOX_CHECK_ARG(!overlap(sigma_dst_dev, 4 * Nd, sigma_src_dev, 4 * Ns) && !overlap(sigma_dst_dev, 4 * Nd, coef_src_dev, 16 * Ns * R4) &&
                      !overlap(coef_dst_dev, 16 * Nd * R4, sigma_src_dev, 4 * Ns) && !overlap(coef_dst_dev, 16 * Nd * R4, coef_src_dev, 16 * Ns * R4) &&
                      !overlap(sigma_dst_dev, 4 * Nd, coef_dst_dev, 16 * Nd * R4),
                  "%s: a destination array overlaps a source array or the other destination array: the source is read while the destination is written", who);
    for (int i = 0; i < 3; ++i) a.step_d[i] = (dst->hi[i] - dst->lo[i]) / (float)dst->res[i];
    a.sigma_s = sigma_src_dev; a.coef_s = reinterpret_cast<const float4*>(coef_src_dev);
    a.sigma_d = sigma_dst_dev; a.coef_d = reinterpret_cast<float4*>(coef_dst_dev);
    a.pieces = (long long)Nd * R4;
    const dim3 blocks((unsigned)((a.pieces + THREADS - 1) / THREADS));
    hipStream_t st = (hipStream_t)stream;
    if (B == 1) hipLaunchKernelGGL(resample_kernel<1>, blocks, dim3(THREADS), 0, st, a);
    else if (B == 4) hipLaunchKernelGGL(resample_kernel<4>, blocks, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(resample_kernel<9>, blocks, dim3(THREADS), 0, st, a);
    VOX_LAUNCH_CHECK("resample_kernel");
    return MI_VOX_OK;
}

int mi_vox_prune(const mi_vox_grid* grid, int B, float tau, const float* sigma_in_dev, float* sigma_out_dev, float* coef_dev, void* stream) {
    const char* who = "mi_vox_prune";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    VOX_CHECK_ARG(isfinite(tau) && tau >= 0.0f, "%s: tau=%g must be a finite number >= 0", who, (double)tau);
    VOX_CHECK_ARG(sigma_in_dev && sigma_out_dev && coef_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(coef_dev, 16) && aligned(sigma_in_dev, 4) && aligned(sigma_out_dev, 4), "%s: coef must be 16-byte aligned, sigma 4-byte aligned", who);
    const int R4 = record_floats(B) / 4;
    const size_t N = (size_t)g.P[0] * g.P[1] * g.P[2];
    VOX_CHECK_ARG(!overlap(sigma_out_dev, 4 * N, sigma_in_dev, 4 * N), "%s: sigma_out overlaps sigma_in: the stencil reads a point's neighbours", who);
    VOX_CHECK_ARG(!overlap(coef_dev, 16 * N * R4, sigma_in_dev, 4 * N) && !overlap(coef_dev, 16 * N * R4, sigma_out_dev, 4 * N), "%s: coef overlaps a sigma plane", who);
    const long long pieces = (long long)N * R4;
    const dim3 blocks((unsigned)((pieces + THREADS - 1) / THREADS));
    hipStream_t st = (hipStream_t)stream;
    float4* coef4 = reinterpret_cast<float4*>(coef_dev);
    if (B == 1) hipLaunchKernelGGL(prune_kernel<1>, blocks, dim3(THREADS), 0, st, g, tau, sigma_in_dev, sigma_out_dev, coef4, pieces);
    else if (B == 4) hipLaunchKernelGGL(prune_kernel<4>, blocks, dim3(THREADS), 0, st, g, tau, sigma_in_dev, sigma_out_dev, coef4, pieces);
    else hipLaunchKernelGGL(prune_kernel<9>, blocks, dim3(THREADS), 0, st, g, tau, sigma_in_dev, sigma_out_dev, coef4, pieces);
    VOX_LAUNCH_CHECK("prune_kernel");
    return MI_VOX_OK;
}

size_t mi_vox_shadow_bytes(const mi_vox_view* view) {
    ViewArgs v;
    if (check_view("mi_vox_shadow_bytes", view, &v)) return 0;
    return shadow_bytes(v);
}

int mi_vox_shadow(const mi_vox_grid* grid, const float* sigma_dev, const uint8_t* skip_dev, const mi_vox_view* view, float* tvol_dev, void* stream) {
    const char* who = "mi_vox_shadow";
    ShadowArgs a{};
    if (int rc = check_grid(who, grid, &a.g)) return rc;
    if (int rc = check_view(who, view, &a.v)) return rc;
    VOX_CHECK_ARG(sigma_dev && tvol_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(sigma_dev, 4) && aligned(tvol_dev, 32), "%s: sigma must be 4-byte aligned, tvol 32-byte aligned", who);
    const size_t N = (size_t)a.g.P[0] * a.g.P[1] * a.g.P[2];
    VOX_CHECK_ARG(!overlap(tvol_dev, shadow_bytes(a.v), sigma_dev, 4 * N), "%s: tvol overlaps sigma: sigma is read while tvol is written", who);
    a.sigma = sigma_dev; a.skip = skip_dev; a.tvol = tvol_dev;
    const long long rays = (long long)a.v.H * a.v.W;
    hipLaunchKernelGGL(shadow_kernel, dim3((unsigned)((rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), dim3(THREADS), 0, (hipStream_t)stream, a);
    VOX_LAUNCH_CHECK("shadow_kernel");
    return MI_VOX_OK;
}

int mi_vox_seen(const mi_vox_grid* grid, const mi_vox_view* view, const float* tvol_dev, int32_t bias, float* od_dev, void* stream) {
    const char* who = "mi_vox_seen";
    SeenArgs a{};
    if (int rc = check_grid(who, grid, &a.g)) return rc;
    if (int rc = check_view(who, view, &a.v)) return rc;
    VOX_CHECK_ARG(bias >= 0, "%s: bias=%d must be >= 0 slices", who, bias);
    VOX_CHECK_ARG(tvol_dev && od_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(tvol_dev, 32) && aligned(od_dev, 4), "%s: tvol must be 32-byte aligned, od 4-byte aligned", who);
    a.N = (long long)a.g.P[0] * a.g.P[1] * a.g.P[2];
    VOX_CHECK_ARG(!overlap(od_dev, 4 * (size_t)a.N, tvol_dev, shadow_bytes(a.v)), "%s: od overlaps tvol: tvol is read while od is written", who);
    for (int i = 0; i < 3; ++i) a.step[i] = (grid->hi[i] - grid->lo[i]) / (float)grid->res[i];
    a.tvol = tvol_dev; a.od = od_dev; a.bias = bias;
    hipLaunchKernelGGL(seen_kernel, dim3((unsigned)((a.N + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    VOX_LAUNCH_CHECK("seen_kernel");
    return MI_VOX_OK;
}

int mi_vox_prune_seen(const mi_vox_grid* grid, int B, float tau, float od_max, const float* sigma_in_dev, const float* od_dev, float* sigma_out_dev,
                      float* coef_dev, void* stream) {
    const char* who = "mi_vox_prune_seen";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    if (int rc = check_basis(who, B)) return rc;
    VOX_CHECK_ARG(isfinite(tau) && tau >= 0.0f, "%s: tau=%g must be a finite number >= 0", who, (double)tau);
    VOX_CHECK_ARG(od_max >= 0.0f, "%s: od_max=%g must be >= 0 (it may be infinite)", who, (double)od_max);
    VOX_CHECK_ARG(sigma_in_dev && od_dev && sigma_out_dev && coef_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(coef_dev, 16) && aligned(sigma_in_dev, 4) && aligned(sigma_out_dev, 4) && aligned(od_dev, 4),
                  "%s: coef must be 16-byte aligned, sigma and od 4-byte aligned", who);
    const int R4 = record_floats(B) / 4;
    const size_t N = (size_t)g.P[0] * g.P[1] * g.P[2];
    VOX_CHECK_ARG(!overlap(sigma_out_dev, 4 * N, sigma_in_dev, 4 * N), "%s: sigma_out overlaps sigma_in: the stencil reads a point's neighbours", who);
    VOX_CHECK_ARG(!overlap(coef_dev, 16 * N * R4, sigma_in_dev, 4 * N) && !overlap(coef_dev, 16 * N * R4, sigma_out_dev, 4 * N), "%s: coef overlaps a sigma plane", who);
    VOX_CHECK_ARG(!overlap(od_dev, 4 * N, sigma_out_dev, 4 * N) && !overlap(od_dev, 4 * N, coef_dev, 16 * N * R4), "%s: od overlaps sigma_out or coef: it is read while they are written", who);
    const long long pieces = (long long)N * R4;
    const dim3 blocks((unsigned)((pieces + THREADS - 1) / THREADS));
    hipStream_t st = (hipStream_t)stream;
    float4* coef4 = reinterpret_cast<float4*>(coef_dev);
    if (B == 1) hipLaunchKernelGGL(prune_seen_kernel<1>, blocks, dim3(THREADS), 0, st, g, tau, od_max, sigma_in_dev, od_dev, sigma_out_dev, coef4, pieces);
    else if (B == 4) hipLaunchKernelGGL(prune_seen_kernel<4>, blocks, dim3(THREADS), 0, st, g, tau, od_max, sigma_in_dev, od_dev, sigma_out_dev, coef4, pieces);
    else hipLaunchKernelGGL(prune_seen_kernel<9>, blocks, dim3(THREADS), 0, st, g, tau, od_max, sigma_in_dev, od_dev, sigma_out_dev, coef4, pieces);
    VOX_LAUNCH_CHECK("prune_seen_kernel");
    return MI_VOX_OK;
}

int mi_vox_render_backward_rays(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev,
                                const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, const float* g_rgb_dev, const float* g_acc_dev,
                                const float* g_depth_dev, float* d_rays_dev, float* rgb_check_dev, float* acc_check_dev, float* depth_check_dev,
                                void* stream) {
    return ray_grad("mi_vox_render_backward_rays", false, grid, B, MI_VOX_FMT_F32, sigma_dev, coef_dev, nullptr, 0, skip_dev, rays_dev, n, cfg, g_rgb_dev,
                    g_acc_dev, g_depth_dev, d_rays_dev, rgb_check_dev, acc_check_dev, depth_check_dev, stream);
}

int mi_vox_render_sparse_backward_rays(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev,
                                       int64_t M, const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg,
                                       const float* g_rgb_dev, const float* g_acc_dev, const float* g_depth_dev, float* d_rays_dev, float* rgb_check_dev,
                                       float* acc_check_dev, float* depth_check_dev, void* stream) {
    return ray_grad("mi_vox_render_sparse_backward_rays", true, grid, B, fmt, sigma_dev, table_dev, slot_dev, M, skip_dev, rays_dev, n, cfg, g_rgb_dev,
                    g_acc_dev, g_depth_dev, d_rays_dev, rgb_check_dev, acc_check_dev, depth_check_dev, stream);
}

int mi_vox_build_skip_signed(const mi_vox_grid* grid, const float* sigma_dev, uint8_t* skip_dev, void* stream) {
    const char* who = "mi_vox_build_skip_signed";
    Lattice g;
    if (int rc = check_grid(who, grid, &g)) return rc;
    VOX_CHECK_ARG(sigma_dev && skip_dev, "%s: NULL pointer", who);
    VOX_CHECK_ARG(aligned(sigma_dev, 4), "%s: sigma must be 4-byte aligned", who);
    hipLaunchKernelGGL(skip_signed_kernel, dim3((unsigned)(g.nb[0] * g.nb[1] * g.nb[2])), dim3(64), 0, (hipStream_t)stream, g, sigma_dev, skip_dev);
    VOX_LAUNCH_CHECK("skip_signed_kernel");
    return MI_VOX_OK;
}

int mi_vox_render_signed(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev, const float* rays_dev,
                         int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev,
                         uint32_t* visited_dev, void* stream) {
    return render("mi_vox_render_signed", false, true, grid, B, MI_VOX_FMT_F32, sigma_dev, coef_dev, nullptr, 0, skip_dev, rays_dev, n, cfg, rgb_dev, disp_dev,
                  acc_dev, depth_dev, visited_dev, stream);
}

int mi_vox_render_sparse_signed(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev, int64_t M,
                                const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev,
                                float* disp_dev, float* acc_dev, float* depth_dev, uint32_t* visited_dev, void* stream) {
    return render("mi_vox_render_sparse_signed", true, true, grid, B, fmt, sigma_dev, table_dev, slot_dev, M, skip_dev, rays_dev, n, cfg, rgb_dev, disp_dev,
                  acc_dev, depth_dev, visited_dev, stream);
}

}  // extern "C"
