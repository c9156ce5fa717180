// vox_rule.h -- what csrc/vox.hip (the radiance-grid renderer) and csrc/voxgrad.hip (its backward pass) both need of THE RENDER RULE of
// include/mi_nerf_vox.h, written once: the launch-shape constants, the record layout, the Lattice, the basis, a point's cell and fraction, the sum over a group's eight
// lanes, lane e's record fetch for the three storages, and on the host side the checks of a grid and of a march configuration.  Like
// abi_error.h it knows no public header: the two libraries' grid and cfg structs reach it as template parameters, and each source
// static_asserts the constants below against its own header.  Everything here is __device__ __forceinline__ or static / inline host
// code: neither library gains a symbol.  No atomic.
//
// What is NOT here is the march itself -- slab, interval, jump, compositing: each kernel spells its own loop.  A forced-inline function is
// optimised on its own before it is inlined, and one that holds the loop (or takes part of its state by reference) reaches the kernel in
// another shape than the same text written in place: the renderer's generated code changed, and with it its speed
// (docs/design/23_radiance_grid_training.md, 23.3).  The pieces below were each checked to leave all kernels' code as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// The including source names its own namespace first (#define VOX_RULE_NAMESPACE mivox): Lattice is a kernel parameter type, so the
// kernels' mangled names stay those of the library.
namespace VOX_RULE_NAMESPACE {

constexpr int THREADS = 256;
constexpr int GROUP = 8;                                 // lanes per ray: the corners of a cell
constexpr int RAYS_PER_BLOCK = THREADS / GROUP;
constexpr int BLK = 8;                                   // cells per axis of a block of the skip plane
constexpr float EPS32 = 5.9604645e-8f;                   // 2^-24

__host__ __device__ constexpr int record_floats(int B) { return B == 1 ? 4 : B == 4 ? 16 : B == 9 ? 32 : 0; }

// the grid as the kernels see it
struct Lattice {
    float lo[3], hi[3], inv[3];
    int res[3];
    int P[3];                                            // points per axis
    int nb[3];                                           // blocks per axis
};

// the basis of the header at a unit vector
template <int B>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float (&Y)[B]) {
    Y[0] = 0.28209479f;
    if constexpr (B >= 4) {
        Y[1] = -0.48860251f * y;
        Y[2] = 0.48860251f * z;
        Y[3] = -0.48860251f * x;
    }
    if constexpr (B >= 9) {
        Y[4] = 1.0925484f * (x * y);
        Y[5] = -1.0925484f * (y * z);
        Y[6] = 0.31539157f * (((2.0f * z) * z - x * x) - y * y);
        Y[7] = -1.0925484f * (x * z);
        Y[8] = 0.54627422f * (x * x - y * y);
    }
}

// step 3's cell and fraction on one axis, from the lattice coordinate g_i = (p_i - lo_i) * inv_i: the renderer's sample and THE RESAMPLING
// RULE's lattice point find their cell here
__device__ __forceinline__ void cell_of(float gi, int res, int& c, float& f) {
    c = min(max((int)floorf(gi), 0), res - 1);
    f = fminf(fmaxf(gi - (float)c, 0.0f), 1.0f);
}

// the sum over a group's eight lanes, in the header's order: x neighbours, y neighbours, then the two halves.  Every lane ends with the
// same bits (an addition commutes).  quad_perm [1,0,3,2] and [2,3,0,1] exchange within a quad; after them a quad's four lanes agree, so
// the mirror of the half-row (lane i <-> 7 - i) hands each lane the other quad's sum.
__device__ __forceinline__ float dpp_quad_x(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)); }
__device__ __forceinline__ float dpp_quad_y(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)); }
__device__ __forceinline__ float dpp_half_mirror(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true)); }
__device__ __forceinline__ float group_sum(float v) {
    v = v + dpp_quad_x(v);
    v = v + dpp_quad_y(v);
    return v + dpp_half_mirror(v);
}

// where an instantiation finds corner e's record
constexpr int DENSE = 0;                                 // coef[flat(corner)], fp32
constexpr int SPARSE32 = 1;                              // table[slot[corner]], fp32
constexpr int SPARSE16 = 2;                              // table[slot[corner]], binary16

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
// two binary16 values of one 32-bit word, widened exactly
__device__ __forceinline__ void widen2(unsigned u, float& lo, float& hi) {
    const half2_t h = __builtin_bit_cast(half2_t, u);
    lo = (float)h.x;
    hi = (float)h.y;
}

// floats a lane holds of its corner's record
template <int B, int ST>
constexpr int record_regs() { return ST == SPARSE16 && B > 1 ? 8 * ((3 * B + 7) / 8) : 4 * ((3 * B + 3) / 4); }

// lane e's record: one aligned piece of the dense array coef, or of the table coef once the slot is known (slot, M: compact grids only)
template <int B, int ST>
__device__ __forceinline__ void fetch_record(const float4* coef, const int* slot, long long M, long long at, float (&kc)[record_regs<B, ST>()]) {
    constexpr int R4 = record_floats(B) / 4;               // 16-byte pieces of an fp32 record
    constexpr int V4 = (3 * B + 3) / 4;                    // the pieces that hold coefficients
    constexpr int H4 = (3 * B + 7) / 8;                    // ... of a binary16 record (B > 1; the B = 1 record is one 8-byte piece)
    if constexpr (ST == DENSE) {
        const float4* rec = coef + at * R4;
#pragma unroll
        for (int q = 0; q < V4; ++q) {
            const float4 v = rec[q];
            kc[4 * q] = v.x; kc[4 * q + 1] = v.y; kc[4 * q + 2] = v.z; kc[4 * q + 3] = v.w;
        }
    } else {
        // The slot is read here, after the sigma_s > 0 decision.  Written beside the sigma load it lands here all the same: the
        // compiler sinks a load into the one branch that uses it (docs/design/22_radiance_grid.md, 22.9).
        // A slot outside [0, M) is a zero record and no load (the one branch that is not uniform in a group: it closes
        // before the next DPP sum).
#pragma unroll
        for (int i = 0; i < record_regs<B, ST>(); ++i) kc[i] = 0.0f;
        const int sl = slot[at];
        if (sl >= 0 && (long long)sl < M) {
            if constexpr (ST == SPARSE32) {
                const float4* rec = coef + (long long)sl * R4;
#pragma unroll
                for (int q = 0; q < V4; ++q) {
                    const float4 v = rec[q];
                    kc[4 * q] = v.x; kc[4 * q + 1] = v.y; kc[4 * q + 2] = v.z; kc[4 * q + 3] = v.w;
                }
            } else if constexpr (B == 1) {
                const uint2 v = reinterpret_cast<const uint2*>(coef)[sl];              // the whole 8-byte record
                widen2(v.x, kc[0], kc[1]);
                widen2(v.y, kc[2], kc[3]);
            } else {
                const uint4* rec = reinterpret_cast<const uint4*>(coef) + (long long)sl * (R4 / 2);
#pragma unroll
                for (int q = 0; q < H4; ++q) {
                    const uint4 v = rec[q];
                    widen2(v.x, kc[8 * q], kc[8 * q + 1]);
                    widen2(v.y, kc[8 * q + 2], kc[8 * q + 3]);
                    widen2(v.z, kc[8 * q + 4], kc[8 * q + 5]);
                    widen2(v.w, kc[8 * q + 6], kc[8 * q + 7]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks of a grid and of a march configuration that both libraries make, worded alike.  Like abi_error.h this file
// knows neither library's header: the grid and cfg structs are template parameters, the limits of the header are arguments, and a
// refusal is written through the library's own set_error.  false: refused.  Each library wraps the three in a line of its own that
// returns its status.
// ------------------------------------------------------------------------------------------------
typedef void (*Refuse)(const char* fmt, ...);
#define VOX_RULE_REQUIRE(cond, ...) do { if (!(cond)) { refuse(__VA_ARGS__); return false; } } while (0)

static inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the samples a ray can take at most: the box's diagonal over the step, rounded up, plus one
template <class Grid>
static int64_t max_steps_of(const Grid* grid, float step) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double e = (double)grid->hi[i] - (double)grid->lo[i];
        s += e * e;
    }
    const double q = ceil(sqrt(s) / (double)step);
    return q >= 9.0e18 ? INT64_MAX : (int64_t)q + 1;
}

// the grid, and the Lattice of it (out may be NULL)
template <class Grid>
static bool grid_ok(Refuse refuse, int max_res, const char* who, const Grid* grid, Lattice* out) {
    VOX_RULE_REQUIRE(grid != nullptr, "%s: grid is NULL", who);
    Lattice g{};
    for (int i = 0; i < 3; ++i) {
        const float lo = grid->lo[i], hi = grid->hi[i];
        const int res = grid->res[i];
        VOX_RULE_REQUIRE(res >= 1 && res <= max_res, "%s: res[%d]=%d: 1 .. %d", who, i, res, max_res);
        VOX_RULE_REQUIRE(isfinite(lo) && isfinite(hi) && lo < hi, "%s: axis %d: lo=%g, hi=%g must be finite with lo < hi", who, i, (double)lo, (double)hi);
        const float step = (hi - lo) / (float)res, inv = (float)res / (hi - lo);
        VOX_RULE_REQUIRE(isfinite(step) && step > 0.0f && isfinite(inv) && inv > 0.0f, "%s: axis %d: the step %g of [%g, %g] / %d is not a positive finite float",
                         who, i, (double)step, (double)lo, (double)hi, res);
        g.lo[i] = lo; g.hi[i] = hi; g.inv[i] = inv; g.res[i] = res; g.P[i] = res + 1; g.nb[i] = (res + BLK - 1) / BLK;
    }
    if (out) *out = g;
    return true;
}

static bool basis_ok(Refuse refuse, const char* who, int B) {
    VOX_RULE_REQUIRE(record_floats(B) != 0, "%s: B=%d: 1, 4 or 9 basis functions", who, B);
    return true;
}

// cfg, the step bound (-> *steps) and the ray count
template <class Grid, class Cfg>
static bool march_ok(Refuse refuse, int max_steps, const char* who, const Grid* grid, const Cfg* cfg, int64_t n, int64_t* steps) {
    VOX_RULE_REQUIRE(cfg != nullptr, "%s: cfg is NULL", who);
    VOX_RULE_REQUIRE(isfinite(cfg->step) && cfg->step > 0.0f, "%s: step=%g must be a positive finite number", who, (double)cfg->step);
    VOX_RULE_REQUIRE(cfg->t_near < cfg->t_far, "%s: t_near=%g must lie below t_far=%g", who, (double)cfg->t_near, (double)cfg->t_far);
    VOX_RULE_REQUIRE(cfg->T_min >= 0.0f && cfg->T_min < 1.0f, "%s: T_min=%g: 0 <= T_min < 1", who, (double)cfg->T_min);
    VOX_RULE_REQUIRE(isfinite(cfg->bg[0]) && isfinite(cfg->bg[1]) && isfinite(cfg->bg[2]), "%s: the background must be finite", who);
    VOX_RULE_REQUIRE(cfg->use_skip == 0 || cfg->use_skip == 1, "%s: use_skip=%d must be 0 or 1", who, cfg->use_skip);
    *steps = max_steps_of(grid, cfg->step);
    VOX_RULE_REQUIRE(*steps <= max_steps, "%s: step=%g gives up to %lld samples per ray, more than %d", who, (double)cfg->step, (long long)*steps, max_steps);
    VOX_RULE_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31) * RAYS_PER_BLOCK - 1, "%s: n=%lld out of range", who, (long long)n);
    return true;
}

}  // namespace VOX_RULE_NAMESPACE
