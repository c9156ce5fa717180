// optim.hip -- libmi_nerf_optim.so (include/mi_nerf_optim.h): the Adam / AdamW step over many small fp32 tensors, plain and guarded.  A
// library of its own: it shares abi_error.h with the others at compile time and nothing at link time.
//
//   adam_kernel<GUARDED>     one workgroup per chunk of MI_OPTIM_CHUNK elements of one tensor.  The per-tensor table (pointers, sizes, the
//                            chunk-count prefix, the bias corrections) is the kernel's argument: the workgroup finds (tensor, chunk) from its
//                            block index by a binary search over the prefix, then takes one path for the whole chunk -- 16-byte accesses
//                            when p, g, m and v of that tensor are 16-byte aligned, 4-byte accesses otherwise.  16 elements per thread, all
//                            loads issued before the first store.  GUARDED: the clip coefficient and the skip word come from the control
//                            block, the bias corrections from the per-tensor device state.
//   lazy_adam_kernel         THE LAZY UPDATE on the same mapping: a thread loads its 16 gradients first and touches p, m, v only for a
//                            16-byte piece (4-byte path: an element) in which some g != 0; untouched components of a touched piece are
//                            stored back as loaded (a select), a touched gradient is overwritten with +0 under `consume`.  Whole waves
//                            and chunks fall through on one predicate: an untouched chunk is 16 KiB of gradient reads and nothing else.
//   grad_partial_kernel      the same mapping over the gradients alone: (sum of squares in double, non-finite count) of the chunk ->
//                            scratch[chunk], thread-sequential, then lanes, then the four waves: a fixed order.
//   grad_finish_kernel       one workgroup: adds the partials (a contiguous run per thread in index order, then a fixed tree), writes the
//                            control block from thread 0 with ordinary stores, and advances the per-tensor state, one thread per tensor.
//
// No atomic, no host synchronisation, no copy, no allocation.  Compiled with -ffp-contract=off: THE UPDATE is evaluated as it is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/mi_nerf_optim.h"
#include "abi_error.h"

namespace mioptim {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_OPTIM_EHIP)
#define OPTIM_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mioptim, MI_OPTIM_EINVAL, cond, __VA_ARGS__)
#define OPTIM_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mioptim, name)

constexpr int MAXT = MI_OPTIM_MAX_TENSORS;
constexpr int CHUNK = MI_OPTIM_CHUNK;
constexpr int THREADS = 256;
constexpr int PER_THREAD = CHUNK / THREADS;             // 16 elements: four 16-byte accesses or sixteen 4-byte ones
static_assert(CHUNK == THREADS * PER_THREAD && PER_THREAD == 16, "the kernels unroll 4 x 4 elements per thread");

// ------------------------------------------------------------------------------------------------
// the constants of THE UPDATE: formed in double, rounded once.  One routine for the host (plain mode) and the finishing kernel (guarded
// mode); beta^step by repeated squaring, so both evaluate the same IEEE products in the same order.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline double pow_int(double b, long long k) {
    double r = 1.0;
    while (k > 0) {
        if (k & 1) r *= b;
        b *= b;
        k >>= 1;
    }
    return r;
}

struct Bias { float bc1, sqrt_bc2, step_size; };
__host__ __device__ inline Bias bias_of(double lr, double beta1, double beta2, long long step) {
    const double bc1 = 1.0 - pow_int(beta1, step), bc2 = 1.0 - pow_int(beta2, step);
    Bias b;
    b.bc1 = (float)bc1;
    b.sqrt_bc2 = (float)sqrt(bc2);
    b.step_size = (float)(lr / bc1);
    return b;
}

// what a launch knows about its tensors and its one configuration: the kernel argument
struct Table {
    float* p[MAXT];
    const float* g[MAXT];
    long long off[MAXT];                 // first element of the tensor's moments in both arenas
    long long numel[MAXT];
    unsigned prefix[MAXT + 1];           // prefix[t] = chunks of the tensors before t
    float step_size[MAXT];               // plain: lr / bc1
    float sqrt_bc2[MAXT];                // plain
    int slot[MAXT];                      // guarded: row of tstate
    int n;
    int wd_mode;                         // 0: none, 1: L2, 2: decoupled
    float beta2, omb1, omb2, eps, wd, decay_mul;
    float *m, *v;
    const float* tstate;
    const unsigned* control;
    long long chunk_base;                // grad_partial_kernel: index of this launch's first partial
    void* partial;
    float p_min;                         // lazy_adam_kernel: the launch's clamp (-inf: none)
    int consume;                         // lazy_adam_kernel: 1: a touched gradient is overwritten with +0
};
static_assert(sizeof(Table) <= 4096, "the table travels as kernel arguments");

struct Consts { float beta2, omb1, omb2, eps, wd, decay_mul, step_size, sqrt_bc2, coef; int wd_mode; };

template <bool GUARDED>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const Consts& c) {
    // the fused multiply-adds are the ones PyTorch's CPU kernels take (add with alpha, lerp, addcmul): one rounding where the sum of two
    // rounded products has three -- over 20 steps of a four-element tensor the plain form was off by twice what PyTorch's fp32 Adam is
    if (GUARDED) g = g * c.coef;
    if (c.wd_mode == 1) g = fmaf(c.wd, p, g);
    else if (c.wd_mode == 2) p = p * c.decay_mul;
    m = fmaf(c.omb1, g - m, m);                                   // beta1 m + (1 - beta1) g as lerp(m, g, 1 - beta1)
    v = fmaf(c.omb2 * g, g, c.beta2 * v);
    const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
    p = p - (c.step_size * m) / denom;
}

// the tensor whose chunks hold block b: the largest t with prefix[t] <= b (a tensor without elements has no chunk and is never found)
__device__ __forceinline__ int find_tensor(const Table& a, unsigned b) {
    int lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.prefix[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <bool GUARDED>
__global__ __launch_bounds__(THREADS) void adam_kernel(const Table a) {
    const int tid = threadIdx.x;
    const int t = find_tensor(a, blockIdx.x);
    const long long c0 = (long long)(blockIdx.x - a.prefix[t]) * CHUNK;
    const long long left = a.numel[t] - c0;
    const int cnt = left < CHUNK ? (int)left : CHUNK;
    Consts c;
    c.beta2 = a.beta2; c.omb1 = a.omb1; c.omb2 = a.omb2; c.eps = a.eps; c.wd = a.wd; c.decay_mul = a.decay_mul;
    c.wd_mode = a.wd_mode;
    if (GUARDED) {
        if (a.control[3] != 0) return;                             // a skipped step writes nothing (the same word for every workgroup)
        c.coef = __uint_as_float(a.control[1]);
        const float* ts = a.tstate + (size_t)a.slot[t] * MI_OPTIM_TSTATE_WORDS;
        c.sqrt_bc2 = ts[2];
        c.step_size = ts[3];
    } else {
        c.coef = 1.0f;
        c.sqrt_bc2 = a.sqrt_bc2[t];
        c.step_size = a.step_size[t];
    }
    float* p = a.p[t] + c0;
    const float* g = a.g[t] + c0;
    float* m = a.m + a.off[t] + c0;
    float* v = a.v + a.off[t] + c0;
    // c0 is a multiple of 4096 elements: the chunk's addresses are aligned as the tensor's are
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
        float4 P[4], G[4], M[4], V[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = (i * THREADS + tid) * 4;
            if (e + 4 <= cnt) {
                P[i] = *reinterpret_cast<const float4*>(p + e);
                G[i] = *reinterpret_cast<const float4*>(g + e);
                M[i] = *reinterpret_cast<const float4*>(m + e);
                V[i] = *reinterpret_cast<const float4*>(v + e);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = (i * THREADS + tid) * 4;
            if (e + 4 <= cnt) {
                adam_elem<GUARDED>(P[i].x, G[i].x, M[i].x, V[i].x, c);
                adam_elem<GUARDED>(P[i].y, G[i].y, M[i].y, V[i].y, c);
                adam_elem<GUARDED>(P[i].z, G[i].z, M[i].z, V[i].z, c);
                adam_elem<GUARDED>(P[i].w, G[i].w, M[i].w, V[i].w, c);
                *reinterpret_cast<float4*>(p + e) = P[i];
                *reinterpret_cast<float4*>(m + e) = M[i];
                *reinterpret_cast<float4*>(v + e) = V[i];
            } else if (e < cnt) {                                  // the tensor's last one to three elements
                for (int k = e; k < cnt; ++k) {
                    float pk = p[k], mk = m[k], vk = v[k];
                    adam_elem<GUARDED>(pk, g[k], mk, vk, c);
                    p[k] = pk; m[k] = mk; v[k] = vk;
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float P[4], G[4], M[4], V[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (j * 4 + i) * THREADS + tid;
                if (e < cnt) { P[i] = p[e]; G[i] = g[e]; M[i] = m[e]; V[i] = v[e]; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (j * 4 + i) * THREADS + tid;
                if (e < cnt) {
                    adam_elem<GUARDED>(P[i], G[i], M[i], V[i], c);
                    p[e] = P[i]; m[e] = M[i]; v[e] = V[i];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// THE LAZY UPDATE
// ------------------------------------------------------------------------------------------------
// one touched element: THE UPDATE, then the clamp (a NaN compares false and stays)
__device__ __forceinline__ void lazy_elem(float& p, float g, float& m, float& v, const Consts& c, float p_min) {
    float pn = p, mn = m, vn = v;
    adam_elem<false>(pn, g, mn, vn, c);
    pn = pn < p_min ? p_min : pn;
    const bool touched = g != 0.0f;                               // -0.0 is untouched, NaN is touched
    p = touched ? pn : p;                                         // selects: an untouched component of a touched piece is stored back
    m = touched ? mn : m;                                         // with the bits that were loaded
    v = touched ? vn : v;
}

__device__ __forceinline__ bool any_touched(const float4& g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f || g.w != 0.0f; }

__global__ __launch_bounds__(THREADS) void lazy_adam_kernel(const Table a) {
    const int tid = threadIdx.x;
    const int t = find_tensor(a, blockIdx.x);
    const long long c0 = (long long)(blockIdx.x - a.prefix[t]) * CHUNK;
    const long long left = a.numel[t] - c0;
    const int cnt = left < CHUNK ? (int)left : CHUNK;
    Consts c;
    c.beta2 = a.beta2; c.omb1 = a.omb1; c.omb2 = a.omb2; c.eps = a.eps; c.wd = 0.0f; c.decay_mul = 1.0f;
    c.wd_mode = 0;
    c.coef = 1.0f;
    c.sqrt_bc2 = a.sqrt_bc2[t];
    c.step_size = a.step_size[t];
    const float p_min = a.p_min;
    const bool consume = a.consume != 0;
    float* p = a.p[t] + c0;
    float* g = const_cast<float*>(a.g[t]) + c0;                    // the lazy entry takes its gradients writable
    float* m = a.m + a.off[t] + c0;
    float* v = a.v + a.off[t] + c0;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
        float4 G[4];
        bool hit[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                              // every gradient load first: the untouched chunk ends after them
            const int e = (i * THREADS + tid) * 4;
            G[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (e + 4 <= cnt) G[i] = *reinterpret_cast<const float4*>(g + e);
            hit[i] = any_touched(G[i]);
        }
        float4 P[4], M[4], V[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = (i * THREADS + tid) * 4;
            if (hit[i]) {
                P[i] = *reinterpret_cast<const float4*>(p + e);
                M[i] = *reinterpret_cast<const float4*>(m + e);
                V[i] = *reinterpret_cast<const float4*>(v + e);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = (i * THREADS + tid) * 4;
            if (hit[i]) {
                lazy_elem(P[i].x, G[i].x, M[i].x, V[i].x, c, p_min);
                lazy_elem(P[i].y, G[i].y, M[i].y, V[i].y, c, p_min);
                lazy_elem(P[i].z, G[i].z, M[i].z, V[i].z, c, p_min);
                lazy_elem(P[i].w, G[i].w, M[i].w, V[i].w, c, p_min);
                *reinterpret_cast<float4*>(p + e) = P[i];
                *reinterpret_cast<float4*>(m + e) = M[i];
                *reinterpret_cast<float4*>(v + e) = V[i];
                if (consume) *reinterpret_cast<float4*>(g + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else if (e < cnt && e + 4 > cnt) {                   // the tensor's last one to three elements
                for (int k = e; k < cnt; ++k) {
                    const float gk = g[k];
                    if (gk != 0.0f) {
                        float pk = p[k], mk = m[k], vk = v[k];
                        lazy_elem(pk, gk, mk, vk, c, p_min);
                        p[k] = pk; m[k] = mk; v[k] = vk;
                        if (consume) g[k] = 0.0f;
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float G[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (j * 4 + i) * THREADS + tid;
                G[i] = e < cnt ? g[e] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (j * 4 + i) * THREADS + tid;
                if (G[i] != 0.0f) {
                    float pe = p[e], me = m[e], ve = v[e];
                    lazy_elem(pe, G[i], me, ve, c, p_min);
                    p[e] = pe; m[e] = me; v[e] = ve;
                    if (consume) g[e] = 0.0f;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// mi_optim_grad_stats
// ------------------------------------------------------------------------------------------------
struct Partial { double sumsq; unsigned long long bad; };
static_assert(sizeof(Partial) == 16, "one 16-byte partial per workgroup");

__device__ __forceinline__ void stat_elem(float g, double& s, unsigned& bad) {
    s += (double)g * (double)g;
    bad += (__float_as_uint(g) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
}

__global__ __launch_bounds__(THREADS) void grad_partial_kernel(const Table a) {
    __shared__ double red_s[THREADS / 64];
    __shared__ unsigned red_b[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = find_tensor(a, blockIdx.x);
    const long long c0 = (long long)(blockIdx.x - a.prefix[t]) * CHUNK;
    const long long left = a.numel[t] - c0;
    const int cnt = left < CHUNK ? (int)left : CHUNK;
    const float* g = a.g[t] + c0;
    double s = 0.0;
    unsigned bad = 0;
    if (aligned16(g)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = (i * THREADS + tid) * 4;
            if (e + 4 <= cnt) {
                const float4 G = *reinterpret_cast<const float4*>(g + e);
                stat_elem(G.x, s, bad); stat_elem(G.y, s, bad); stat_elem(G.z, s, bad); stat_elem(G.w, s, bad);
            } else if (e < cnt) {
                for (int k = e; k < cnt; ++k) stat_elem(g[k], s, bad);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const int e = i * THREADS + tid;
            if (e < cnt) stat_elem(g[e], s, bad);
        }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        s += __shfl_xor(s, msk, 64);
        bad += __shfl_xor(bad, msk, 64);
    }
    if (lane == 0) { red_s[wave] = s; red_b[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
        Partial out;
        out.sumsq = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        out.bad = (unsigned long long)red_b[0] + red_b[1] + red_b[2] + red_b[3];
        reinterpret_cast<Partial*>(a.partial)[a.chunk_base + blockIdx.x] = out;
    }
}

struct FinishArgs {
    const Partial* partial;
    long long nparts;
    int first;                           // 1: this launch adds the partials and writes the control block; 0: it reads the skip word
    int skip_nonfinite;
    float max_norm;
    unsigned* control;
    float* tstate;
    int n;
    int slot[MAXT];
    double lr, beta1, beta2;
};
static_assert(sizeof(FinishArgs) <= 4096, "the table travels as kernel arguments");

__global__ __launch_bounds__(THREADS) void grad_finish_kernel(const FinishArgs a) {
    __shared__ double red_s[THREADS];
    __shared__ unsigned long long red_b[THREADS];
    __shared__ unsigned skip_word;
    const int tid = threadIdx.x;
    if (a.first) {
        const long long per = (a.nparts + THREADS - 1) / THREADS;
        const long long lo = tid * per, hi = lo + per < a.nparts ? lo + per : a.nparts;
        double s = 0.0;
        unsigned long long bad = 0;
        for (long long i = lo; i < hi; ++i) { s += a.partial[i].sumsq; bad += a.partial[i].bad; }
        red_s[tid] = s;
        red_b[tid] = bad;
        __syncthreads();
        for (int w = THREADS / 2; w >= 1; w >>= 1) {
            if (tid < w) { red_s[tid] += red_s[tid + w]; red_b[tid] += red_b[tid + w]; }
            __syncthreads();
        }
        if (tid == 0) {
            const double norm = sqrt(red_s[0]);
            const unsigned long long nbad = red_b[0];
            double coef = 1.0;
            if (!isinf(a.max_norm)) {                              // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1), NaN stays NaN
                const double ratio = (double)a.max_norm / (norm + 1e-6);
                coef = ratio > 1.0 ? 1.0 : ratio;
            }
            const unsigned skip = (a.skip_nonfinite && nbad != 0) ? 1u : 0u;
            a.control[0] = __float_as_uint((float)norm);
            a.control[1] = __float_as_uint((float)coef);
            a.control[2] = nbad > 0xffffffffull ? 0xffffffffu : (unsigned)nbad;
            a.control[3] = skip;
            a.control[4] = a.control[4] + skip;
            a.control[5] = 0; a.control[6] = 0; a.control[7] = 0;
            skip_word = skip;
        }
    } else if (tid == 0) {
        skip_word = a.control[3];                                  // left by the first finishing launch, earlier on this stream
    }
    __syncthreads();
    if (tid < a.n && skip_word == 0) {
        float* ts = a.tstate + (size_t)a.slot[tid] * MI_OPTIM_TSTATE_WORDS;
        const float step = ts[0] + 1.0f;
        const Bias b = bias_of(a.lr, a.beta1, a.beta2, (long long)step);
        ts[0] = step; ts[1] = b.bc1; ts[2] = b.sqrt_bc2; ts[3] = b.step_size;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: checks, batches, launches
// ------------------------------------------------------------------------------------------------
static inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline long long chunks_of(long long numel) { return (numel + CHUNK - 1) / CHUNK; }

// what every entry checks of THE TENSOR LIST (params / state_off / slot: NULL when the entry does not take them)
static int check_list(const char* who, int n, float* const* params, bool with_params, const float* const* grads, const int64_t* numel,
                      const int64_t* state_off, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg, const int32_t* cfg_of,
                      const int32_t* slot, bool with_slot, int n_slots) {
    OPTIM_CHECK_ARG(n > 0, "%s: n=%d must be positive", who, n);
    OPTIM_CHECK_ARG(grads && numel && (!with_params || (params && state_off)), "%s: NULL tensor array", who);
    OPTIM_CHECK_ARG(cfgs && n_cfg > 0, "%s: no configuration (cfgs=%p, n_cfg=%d)", who, (const void*)cfgs, n_cfg);
    OPTIM_CHECK_ARG(!with_slot || (slot && n_slots > 0), "%s: NULL slot array or n_slots=%d", who, n_slots);
    for (int k = 0; k < n_cfg; ++k) {
        const mi_optim_adam_cfg& c = cfgs[k];
        OPTIM_CHECK_ARG(c.size == sizeof(mi_optim_adam_cfg), "%s: cfgs[%d].size=%u is not sizeof(mi_optim_adam_cfg)=%zu", who, k, c.size,
                        sizeof(mi_optim_adam_cfg));
        OPTIM_CHECK_ARG(isfinite(c.lr) && c.lr >= 0.0, "%s: cfgs[%d].lr=%g must be finite and not negative", who, k, c.lr);
        OPTIM_CHECK_ARG(isfinite(c.eps) && c.eps >= 0.0, "%s: cfgs[%d].eps=%g must be finite and not negative", who, k, c.eps);
        OPTIM_CHECK_ARG(isfinite(c.weight_decay) && c.weight_decay >= 0.0, "%s: cfgs[%d].weight_decay=%g must be finite and not negative", who, k,
                        c.weight_decay);
        OPTIM_CHECK_ARG(c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0, "%s: cfgs[%d] betas (%g, %g) must lie in [0, 1)", who, k,
                        c.beta1, c.beta2);
        OPTIM_CHECK_ARG(c.decoupled == 0 || c.decoupled == 1, "%s: cfgs[%d].decoupled=%d must be 0 or 1", who, k, c.decoupled);
    }
    for (int i = 0; i < n; ++i) {
        OPTIM_CHECK_ARG(numel[i] >= 0 && numel[i] <= ((int64_t)1 << 40), "%s: numel[%d]=%lld: 0 .. 2^40", who, i, (long long)numel[i]);
        OPTIM_CHECK_ARG(grads[i] != nullptr || numel[i] == 0, "%s: grads[%d] is NULL", who, i);
        OPTIM_CHECK_ARG(aligned(grads[i], 4), "%s: grads[%d] is not 4-byte aligned", who, i);
        OPTIM_CHECK_ARG(!cfg_of || (cfg_of[i] >= 0 && cfg_of[i] < n_cfg), "%s: cfg_of[%d]=%d outside [0, %d)", who, i, cfg_of ? cfg_of[i] : 0, n_cfg);
        if (with_params) {
            OPTIM_CHECK_ARG(params[i] != nullptr || numel[i] == 0, "%s: params[%d] is NULL", who, i);
            OPTIM_CHECK_ARG(aligned(params[i], 4), "%s: params[%d] is not 4-byte aligned", who, i);
            OPTIM_CHECK_ARG(state_off[i] >= 0 && state_off[i] <= state_numel - numel[i], "%s: tensor %d: moments [%lld, +%lld) outside the arenas of %lld",
                            who, i, (long long)state_off[i], (long long)numel[i], (long long)state_numel);
        }
        OPTIM_CHECK_ARG(!with_slot || (slot[i] >= 0 && slot[i] < n_slots), "%s: slot[%d]=%d outside [0, %d)", who, i, with_slot ? slot[i] : 0, n_slots);
    }
    return MI_OPTIM_OK;
}

// the launch that starts at tensor lo: consecutive tensors of one configuration (and, lazy, of one p_min: compared as bits, a NaN was
// refused), at most MAXT, at most 2^31 - 1 chunks
static inline uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static int batch_end(int lo, int n, const int64_t* numel, const int32_t* cfg_of, const float* p_min = nullptr) {
    long long chunks = 0;
    int hi = lo;
    while (hi < n && hi - lo < MAXT && (!cfg_of || cfg_of[hi] == cfg_of[lo]) && (!p_min || float_bits(p_min[hi]) == float_bits(p_min[lo])) &&
           chunks + chunks_of(numel[hi]) <= 0x7fffffffLL)
        chunks += chunks_of(numel[hi++]);
    return hi > lo ? hi : lo + 1;        // (one tensor alone never exceeds the bound: numel <= 2^40 is 2^28 chunks)
}

// tensors [lo, hi) -> the table's sizes and prefix; the number of chunks
static long long fill_shape(Table& t, int lo, int hi, const float* const* grads, const int64_t* numel) {
    t.n = hi - lo;
    t.prefix[0] = 0;
    for (int i = lo; i < hi; ++i) {
        t.g[i - lo] = grads[i];
        t.numel[i - lo] = numel[i];
        t.prefix[i - lo + 1] = t.prefix[i - lo] + (unsigned)chunks_of(numel[i]);
    }
    return t.prefix[t.n];
}

static void fill_cfg(Table& t, const mi_optim_adam_cfg& c) {
    t.wd_mode = c.weight_decay == 0.0 ? 0 : c.decoupled ? 2 : 1;
    t.beta2 = (float)c.beta2;
    t.omb1 = (float)(1.0 - c.beta1); t.omb2 = (float)(1.0 - c.beta2);
    t.eps = (float)c.eps; t.wd = (float)c.weight_decay;
    t.decay_mul = (float)(1.0 - c.lr * c.weight_decay);
}

enum StepKind { PLAIN, GUARDED, LAZY };

static int step_launches(StepKind kind, int n, float* const* params, const float* const* grads, const int64_t* numel, const int64_t* state_off,
                         const int64_t* step, float* exp_avg, float* exp_avg_sq, const mi_optim_adam_cfg* cfgs, const int32_t* cfg_of,
                         const int32_t* slot, const float* tstate, const void* control, const float* p_min, int consume, hipStream_t st) {
    const bool guarded = kind == GUARDED;
    for (int lo = 0; lo < n;) {
        const int hi = batch_end(lo, n, numel, cfg_of, kind == LAZY ? p_min : nullptr);
        const mi_optim_adam_cfg& c = cfgs[cfg_of ? cfg_of[lo] : 0];
        Table t{};
        const long long chunks = fill_shape(t, lo, hi, grads, numel);
        fill_cfg(t, c);
        t.m = exp_avg; t.v = exp_avg_sq; t.tstate = tstate; t.control = (const unsigned*)control;
        t.p_min = p_min ? p_min[lo] : -INFINITY;
        t.consume = consume;
        for (int i = lo; i < hi; ++i) {
            t.p[i - lo] = params[i];
            t.off[i - lo] = state_off[i];
            if (guarded) {
                t.slot[i - lo] = slot[i];
            } else {
                const Bias b = bias_of(c.lr, c.beta1, c.beta2, step[i]);
                t.step_size[i - lo] = b.step_size;
                t.sqrt_bc2[i - lo] = b.sqrt_bc2;
            }
        }
        if (chunks > 0) {
            if (kind == LAZY) hipLaunchKernelGGL(lazy_adam_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, st, t);
            else if (guarded) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)chunks), dim3(THREADS), 0, st, t);
            else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)chunks), dim3(THREADS), 0, st, t);
            OPTIM_LAUNCH_CHECK("adam_kernel");
        }
        lo = hi;
    }
    return MI_OPTIM_OK;
}

}  // namespace mioptim

using namespace mioptim;

extern "C" {

int mi_optim_abi_version(void) { return MI_OPTIM_ABI_VERSION; }
const char* mi_optim_last_error(void) { return g_err; }

int mi_optim_adam_step(int n, float* const* params, const float* const* grads, const int64_t* numel, const int64_t* state_off,
                       const int64_t* step, float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                       const int32_t* cfg_of, void* stream) {
    const char* who = "mi_optim_adam_step";
    OPTIM_CHECK_ARG(exp_avg && exp_avg_sq && aligned(exp_avg, 4) && aligned(exp_avg_sq, 4) && state_numel >= 0, "%s: the state arenas must be given, 4-byte aligned", who);
    if (int rc = check_list(who, n, params, true, grads, numel, state_off, state_numel, cfgs, n_cfg, cfg_of, nullptr, false, 0)) return rc;
    OPTIM_CHECK_ARG(step != nullptr, "%s: step is NULL", who);
    for (int i = 0; i < n; ++i)
        OPTIM_CHECK_ARG(step[i] >= 1 && step[i] <= ((int64_t)1 << 53), "%s: step[%d]=%lld: the step being taken is at least 1", who, i, (long long)step[i]);
    return step_launches(PLAIN, n, params, grads, numel, state_off, step, exp_avg, exp_avg_sq, cfgs, cfg_of, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
}

int mi_optim_adam_step_lazy(int n, float* const* params, float* const* grads, const int64_t* numel, const int64_t* state_off,
                            const int64_t* step, float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                            const int32_t* cfg_of, const float* p_min, int consume, void* stream) {
    const char* who = "mi_optim_adam_step_lazy";
    OPTIM_CHECK_ARG(exp_avg && exp_avg_sq && aligned(exp_avg, 4) && aligned(exp_avg_sq, 4) && state_numel >= 0, "%s: the state arenas must be given, 4-byte aligned", who);
    if (int rc = check_list(who, n, params, true, grads, numel, state_off, state_numel, cfgs, n_cfg, cfg_of, nullptr, false, 0)) return rc;
    OPTIM_CHECK_ARG(step != nullptr, "%s: step is NULL", who);
    for (int i = 0; i < n; ++i)
        OPTIM_CHECK_ARG(step[i] >= 1 && step[i] <= ((int64_t)1 << 53), "%s: step[%d]=%lld: the step being taken is at least 1", who, i, (long long)step[i]);
    for (int k = 0; k < n_cfg; ++k)
        OPTIM_CHECK_ARG(cfgs[k].weight_decay == 0.0, "%s: cfgs[%d].weight_decay=%g: a lazy weight decay is not defined, it must be 0", who, k, cfgs[k].weight_decay);
    OPTIM_CHECK_ARG(consume == 0 || consume == 1, "%s: consume=%d must be 0 or 1", who, consume);
    for (int i = 0; p_min && i < n; ++i)
        OPTIM_CHECK_ARG(!isnan(p_min[i]), "%s: p_min[%d] is NaN (-inf: no clamp)", who, i);
    return step_launches(LAZY, n, params, grads, numel, state_off, step, exp_avg, exp_avg_sq, cfgs, cfg_of, nullptr, nullptr, nullptr, p_min, consume, (hipStream_t)stream);
}

size_t mi_optim_grad_stats_scratch_bytes(int n, const int64_t* numel) {
    if (n <= 0 || !numel) return 0;
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0 || numel[i] > ((int64_t)1 << 40)) return 0;
        chunks += chunks_of(numel[i]);
    }
    return (size_t)(chunks > 0 ? chunks : 1) * sizeof(Partial);
}

int mi_optim_grad_stats(int n, const float* const* grads, const int64_t* numel, const mi_optim_adam_cfg* cfgs, int n_cfg, const int32_t* cfg_of,
                        const int32_t* slot, int n_slots, float max_norm, int skip_nonfinite, float* tstate, void* control, void* scratch,
                        size_t scratch_bytes, void* stream) {
    const char* who = "mi_optim_grad_stats";
    if (int rc = check_list(who, n, nullptr, false, grads, numel, nullptr, 0, cfgs, n_cfg, cfg_of, slot, true, n_slots)) return rc;
    OPTIM_CHECK_ARG(max_norm > 0.0f, "%s: max_norm=%g must be positive (+inf: no clipping)", who, (double)max_norm);
    OPTIM_CHECK_ARG(skip_nonfinite == 0 || skip_nonfinite == 1, "%s: skip_nonfinite=%d must be 0 or 1", who, skip_nonfinite);
    OPTIM_CHECK_ARG(tstate && control && aligned(tstate, 16) && aligned(control, 16), "%s: tstate and control must be given, 16-byte aligned", who);
    const size_t need = mi_optim_grad_stats_scratch_bytes(n, numel);
    OPTIM_CHECK_ARG(scratch && aligned(scratch, 16) && scratch_bytes >= need, "%s: scratch must be 16-byte aligned and hold %zu bytes (got %zu)", who, need,
                    scratch_bytes);
    hipStream_t st = (hipStream_t)stream;
    long long base = 0;
    for (int lo = 0; lo < n;) {
        const int hi = batch_end(lo, n, numel, cfg_of);
        Table t{};
        const long long chunks = fill_shape(t, lo, hi, grads, numel);
        t.chunk_base = base;
        t.partial = scratch;
        if (chunks > 0) {
            hipLaunchKernelGGL(grad_partial_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, st, t);
            OPTIM_LAUNCH_CHECK("grad_partial_kernel");
        }
        base += chunks;
        lo = hi;
    }
    for (int lo = 0; lo < n;) {
        const int hi = batch_end(lo, n, numel, cfg_of);
        const mi_optim_adam_cfg& c = cfgs[cfg_of ? cfg_of[lo] : 0];
        FinishArgs f{};
        f.partial = (const Partial*)scratch; f.nparts = base; f.first = lo == 0; f.skip_nonfinite = skip_nonfinite; f.max_norm = max_norm;
        f.control = (unsigned*)control; f.tstate = tstate; f.n = hi - lo;
        f.lr = c.lr; f.beta1 = c.beta1; f.beta2 = c.beta2;
        for (int i = lo; i < hi; ++i) f.slot[i - lo] = slot[i];
        hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(THREADS), 0, st, f);
        OPTIM_LAUNCH_CHECK("grad_finish_kernel");
        lo = hi;
    }
    return MI_OPTIM_OK;
}

int mi_optim_adam_step_guarded(int n, float* const* params, const float* const* grads, const int64_t* numel, const int64_t* state_off,
                               float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                               const int32_t* cfg_of, const int32_t* slot, int n_slots, const float* tstate, const void* control, void* stream) {
    const char* who = "mi_optim_adam_step_guarded";
    OPTIM_CHECK_ARG(exp_avg && exp_avg_sq && aligned(exp_avg, 4) && aligned(exp_avg_sq, 4) && state_numel >= 0, "%s: the state arenas must be given, 4-byte aligned", who);
    if (int rc = check_list(who, n, params, true, grads, numel, state_off, state_numel, cfgs, n_cfg, cfg_of, slot, true, n_slots)) return rc;
    OPTIM_CHECK_ARG(tstate && control && aligned(tstate, 16) && aligned(control, 16), "%s: tstate and control must be given, 16-byte aligned", who);
    return step_launches(GUARDED, n, params, grads, numel, state_off, nullptr, exp_avg, exp_avg_sq, cfgs, cfg_of, slot, tstate, control, nullptr, 0, (hipStream_t)stream);
}

}  // extern "C"
