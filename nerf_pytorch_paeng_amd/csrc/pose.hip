// pose.hip -- libmi_nerf_pose.so (include/mi_nerf_pose.h): gradients of the training path with respect to rays and camera poses.  A library
// of its own: it shares common.h / stage_dev.h with libmi_nerf.so at compile time (the sin / cos of the forward's positional encoding, so
// that the backward differentiates the numbers the forward produced; wave_sum) and nothing at link time.
//
//   input_grad_kernel<W>        one 64-lane wavefront per ray.  Per 32-sample tile: [32 points][64 + 32 columns] = delta rows x the three
//                               narrow weight blocks on v_mfma_f32_32x32x2_f32 (weights staged once per workgroup in LDS, delta rows read
//                               straight from HBM, 64 contiguous bytes per lane); the accumulator tile has a gamma channel on the lane and the
//                               points in the registers, so the positional-encoding backward is one coefficient per (lane, point) and the
//                               per-ray sums stay in the lane until the ray ends.  g_gamma never goes to HBM unless d_emb is asked for.
//   ndc_bwd_kernel              closed-form backward of ndc_kernel (stages.hip), one thread per ray
//   o_d_partial_kernel / o_d_final_kernel   the sixteen sums of the make_o_d backward: block partials in fixed order, then one block
//
// No atomic, no host synchronisation, no allocation.  Compiled with -ffp-contract=off like stages.hip: x = o + z d is the forward's x.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_pose.h"
#include "abi_error.h"
#include "common.h"
#include "stage_dev.h"

namespace mipose {

using minerf::f32x16;
using minerf::f32x4;
using minerf::SINCOS_FAST_LIMIT;
using minerf::sin_cos_fast;
using minerf::sin_cos_slow;
using minerf::wave_sum;

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_POSE_EHIP)
#define POSE_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::mipose, MI_POSE_EINVAL, cond, __VA_ARGS__)
#define POSE_HIP(call) ABI_HIP(::mipose, call, #call)
#define POSE_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::mipose, name)

// sum over the 32 lanes of this lane's half of the wave
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------
// mi_pose_input_grad
// ------------------------------------------------------------------------------------------------
struct InputGradArgs {
    const float *rays, *z, *raw, *d_raw;
    long long n;
    int S, L_x, L_d;
    const float *delta_x0, *delta_skip, *delta_d;
    const float *w_x0, *w_skip, *w_d;
    int ld_x0, ld_skip, ld_d;
    float *d_rays, *d_pts, *d_view, *d_emb;
};

// One column of gamma (PositionalEncoding.py:18-30): which component of the 3-vector it encodes, its frequency, and what it is.
enum { CH_ID = 0, CH_SIN = 1, CH_COS = 2, CH_NONE = 3 };
struct Chan { int axis, kind; float freq; };
__device__ __forceinline__ Chan channel(int c, int in) {
    Chan ch;
    if (c >= in) { ch.axis = 0; ch.kind = CH_NONE; ch.freq = 0.0f; return ch; }
    if (c < 3) { ch.axis = c; ch.kind = CH_ID; ch.freq = 1.0f; return ch; }
    const int q = c - 3;
    ch.axis = q % 3;
    ch.kind = ((q / 3) & 1) ? CH_COS : CH_SIN;
    ch.freq = (float)(1 << (q / 6));
    return ch;
}
// d gamma_channel / d component at component value b:  1,  2^k cos(2^k b),  -2^k sin(2^k b)
__device__ __forceinline__ float channel_slope(const Chan& ch, float b) {
    if (ch.kind == CH_ID) return 1.0f;
    if (ch.kind == CH_NONE) return 0.0f;
    const float y = b * ch.freq;
    const int shift = ch.kind == CH_SIN ? 1 : 0;                        // sin channel: cos(y);  cos channel: -sin(y)
    const float t = (__builtin_fabsf(y) < SINCOS_FAST_LIMIT) ? sin_cos_fast(y, shift) : sin_cos_slow(y, shift);
    return ch.kind == CH_SIN ? ch.freq * t : -(ch.freq * t);
}
__device__ __forceinline__ float pick3(int axis, float a, float b, float c) { return axis == 0 ? a : axis == 1 ? b : c; }

// acc (+)= delta[32 points of the tile][K] x wl[K][NB * 32] for this wave.  Lane (col, hh) reads 16 consecutive floats of its point's row per
// step of 32 k: k = kb + 16 hh + j is the MFMA's k index hh at sub-step j, on both operands.
template <int K, int NB>
__device__ __forceinline__ void tile_product(const float* __restrict__ drow, const float* __restrict__ wl, int col, int hh, f32x16 (&acc)[NB]) {
    constexpr int LDW = NB * 32;
    const float* dp = drow + 16 * hh;
    f32x4 nx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) nx[q] = *(const f32x4*)(dp + 4 * q);
#pragma unroll 1
    for (int kb = 0; kb < K; kb += 32) {
        f32x4 cur[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = nx[q];
        if (kb + 32 < K) {
#pragma unroll
            for (int q = 0; q < 4; ++q) nx[q] = *(const f32x4*)(dp + kb + 32 + 4 * q);
        }
        const float* wk = wl + (size_t)(kb + 16 * hh) * LDW + col;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float av = cur[j >> 2][j & 3];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wk[j * LDW + 32 * b], acc[b], 0, 0, 0);
        }
    }
}

template <int W>
__global__ __launch_bounds__(256) void input_grad_kernel(const InputGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, hh = lane >> 5;
    const int in_x = 3 + 6 * a.L_x, in_d = 3 + 6 * a.L_d, in_all = in_x + in_d;
    const int nsrc = a.delta_skip ? 2 : 1;
    float* wx = lds;                                      // [nsrc * W][64]: Wx0, then Wskip[:, :in_x]; columns beyond in_x are zero
    float* wd = lds + (size_t)nsrc * W * 64;              // [W / 2][32]:    Wd[:, W : W + in_d];      columns beyond in_d are zero
    for (int i = tid; i < W * 64; i += 256) {
        const int k = i >> 6, c = i & 63;
        wx[i] = c < in_x ? a.w_x0[(size_t)k * a.ld_x0 + c] : 0.0f;
        if (nsrc == 2) wx[W * 64 + i] = c < in_x ? a.w_skip[(size_t)k * a.ld_skip + c] : 0.0f;
    }
    for (int i = tid; i < (W / 2) * 32; i += 256) {
        const int k = i >> 5, c = i & 31;
        wd[i] = c < in_d ? a.w_d[(size_t)k * a.ld_d + W + c] : 0.0f;
    }
    __syncthreads();

    const Chan c0 = channel(col, in_x), c1 = channel(col + 32, in_x), cd = channel(col, in_d);
    const int S = a.S, tpr = (S + 31) / 32;

    for (long long ray = (long long)blockIdx.x * 4 + wave; ray < a.n; ray += (long long)gridDim.x * 4) {
        const float* rp = a.rays + ray * 6;
        const float ox = rp[0], oy = rp[1], oz = rp[2], dx = rp[3], dy = rp[4], dz = rp[5];
        const float nrm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);          // nerf_process.py:39
        const float vx = dx / nrm, vy = dy / nrm, vz = dz / nrm;
        const float o0 = pick3(c0.axis, ox, oy, oz), d0 = pick3(c0.axis, dx, dy, dz);
        const float o1 = pick3(c1.axis, ox, oy, oz), d1 = pick3(c1.axis, dx, dy, dz);
        const float* zr = a.z + ray * S;
        float so0 = 0.0f, sz0 = 0.0f, so1 = 0.0f, sz1 = 0.0f, sv = 0.0f;      // this lane's column(s), summed over the ray's samples

        for (int t = 0; t < tpr; ++t) {
            const int s0 = t * 32;
            const int sa = (s0 + col < S) ? s0 + col : S - 1;                    // rows beyond S recompute the last sample and are masked below
            const long long pa = ray * S + sa;
            f32x16 ax[2], ad[1];
#pragma unroll
            for (int r = 0; r < 16; ++r) { ax[0][r] = 0.0f; ax[1][r] = 0.0f; ad[0][r] = 0.0f; }
            tile_product<W, 2>(a.delta_x0 + (size_t)pa * W, wx, col, hh, ax);
            if (nsrc == 2) tile_product<W, 2>(a.delta_skip + (size_t)pa * W, wx + W * 64, col, hh, ax);
            tile_product<W / 2, 1>(a.delta_d + (size_t)pa * (W / 2), wd, col, hh, ad);

            const float zl = zr[sa];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;                 // C/D map of the 32x32 MFMA: column on the lane
                const float zv = __shfl(zl, row, 64);
                const bool valid = s0 + row < S;
                const float t0 = valid ? ax[0][r] * channel_slope(c0, o0 + d0 * zv) : 0.0f;
                const float t1 = valid ? ax[1][r] * channel_slope(c1, o1 + d1 * zv) : 0.0f;
                so0 += t0; sz0 += zv * t0;
                so1 += t1; sz1 += zv * t1;
                sv += valid ? ad[0][r] : 0.0f;
                const long long p = ray * S + s0 + row;
                if (a.d_emb && valid) {                                          // wave-uniform pointer test
                    float* e = a.d_emb + (size_t)p * in_all;
                    if (c0.kind != CH_NONE) e[col] = ax[0][r];
                    if (c1.kind != CH_NONE) e[col + 32] = ax[1][r];
                    if (cd.kind != CH_NONE) e[in_x + col] = ad[0][r];
                }
                if (a.d_pts) {                                                   // g_x of the point: the columns of one component, summed across the half
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float g = half_sum((c0.axis == c ? t0 : 0.0f) + (c1.axis == c ? t1 : 0.0f));
                        if (col == 0 && valid) a.d_pts[(size_t)p * 3 + c] = g;
                    }
                }
            }
        }

        // the view direction is one value per ray: its slopes leave the sample sum
        const float gv = sv * channel_slope(cd, pick3(cd.axis, vx, vy, vz));
        float Go[3], Gz[3], Gv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Go[c] = wave_sum((c0.axis == c ? so0 : 0.0f) + (c1.axis == c ? so1 : 0.0f));
            Gz[c] = wave_sum((c0.axis == c ? sz0 : 0.0f) + (c1.axis == c ? sz1 : 0.0f));
            Gv[c] = wave_sum(cd.axis == c ? gv : 0.0f);
        }
        // the |d| of dist_i = (z_{i+1} - z_i) |d|:  sum_s d_raw[s][3] relu(raw[s][3]), lane-strided, then across the wave
        float sg = 0.0f;
        for (int s = lane; s < S; s += 64) {
            const size_t q = ((size_t)(ray * S + s)) * 4 + 3;
            sg += a.d_raw[q] * __builtin_fmaxf(a.raw[q], 0.0f);
        }
        sg = wave_sum(sg);
        if (lane == 0) {
            const float vg = vx * Gv[0] + vy * Gv[1] + vz * Gv[2];
            const float v[3] = {vx, vy, vz};
            float* out = a.d_rays + ray * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out[c] = Go[c];
                out[3 + c] = Gz[c] + (Gv[c] - v[c] * vg) / nrm + v[c] * (sg / nrm);
            }
            if (a.d_view) { a.d_view[ray * 3 + 0] = Gv[0]; a.d_view[ray * 3 + 1] = Gv[1]; a.d_view[ray * 3 + 2] = Gv[2]; }
        }
    }
}

static size_t input_grad_lds_bytes(int W, bool skip) { return ((size_t)(skip ? 2 : 1) * W * 64 + (size_t)(W / 2) * 32) * sizeof(float); }

template <int W>
static int launch_input_grad(const InputGradArgs& a, hipStream_t st) {
    const size_t lds = input_grad_lds_bytes(W, a.delta_skip != nullptr);
    auto kern = input_grad_kernel<W>;
    POSE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int dev = 0, cus = 0;
    POSE_HIP(hipGetDevice(&dev));
    POSE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // every ray belongs to one wave whatever the grid: its size changes the speed, never a bit of the result
    long long grid = (a.n + 3) / 4;
    const long long resident = (long long)(cus > 0 ? cus : 1) * (lds <= 80 * 1024 ? 2 : 1);
    if (grid > resident) grid = resident;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, st, a);
    POSE_LAUNCH_CHECK("input_grad_kernel");
    return MI_POSE_OK;
}

// ------------------------------------------------------------------------------------------------
// mi_pose_ndc_rays_backward.  Forward (ndc_kernel, stages.hip):
//     t = -(near + o_z) / d_z;  p = o + t d;  O = (sx p_x / p_z, sy p_y / p_z, 1 + 2 near / p_z);  D = (sx (d_x / d_z - p_x / p_z), sy (..y..), -2 near / p_z)
// p_z = -near for every ray (d p_z / d o_z = 1 + d_z dt/do_z = 0, d p_z / d d_z = t + d_z dt/dd_z = 0): nothing flows through p_z, and O_z, D_z
// carry no gradient.  With a = dL/dp_x = sx (gO_x - gD_x) / p_z, b = dL/dp_y likewise and g_t = a d_x + b d_y:
//     g_o = (a, b, -g_t / d_z)
//     g_d = (t a + sx gD_x / d_z,  t b + sy gD_y / d_z,  -t g_t / d_z - (sx gD_x d_x + sy gD_y d_y) / d_z^2)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ndc_bwd_kernel(float sx, float sy, float near_, const float* __restrict__ oin, long long os,
                                                       const float* __restrict__ din, long long ds, long long n, const float* __restrict__ go_ndc,
                                                       const float* __restrict__ gd_ndc, float* __restrict__ go, float* __restrict__ gd) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float oz = oin[i * os + 2];
    const float dx = din[i * ds + 0], dy = din[i * ds + 1], dz = din[i * ds + 2];
    const float t = -(near_ + oz) / dz;
    const float pz = oz + t * dz;
    const float gOx = go_ndc ? go_ndc[3 * i + 0] : 0.0f, gOy = go_ndc ? go_ndc[3 * i + 1] : 0.0f;
    const float gDx = gd_ndc ? gd_ndc[3 * i + 0] : 0.0f, gDy = gd_ndc ? gd_ndc[3 * i + 1] : 0.0f;
    const float a = sx * (gOx - gDx) / pz, b = sy * (gOy - gDy) / pz;
    const float gt = a * dx + b * dy;
    const float ex = sx * gDx / dz, ey = sy * gDy / dz;
    go[3 * i + 0] = a;
    go[3 * i + 1] = b;
    go[3 * i + 2] = -gt / dz;
    gd[3 * i + 0] = t * a + ex;
    gd[3 * i + 1] = t * b + ey;
    gd[3 * i + 2] = -(t * gt) / dz - (ex * dx + ey * dy) / dz;
}

// ------------------------------------------------------------------------------------------------
// mi_pose_make_o_d_backward: sixteen sums over the pixels
//     [0..8] d_R[a][b] = sum g_d[a] dirs[b]     [9..11] d_t = sum g_o     [12..15] d_fx, d_fy, d_cx, d_cy
// with g_dirs = R^T g_d,  dirs = ((x - cx) / fx, -(y - cy) / fy, -1):  d_fx = -sum g_dirs_x dirs_x / fx,  d_cx = -sum g_dirs_x / fx,
// d_fy = -sum g_dirs_y dirs_y / fy,  d_cy = sum g_dirs_y / fy.
// Block b sums the pixels [b chunk, (b + 1) chunk) -- thread t its pixels t, t + 256, ... in order, then the lanes, then the four waves -- and the
// final block sums the partials in block order: the order is a function of n alone.
// ------------------------------------------------------------------------------------------------
struct CamArgs { float fx, fy, cx, cy, r[9]; };

__global__ __launch_bounds__(256) void o_d_partial_kernel(CamArgs c, int W, int row0, const long long* __restrict__ pix, long long n, long long chunk,
                                                           const float* __restrict__ g_o, const float* __restrict__ g_d, float* __restrict__ partial) {
    __shared__ float red[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.0f;
    for (long long i = lo + tid; i < hi; i += 256) {
        const long long p = pix ? pix[i] : i + (long long)row0 * W;
        const int x = (int)(p % W), y = (int)(p / W);
        const float dir[3] = {((float)x - c.cx) / c.fx, -((float)y - c.cy) / c.fy, -1.0f};           // rays.py:28-30
        const float g[3] = {g_d[3 * i + 0], g_d[3 * i + 1], g_d[3 * i + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) s[3 * a + b] += g[a] * dir[b];
        if (g_o) { s[9] += g_o[3 * i + 0]; s[10] += g_o[3 * i + 1]; s[11] += g_o[3 * i + 2]; }
        const float gx = c.r[0] * g[0] + c.r[3] * g[1] + c.r[6] * g[2];                               // (R^T g_d)_x
        const float gy = c.r[1] * g[0] + c.r[4] * g[1] + c.r[7] * g[2];
        s[12] += -(gx * dir[0]) / c.fx;
        s[13] += -(gy * dir[1]) / c.fy;
        s[14] += -gx / c.fx;
        s[15] += gy / c.fy;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) red[wave][k] = s[k];
    }
    __syncthreads();
    if (tid < 16) partial[(size_t)blockIdx.x * 16 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64) void o_d_final_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ d_pose12,
                                                        float* __restrict__ d_k4) {
    const int k = threadIdx.x;
    if (k >= 16) return;
    float s = 0.0f;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * 16 + k];
    if (k < 9) { if (d_pose12) d_pose12[4 * (k / 3) + k % 3] = s; }
    else if (k < 12) { if (d_pose12) d_pose12[4 * (k - 9) + 3] = s; }
    else if (d_k4) d_k4[k - 12] = s;
}

static inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace mipose

using namespace mipose;

extern "C" {

int mi_pose_abi_version(void) { return MI_POSE_ABI_VERSION; }
const char* mi_pose_last_error(void) { return g_err; }

int mi_pose_input_grad(const float* rays, const float* z, const float* raw, const float* d_raw, int64_t n, int S, const float* delta_x0,
                       const float* delta_skip, const float* delta_d, const float* w_x0, int ld_x0, const float* w_skip, int ld_skip,
                       const float* w_d, int ld_d, int W, int L_x, int L_d, float* d_rays, float* d_pts, float* d_view, float* d_emb,
                       void* stream) {
    const char* who = "mi_pose_input_grad";
    POSE_CHECK_ARG(W == 128 || W == 256, "%s: W=%d: the training kernels run W = 128 and W = 256", who, W);
    POSE_CHECK_ARG(L_x >= 0 && L_x <= MI_POSE_MAX_LX, "%s: L_x=%d: 0..%d", who, L_x, MI_POSE_MAX_LX);
    POSE_CHECK_ARG(L_d >= 0 && L_d <= MI_POSE_MAX_LD, "%s: L_d=%d: 0..%d", who, L_d, MI_POSE_MAX_LD);
    POSE_CHECK_ARG(S >= 1, "%s: S=%d must be at least 1", who, S);
    POSE_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40) / S, "%s: n=%lld: 0 .. 2^40 / S", who, (long long)n);
    const int in_x = 3 + 6 * L_x, in_d = 3 + 6 * L_d;
    POSE_CHECK_ARG((delta_skip == nullptr) == (w_skip == nullptr), "%s: delta_skip and w_skip are given together or not at all", who);
    POSE_CHECK_ARG(ld_x0 >= in_x && (!w_skip || ld_skip >= in_x) && ld_d >= W + in_d,
                   "%s: leading dimensions %d / %d / %d below in_x=%d / in_x / W + in_d=%d", who, ld_x0, ld_skip, ld_d, in_x, W + in_d);
    POSE_CHECK_ARG(n == 0 || d_rays != nullptr, "%s: d_rays is NULL", who);
    POSE_CHECK_ARG(n == 0 || (rays && z && raw && d_raw && delta_x0 && delta_d && w_x0 && w_d), "%s: NULL input pointer", who);
    POSE_CHECK_ARG(aligned(raw, 16) && aligned(d_raw, 16), "%s: raw / d_raw must be 16-byte aligned", who);
    POSE_CHECK_ARG(aligned(delta_x0, 16) && aligned(delta_skip, 16) && aligned(delta_d, 16), "%s: the delta tensors must be 16-byte aligned", who);
    POSE_CHECK_ARG(aligned(rays, 4) && aligned(z, 4) && aligned(w_x0, 4) && aligned(w_skip, 4) && aligned(w_d, 4) && aligned(d_rays, 4) &&
                   aligned(d_pts, 4) && aligned(d_view, 4) && aligned(d_emb, 4), "%s: float pointers must be 4-byte aligned", who);
    if (n == 0) return MI_POSE_OK;
    InputGradArgs a{};
    a.rays = rays; a.z = z; a.raw = raw; a.d_raw = d_raw;
    a.n = n; a.S = S; a.L_x = L_x; a.L_d = L_d;
    a.delta_x0 = delta_x0; a.delta_skip = delta_skip; a.delta_d = delta_d;
    a.w_x0 = w_x0; a.w_skip = w_skip; a.w_d = w_d;
    a.ld_x0 = ld_x0; a.ld_skip = ld_skip; a.ld_d = ld_d;
    a.d_rays = d_rays; a.d_pts = d_pts; a.d_view = d_view; a.d_emb = d_emb;
    return W == 256 ? launch_input_grad<256>(a, (hipStream_t)stream) : launch_input_grad<128>(a, (hipStream_t)stream);
}

int mi_pose_ndc_rays_backward(int H, int W, float focal, float near_, const float* rays_o, int64_t o_stride, const float* rays_d,
                              int64_t d_stride, int64_t n, const float* g_o_ndc, const float* g_d_ndc, float* g_o, float* g_d, void* stream) {
    const char* who = "mi_pose_ndc_rays_backward";
    POSE_CHECK_ARG(H > 0 && W > 0, "%s: bad image size H=%d W=%d", who, H, W);
    POSE_CHECK_ARG(isfinite(focal) && focal != 0.0f && isfinite(near_), "%s: focal=%g / near=%g", who, (double)focal, (double)near_);
    POSE_CHECK_ARG(n >= 0 && n <= (int64_t)256 * 0x7fffffff, "%s: n=%lld out of range", who, (long long)n);
    POSE_CHECK_ARG((o_stride == 0 || o_stride == 3) && (d_stride == 0 || d_stride == 3), "%s: strides %lld / %lld must be 0 or 3", who,
                   (long long)o_stride, (long long)d_stride);
    POSE_CHECK_ARG(n == 0 || (rays_o && rays_d && g_o && g_d), "%s: NULL pointer", who);
    POSE_CHECK_ARG(aligned(rays_o, 4) && aligned(rays_d, 4) && aligned(g_o_ndc, 4) && aligned(g_d_ndc, 4) && aligned(g_o, 4) && aligned(g_d, 4),
                   "%s: float pointers must be 4-byte aligned", who);
    if (n == 0) return MI_POSE_OK;
    const float sx = (float)(-1.0 / ((double)W / (2.0 * (double)focal)));
    const float sy = (float)(-1.0 / ((double)H / (2.0 * (double)focal)));
    hipLaunchKernelGGL(ndc_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sx, sy, near_, rays_o,
                       (long long)o_stride, rays_d, (long long)d_stride, (long long)n, g_o_ndc, g_d_ndc, g_o, g_d);
    POSE_LAUNCH_CHECK("ndc_bwd_kernel");
    return MI_POSE_OK;
}

size_t mi_pose_reduce_scratch_bytes(void) { return (size_t)MI_POSE_REDUCE_BLOCKS * 16 * sizeof(float); }

int mi_pose_make_o_d_backward(int W, int H, const float k4[4], const float pose12[12], const int64_t* pix, int row0, int64_t n,
                              const float* g_o, const float* g_d, float* d_pose12, float* d_k4, void* scratch, size_t scratch_bytes,
                              void* stream) {
    const char* who = "mi_pose_make_o_d_backward";
    POSE_CHECK_ARG(W > 0 && H > 0, "%s: bad image size W=%d H=%d", who, W, H);
    POSE_CHECK_ARG(k4 && pose12, "%s: k4 / pose12 is NULL", who);
    POSE_CHECK_ARG(k4[0] != 0.0f && k4[1] != 0.0f, "%s: fx=%g / fy=%g must not be zero", who, (double)k4[0], (double)k4[1]);
    POSE_CHECK_ARG(n >= 0 && n <= (int64_t)1 << 40, "%s: n=%lld out of range", who, (long long)n);
    POSE_CHECK_ARG(pix || (row0 >= 0 && n % W == 0 && row0 + n / W <= H), "%s: rows [%d, +%lld / %d) outside the image of %d rows", who, row0,
                   (long long)n, W, H);
    POSE_CHECK_ARG(n == 0 || g_d != nullptr, "%s: g_d is NULL", who);
    POSE_CHECK_ARG(d_pose12 || d_k4, "%s: d_pose12 and d_k4 are both NULL", who);
    POSE_CHECK_ARG(scratch && scratch_bytes >= mi_pose_reduce_scratch_bytes() && aligned(scratch, 16), "%s: scratch must be 16-byte aligned and hold %zu bytes",
                   who, mi_pose_reduce_scratch_bytes());
    POSE_CHECK_ARG(aligned(pix, 8) && aligned(g_o, 4) && aligned(g_d, 4) && aligned(d_pose12, 4) && aligned(d_k4, 4), "%s: misaligned pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                                                          // the gradient of no pixel is zero: no launch
        if (d_pose12) POSE_HIP(hipMemsetAsync(d_pose12, 0, 12 * sizeof(float), st));
        if (d_k4) POSE_HIP(hipMemsetAsync(d_k4, 0, 4 * sizeof(float), st));
        return MI_POSE_OK;
    }
    CamArgs c;
    c.fx = k4[0]; c.fy = k4[1]; c.cx = k4[2]; c.cy = k4[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c.r[3 * i + j] = pose12[4 * i + j];
    const long long per = ((long long)n + (256LL * MI_POSE_REDUCE_BLOCKS) - 1) / (256LL * MI_POSE_REDUCE_BLOCKS);
    const long long chunk = 256 * per;
    const int blocks = (int)((n + chunk - 1) / chunk);
    hipLaunchKernelGGL(o_d_partial_kernel, dim3(blocks), dim3(256), 0, st, c, W, row0, (const long long*)pix, (long long)n, chunk, g_o, g_d,
                       (float*)scratch);
    POSE_LAUNCH_CHECK("o_d_partial_kernel");
    hipLaunchKernelGGL(o_d_final_kernel, dim3(1), dim3(64), 0, st, (const float*)scratch, blocks, d_pose12, d_k4);
    POSE_LAUNCH_CHECK("o_d_final_kernel");
    return MI_POSE_OK;
}

}  // extern "C"
