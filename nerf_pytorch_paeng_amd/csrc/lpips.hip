// lpips.hip -- libmi_nerf_lpips.so (include/mi_nerf_lpips.h): the LPIPS distance of rendered frames against their targets (utils.py:31-34,
// test.py:75), on the device where test() already holds both images.  A library of its own: nothing of libmi_nerf.so is linked in.
//
// conv_first_kernel   the cin0-channel first layer (K = 9 * cin0 <= 36): one thread per output element, an fmaf chain; applies the input affine.
// conv3x3_mfma_kernel every other convolution: an implicit GEMM (M = pixels, N = cout, K = 9 * cin) on v_mfma_f32_32x32x2_f32 over channel-last
//                     maps.  One workgroup (4 waves) = an 8 x 16 pixel tile (four M-tiles of 2 rows x 16 columns) x 32 * MT output channels.
//                     Wave w owns N-tile w % MT and MT of the four M-tiles; MT is 4, 2 or 1, narrowed on small maps until the grid fills the CUs.  K runs over 32-channel chunks of cin, and inside a chunk over the
//                     nine taps: a chunk's 10 x 18 halo tile goes to LDS once, channel-major, so that a tap is an LDS offset and the A operand of
//                     a k-step is one ds_read_b32 per M-tile.  The B operand never touches LDS: the host packer wrote each N-tile's weights in
//                     the order (chunk, tap, k-pair, lane) the wave consumes them, so a k-step's B is one coalesced 256-byte load, fetched a
//                     tap ahead into registers.  Bias, ReLU and (when a POOL follows directly) the 2 x 2 max-pool are the epilogue: the MFMA's
//                     C layout keeps each pool window in one lane.
// pool_kernel         2 x 2 max-pool of its own, for a POOL that follows a TAP (the un-pooled map is needed first) or the first layer.
// tap_kernel          one wave per pixel: both images' C_t features once, channel norms, weighted squared difference, all in fp64; one fp64
//                     partial per 256 pixels.  tap_final_kernel adds them in a fixed order; after the last tap it adds the d_t and rounds once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/mi_nerf_lpips.h"
#include "abi_error.h"

namespace milpips {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_LPIPS_EHIP)
#define LP_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::milpips, MI_LPIPS_EINVAL, cond, __VA_ARGS__)
#define LP_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::milpips, name)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- geometry ----------------------------------------------------------------------------------
constexpr int TH = 8, TW = 16;              // pixel tile of a workgroup: 4 M-tiles of 2 rows x 16 columns
constexpr int HR = TH + 2, HC = TW + 2;     // with the 1-pixel halo
constexpr int KC = 32;                      // channels of a K chunk
constexpr int PLANE = 226;                  // floats between two channels' halo tiles in LDS: >= HR * HC = 180, and 226 % 64 = 34 puts the two
                                            // k-halves of a wave's ds_read (rows of 16 at +0 and +18) on disjoint banks but for four lanes
constexpr int STEP_FLOATS = (KC / 2) * 64;  // packed weights of one (chunk, tap) of one N-tile
constexpr int ALIGN_FLOATS = 64;            // every section of the blob starts on 256 bytes
constexpr int TAP_PIX = 256;                // pixels per tap partial
constexpr int FILL_BLOCKS = 256;            // workgroups of a convolution launch below which it takes narrower channel groups: one per CU
static_assert(PLANE >= HR * HC, "halo tile fits its plane");

// NaN-propagating: a NaN fails the comparison and stays
__device__ __forceinline__ float relu_nan(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// ---- first layer ---------------------------------------------------------------------------------
// w: [9][cin][cout]; in0 / in1: image 0 and 1 ([H, W, cin] each); out: [n_img][H, W, cout]
__global__ __launch_bounds__(256) void conv_first_kernel(const float* __restrict__ in0, const float* __restrict__ in1, const float* __restrict__ ab,
                                                         const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                         size_t out_img_stride, int H, int W, int cin, int cout) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)H * W * cout;
    if (idx >= total) return;
    const int co = (int)(idx % cout);
    const size_t pix = idx / cout;
    const int y = (int)(pix / W), x = (int)(pix % W);
    const float* in = blockIdx.y ? in1 : in0;
    float acc = bias[co];
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = x + kx - 1;
            if (xx < 0 || xx >= W) continue;
            const float* p = in + ((size_t)yy * W + xx) * cin;
            const float* wt = w + (size_t)(ky * 3 + kx) * cin * cout + co;
            for (int ci = 0; ci < cin; ++ci) acc = fmaf(fmaf(ab[ci], p[ci], ab[4 + ci]), wt[(size_t)ci * cout], acc);
        }
    }
    out[blockIdx.y * out_img_stride + idx] = relu_nan(acc);
}

// ---- the implicit-GEMM convolution -----------------------------------------------------------------------
// in: [n_img][H, W, cin]; wpk: [cout / 32][cin / 32][9][16][64]; out: [n_img][H, W, cout], or with POOL [n_img][H / 2, W / 2, cout]
template <int MT, bool POOL>
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(const float* __restrict__ in, size_t in_img_stride, const float* __restrict__ wpk,
                                                           const float* __restrict__ bias, float* __restrict__ out, size_t out_img_stride, int H,
                                                           int W, int cin, int cout, int tiles_x) {
    __shared__ float halo[KC * PLANE];
    constexpr int MG = 4 / MT;                                  // M-tile groups: wave's M-tiles are g, g + MG, ...
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = blockIdx.y * MT + wave % MT;
    const int g = wave / MT;
    const int y0 = (blockIdx.x / tiles_x) * TH, x0 = (blockIdx.x % tiles_x) * TW;
    in += blockIdx.z * in_img_stride;
    out += blockIdx.z * out_img_stride;
    const int steps = (cin / KC) * 9;
    const float* wp = wpk + (size_t)nt * steps * STEP_FLOATS + lane;
    const int i = lane & 31, kk = lane >> 5;
    const int abase = kk * PLANE + (2 * g + (i >> 4)) * HC + (i & 15);

    f32x16 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    float bcur[KC / 2], bnext[KC / 2];
#pragma unroll
    for (int kp = 0; kp < KC / 2; ++kp) bcur[kp] = wp[kp * 64];

    int s = 0;
#pragma unroll 1
    for (int c0 = 0; c0 < cin; c0 += KC) {
        __syncthreads();                                        // the previous chunk's reads are done
        for (int idx = threadIdx.x; idx < HR * HC * (KC / 4); idx += 256) {
            const int pix = idx >> 3, cg = idx & 7;
            const int y = y0 - 1 + pix / HC, x = x0 - 1 + pix % HC;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // the zero padding, and what lies beyond a partial tile
            if (y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const float4*>(in + ((size_t)y * W + x) * cin + c0 + cg * 4);
            float* d = halo + (cg * 4) * PLANE + pix;
            d[0] = v.x;
            d[PLANE] = v.y;
            d[2 * PLANE] = v.z;
            d[3 * PLANE] = v.w;
        }
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap, ++s) {
            if (s + 1 < steps) {
#pragma unroll
                for (int kp = 0; kp < KC / 2; ++kp) bnext[kp] = wp[(size_t)(s + 1) * STEP_FLOATS + kp * 64];
            }
            const float* a = halo + abase + (tap / 3) * HC + tap % 3;
#pragma unroll
            for (int kp = 0; kp < KC / 2; ++kp)
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kp * 2 * PLANE + j * MG * 2 * HC], bcur[kp], acc[j], 0, 0, 0);
#pragma unroll
            for (int kp = 0; kp < KC / 2; ++kp) bcur[kp] = bnext[kp];
        }
    }

    // C layout: column (cout) = lane & 31, row (pixel of the M-tile) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int co = nt * 32 + i;
    const float bv = bias[co];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int m = g + j * MG;                               // tile rows 2m, 2m + 1
        if (POOL) {
            // pixel p of row 0 is register r(p), pixel p of row 1 is r(p) + 8: a pool window is registers r, r + 1, r + 8, r + 9 of one lane
            const int Hp = H >> 1, Wp = W >> 1;
            const int py = (y0 >> 1) + m;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const int col = (r & 3) + 8 * (r >> 2) + 4 * kk;
                const int px = (x0 + col) >> 1;
                const float v = max_nan(max_nan(relu_nan(acc[j][r] + bv), relu_nan(acc[j][r + 1] + bv)),
                                        max_nan(relu_nan(acc[j][r + 8] + bv), relu_nan(acc[j][r + 9] + bv)));
                if (py < Hp && px < Wp) out[((size_t)py * Wp + px) * cout + co] = v;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = (r & 3) + 8 * (r >> 2) + 4 * kk;
                const int y = y0 + 2 * m + (p >> 4), x = x0 + (p & 15);
                if (y < H && x < W) out[((size_t)y * W + x) * cout + co] = relu_nan(acc[j][r] + bv);
            }
        }
    }
}

// in: [n_img][H, W, C] -> out: [n_img][H / 2, W / 2, C]; the remainder row / column is never read
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ in, size_t in_img_stride, float* __restrict__ out, size_t out_img_stride,
                                                   int H, int W, int C) {
    const int Hp = H >> 1, Wp = W >> 1;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)Hp * Wp * C) return;
    const int c = (int)(idx % C);
    const size_t pix = idx / C;
    const int py = (int)(pix / Wp), px = (int)(pix % Wp);
    const float* p = in + blockIdx.y * in_img_stride + ((size_t)(2 * py) * W + 2 * px) * C + c;
    const size_t row = (size_t)W * C;
    out[blockIdx.y * out_img_stride + idx] = max_nan(max_nan(p[0], p[C]), max_nan(p[row], p[row + C]));
}

// ---- the distance at a tap ---------------------------------------------------------------------------
// fx, fy: [n_pix, C]; w: [C]; partial[blockIdx.x] = sum over the block's TAP_PIX pixels of sum_c w_c (fhat_x_c - fhat_y_c)^2
__global__ __launch_bounds__(256) void tap_kernel(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w,
                                                  size_t n_pix, int C, double* __restrict__ partial) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NV = MI_LPIPS_MAX_COUT / 64;
    double wv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) wv[k] = lane + 64 * k < C ? (double)w[lane + 64 * k] : 0.0;
    double sum = 0.0;                                           // the wave's pixels, in order
    const size_t p0 = (size_t)blockIdx.x * TAP_PIX + wave * (TAP_PIX / 4);
    for (int q = 0; q < TAP_PIX / 4; ++q) {
        const size_t p = p0 + q;
        if (p >= n_pix) break;                                  // uniform over the wave
        double x[NV], y[NV], sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = lane + 64 * k;
            x[k] = c < C ? (double)fx[p * C + c] : 0.0;
            y[k] = c < C ? (double)fy[p * C + c] : 0.0;
            sx = __builtin_fma(x[k], x[k], sx);
            sy = __builtin_fma(y[k], y[k], sy);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sx += __shfl_xor(sx, m, 64);
            sy += __shfl_xor(sy, m, 64);
        }
        const double nx = sqrt(sx) + 1e-10, ny = sqrt(sy) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const double e = x[k] / nx - y[k] / ny;
            d = __builtin_fma(wv[k] * e, e, d);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
        sum += d;
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: d_t = sum(partial) / n_pix into tapvals[t]; after the last tap, LPIPS = sum_t d_t, rounded once
__global__ __launch_bounds__(256) void tap_final_kernel(const double* __restrict__ partial, int n_partial, double n_pix, double* __restrict__ tapvals,
                                                        int t, int n_taps, float* __restrict__ out, float* __restrict__ per_tap) {
    __shared__ double red[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < n_partial; k += 256) s += partial[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double d = red[0] / n_pix;
        tapvals[t] = d;
        if (per_tap) per_tap[t] = (float)d;
        if (t == n_taps - 1) {
            double total = 0.0;
            for (int k = 0; k < n_taps; ++k) total += tapvals[k];
            *out = (float)total;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Plan {
    int n_conv, n_taps, n_pools;
    int conv_cin[MI_LPIPS_MAX_OPS], conv_cout[MI_LPIPS_MAX_OPS];
    size_t conv_w_off[MI_LPIPS_MAX_OPS], conv_b_off[MI_LPIPS_MAX_OPS];   // in floats into the blob
    int tap_c[MI_LPIPS_MAX_TAPS];
    size_t tap_w_off[MI_LPIPS_MAX_TAPS];
    size_t blob_floats;
};

static int resolve_net(const mi_lpips_net* net, Plan* out) {
    LP_CHECK_ARG(net, "NULL net");
    LP_CHECK_ARG(net->n_ops >= 1 && net->n_ops <= MI_LPIPS_MAX_OPS, "n_ops=%d outside 1..%d", net->n_ops, MI_LPIPS_MAX_OPS);
    LP_CHECK_ARG(net->cin0 >= 1 && net->cin0 <= 4, "cin0=%d outside 1..4", net->cin0);
    LP_CHECK_ARG(net->ops[0].kind == MI_LPIPS_CONV, "the first operation must be a CONV (got kind %d)", net->ops[0].kind);
    Plan P;
    memset(&P, 0, sizeof(P));
    size_t off = ALIGN_FLOATS;                                  // a[4], b[4] first
    int c = net->cin0;
    for (int k = 0; k < net->n_ops; ++k) {
        const mi_lpips_op& op = net->ops[k];
        if (op.kind == MI_LPIPS_CONV) {
            LP_CHECK_ARG(op.cout >= 32 && op.cout <= MI_LPIPS_MAX_COUT && op.cout % 32 == 0,
                         "operation %d: cout=%d must be a multiple of 32 in 32..%d", k, op.cout, MI_LPIPS_MAX_COUT);
            const int n = P.n_conv++;
            P.conv_cin[n] = c;
            P.conv_cout[n] = op.cout;
            P.conv_b_off[n] = off;
            off += align_up((size_t)op.cout, ALIGN_FLOATS);
            P.conv_w_off[n] = off;
            off += align_up((size_t)9 * c * op.cout, ALIGN_FLOATS);
            c = op.cout;
        } else if (op.kind == MI_LPIPS_POOL) {
            ++P.n_pools;
        } else if (op.kind == MI_LPIPS_TAP) {
            LP_CHECK_ARG(net->ops[k - 1].kind == MI_LPIPS_CONV, "operation %d: a TAP must follow a CONV directly", k);
            LP_CHECK_ARG(P.n_taps < MI_LPIPS_MAX_TAPS, "more than %d taps", MI_LPIPS_MAX_TAPS);
            const int t = P.n_taps++;
            P.tap_c[t] = c;
            P.tap_w_off[t] = off;
            off += align_up((size_t)c, ALIGN_FLOATS);
        } else {
            LP_CHECK_ARG(false, "operation %d: unknown kind %d", k, op.kind);
        }
    }
    LP_CHECK_ARG(P.n_taps >= 1, "the network has no TAP");
    P.blob_floats = off;
    *out = P;
    return MI_LPIPS_OK;
}

struct Scratch { size_t tapvals, partial, maps, slot, total; };   // byte offsets; slot: floats of one image's map

static int resolve_shape(const mi_lpips_net* net, int H, int W, Plan* P, Scratch* S) {
    if (int rc = resolve_net(net, P)) return rc;
    LP_CHECK_ARG(H >= (1 << P->n_pools) && W >= (1 << P->n_pools) && H <= MI_LPIPS_MAX_DIM && W <= MI_LPIPS_MAX_DIM,
                 "bad image size H=%d W=%d (%d..%d with %d pools)", H, W, 1 << P->n_pools, MI_LPIPS_MAX_DIM, P->n_pools);
    size_t slot = 0;
    int h = H, w = W;
    for (int k = 0; k < net->n_ops; ++k) {
        if (net->ops[k].kind == MI_LPIPS_CONV) {
            const size_t e = (size_t)h * w * net->ops[k].cout;
            slot = e > slot ? e : slot;
        } else if (net->ops[k].kind == MI_LPIPS_POOL) {
            h >>= 1;
            w >>= 1;
        }
    }
    S->slot = align_up(slot, ALIGN_FLOATS);
    S->tapvals = 0;
    S->partial = 256;
    S->maps = align_up(S->partial + ((size_t)H * W + TAP_PIX - 1) / TAP_PIX * sizeof(double), 256);
    S->total = S->maps + 4 * S->slot * sizeof(float);
    return MI_LPIPS_OK;
}

template <int MT>
static void launch_conv(bool pool, dim3 grid, hipStream_t st, const float* in, size_t in_stride, const float* wpk, const float* bias, float* out,
                        size_t out_stride, int H, int W, int cin, int cout, int tiles_x) {
    if (pool)
        hipLaunchKernelGGL((conv3x3_mfma_kernel<MT, true>), grid, dim3(256), 0, st, in, in_stride, wpk, bias, out, out_stride, H, W, cin, cout, tiles_x);
    else
        hipLaunchKernelGGL((conv3x3_mfma_kernel<MT, false>), grid, dim3(256), 0, st, in, in_stride, wpk, bias, out, out_stride, H, W, cin, cout, tiles_x);
}

// Runs the network on n_img (1 or 2) images img0 / img1.  stop_tap >= 0: stop at that tap with its convolution writing to feat_out (features);
// otherwise the distance of img0 against img1 into out / per_tap.
static int run(const mi_lpips_net* net, const Plan& P, const Scratch& S, const float* blob, const float* img0, const float* img1, int n_img, int H,
               int W, int stop_tap, float* feat_out, float* out, float* per_tap, char* scratch, hipStream_t st) {
    double* tapvals = (double*)(scratch + S.tapvals);
    double* partial = (double*)(scratch + S.partial);
    float* buf[2] = {(float*)(scratch + S.maps), (float*)(scratch + S.maps) + 2 * S.slot};
    const float* cur = nullptr;                                 // the map the next operation reads: [n_img][h, w, c], images S.slot apart
    size_t cur_stride = S.slot;
    int which = 0, h = H, w = W, c = net->cin0, conv = 0, tap = 0;
    for (int k = 0; k < net->n_ops; ++k) {
        const int kind = net->ops[k].kind;
        if (kind == MI_LPIPS_CONV) {
            const int cout = net->ops[k].cout;
            const bool last = stop_tap >= 0 && k + 1 < net->n_ops && net->ops[k + 1].kind == MI_LPIPS_TAP && tap == stop_tap;
            float* dst = last ? feat_out : buf[which];
            const float* bias = blob + P.conv_b_off[conv];
            const float* wts = blob + P.conv_w_off[conv];
            if (conv == 0) {
                const size_t blocks = ((size_t)h * w * cout + 255) / 256;
                hipLaunchKernelGGL(conv_first_kernel, dim3((unsigned)blocks, n_img), dim3(256), 0, st, img0, img1, blob, wts, bias, dst, S.slot, h, w, c,
                                   cout);
                LP_LAUNCH_CHECK("conv_first_kernel");
            } else {
                const bool pool = k + 1 < net->n_ops && net->ops[k + 1].kind == MI_LPIPS_POOL;
                const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
                const int ntiles = cout / 32;
                // the widest channel group that divides cout, narrowed while the grid would leave CUs idle (an element's fmaf chain, and so every
                // result bit, is the same for every MT)
                int mt = ntiles % 4 == 0 ? 4 : ntiles % 2 == 0 ? 2 : 1;
                while (mt > 1 && (long long)tiles_x * tiles_y * (ntiles / mt) * n_img < FILL_BLOCKS) mt >>= 1;
                const dim3 grid((unsigned)(tiles_x * tiles_y), ntiles / mt, n_img);
                if (mt == 4) launch_conv<4>(pool, grid, st, cur, cur_stride, wts, bias, dst, S.slot, h, w, c, cout, tiles_x);
                else if (mt == 2) launch_conv<2>(pool, grid, st, cur, cur_stride, wts, bias, dst, S.slot, h, w, c, cout, tiles_x);
                else launch_conv<1>(pool, grid, st, cur, cur_stride, wts, bias, dst, S.slot, h, w, c, cout, tiles_x);
                LP_LAUNCH_CHECK("conv3x3_mfma_kernel");
                if (pool) {                                     // fused: the POOL is done
                    h >>= 1;
                    w >>= 1;
                    ++k;
                }
            }
            if (last) return MI_LPIPS_OK;
            cur = dst;
            which ^= 1;
            c = cout;
            ++conv;
        } else if (kind == MI_LPIPS_POOL) {
            const size_t blocks = ((size_t)(h >> 1) * (w >> 1) * c + 255) / 256;
            hipLaunchKernelGGL(pool_kernel, dim3((unsigned)blocks, n_img), dim3(256), 0, st, cur, cur_stride, buf[which], S.slot, h, w, c);
            LP_LAUNCH_CHECK("pool_kernel");
            cur = buf[which];
            which ^= 1;
            h >>= 1;
            w >>= 1;
        } else {                                                // TAP
            if (stop_tap < 0) {
                const size_t n_pix = (size_t)h * w;
                const int blocks = (int)((n_pix + TAP_PIX - 1) / TAP_PIX);
                hipLaunchKernelGGL(tap_kernel, dim3(blocks), dim3(256), 0, st, cur, cur + cur_stride, blob + P.tap_w_off[tap], n_pix, c, partial);
                LP_LAUNCH_CHECK("tap_kernel");
                hipLaunchKernelGGL(tap_final_kernel, dim3(1), dim3(256), 0, st, partial, blocks, (double)n_pix, tapvals, tap, P.n_taps, out, per_tap);
                LP_LAUNCH_CHECK("tap_final_kernel");
            }
            ++tap;
        }
    }
    return MI_LPIPS_OK;
}

static int check_run_args(const mi_lpips_net* net, const void* blob, size_t blob_bytes, int64_t n, int H, int W, const void* scratch,
                          size_t scratch_bytes, Plan* P, Scratch* S) {
    if (int rc = resolve_shape(net, H, W, P, S)) return rc;
    LP_CHECK_ARG(n >= 1, "needs at least one image (n=%lld)", (long long)n);
    LP_CHECK_ARG(blob && scratch, "NULL pointer (blob and scratch are required)");
    LP_CHECK_ARG(blob_bytes >= P->blob_floats * sizeof(float), "blob too small: %zu < %zu", blob_bytes, P->blob_floats * sizeof(float));
    LP_CHECK_ARG(scratch_bytes >= S->total, "scratch too small: %zu < %zu", scratch_bytes, S->total);
    LP_CHECK_ARG(((uintptr_t)blob & 255) == 0 && ((uintptr_t)scratch & 255) == 0, "blob and scratch must be 256-byte aligned");
    return MI_LPIPS_OK;
}

}  // namespace milpips

extern "C" {

int mi_lpips_abi_version(void) { return MI_LPIPS_ABI_VERSION; }
const char* mi_lpips_last_error(void) { return milpips::g_err; }

int mi_lpips_vgg16(mi_lpips_net* net) {
    LP_CHECK_ARG(net, "NULL net");
    static const int channels[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
    memset(net, 0, sizeof(*net));
    net->cin0 = 3;
    int n = 0;
    for (int k = 0; k < 13; ++k) {
        net->ops[n].kind = MI_LPIPS_CONV;
        net->ops[n++].cout = channels[k];
        if (k == 1 || k == 3 || k == 6 || k == 9 || k == 12) net->ops[n++].kind = MI_LPIPS_TAP;
        if (k == 1 || k == 3 || k == 6 || k == 9) net->ops[n++].kind = MI_LPIPS_POOL;
    }
    net->n_ops = n;
    return MI_LPIPS_OK;
}

size_t mi_lpips_packed_bytes(const mi_lpips_net* net) {
    milpips::Plan P;
    return milpips::resolve_net(net, &P) == MI_LPIPS_OK ? P.blob_floats * sizeof(float) : 0;
}

int mi_lpips_pack_weights(const mi_lpips_net* net, const float* const* conv_w, const float* const* conv_b, const float* const* tap_w,
                          const float* a, const float* b, void* blob_host, size_t bytes) {
    using namespace milpips;
    Plan P;
    if (int rc = resolve_net(net, &P)) return rc;
    LP_CHECK_ARG(conv_w && conv_b && tap_w && a && b && blob_host, "NULL pointer");
    for (int n = 0; n < P.n_conv; ++n) LP_CHECK_ARG(conv_w[n] && conv_b[n], "NULL weight or bias of convolution %d", n);
    for (int t = 0; t < P.n_taps; ++t) LP_CHECK_ARG(tap_w[t], "NULL weights of tap %d", t);
    LP_CHECK_ARG(bytes >= P.blob_floats * sizeof(float), "blob too small: %zu < %zu", bytes, P.blob_floats * sizeof(float));
    float* blob = (float*)blob_host;
    memset(blob, 0, P.blob_floats * sizeof(float));
    for (int ci = 0; ci < net->cin0; ++ci) {
        blob[ci] = a[ci];
        blob[4 + ci] = b[ci];
    }
    for (int n = 0; n < P.n_conv; ++n) {
        const int cin = P.conv_cin[n], cout = P.conv_cout[n];
        const float* w = conv_w[n];                             // [cout][cin][3][3]
        memcpy(blob + P.conv_b_off[n], conv_b[n], cout * sizeof(float));
        float* d = blob + P.conv_w_off[n];
        if (n == 0) {                                           // [tap][cin][cout]
            for (int tap = 0; tap < 9; ++tap)
                for (int ci = 0; ci < cin; ++ci)
                    for (int co = 0; co < cout; ++co) d[((size_t)tap * cin + ci) * cout + co] = w[((size_t)co * cin + ci) * 9 + tap];
        } else {                                                // [N-tile][chunk][tap][k-pair][lane]: lane l holds B[k = l >> 5][column l & 31]
            for (int nt = 0; nt < cout / 32; ++nt)
                for (int ch = 0; ch < cin / KC; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int kp = 0; kp < KC / 2; ++kp)
                            for (int l = 0; l < 64; ++l) {
                                const int co = nt * 32 + (l & 31), ci = ch * KC + 2 * kp + (l >> 5);
                                *d++ = w[((size_t)co * cin + ci) * 9 + tap];
                            }
        }
    }
    for (int t = 0; t < P.n_taps; ++t) memcpy(blob + P.tap_w_off[t], tap_w[t], P.tap_c[t] * sizeof(float));
    return MI_LPIPS_OK;
}

size_t mi_lpips_scratch_bytes(const mi_lpips_net* net, int H, int W) {
    milpips::Plan P;
    milpips::Scratch S;
    return milpips::resolve_shape(net, H, W, &P, &S) == MI_LPIPS_OK ? S.total : 0;
}

int mi_lpips_distance(const mi_lpips_net* net, const void* blob, size_t blob_bytes, const float* pred, const float* target, int64_t n_pairs, int H,
                      int W, float* out, float* per_tap, void* scratch, size_t scratch_bytes, void* stream) {
    using namespace milpips;
    Plan P;
    Scratch S;
    if (int rc = check_run_args(net, blob, blob_bytes, n_pairs, H, W, scratch, scratch_bytes, &P, &S)) return rc;
    LP_CHECK_ARG(pred && target && out, "NULL pointer (pred, target and out are required)");
    LP_CHECK_ARG((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)out | (uintptr_t)per_tap) & 3) == 0, "pred, target, out and per_tap must be 4-byte aligned");
    const size_t img = (size_t)H * W * net->cin0;
    for (int64_t i = 0; i < n_pairs; ++i)
        if (int rc = run(net, P, S, (const float*)blob, pred + i * img, target + i * img, 2, H, W, -1, nullptr, out + i,
                         per_tap ? per_tap + i * P.n_taps : nullptr, (char*)scratch, (hipStream_t)stream))
            return rc;
    return MI_LPIPS_OK;
}

int mi_lpips_features(const mi_lpips_net* net, const void* blob, size_t blob_bytes, const float* img, int64_t n, int H, int W, int tap, float* out,
                      void* scratch, size_t scratch_bytes, void* stream) {
    using namespace milpips;
    Plan P;
    Scratch S;
    if (int rc = check_run_args(net, blob, blob_bytes, n, H, W, scratch, scratch_bytes, &P, &S)) return rc;
    LP_CHECK_ARG(img && out, "NULL pointer (img and out are required)");
    LP_CHECK_ARG((((uintptr_t)img | (uintptr_t)out) & 3) == 0, "img and out must be 4-byte aligned");
    LP_CHECK_ARG(tap >= 0 && tap < P.n_taps, "tap=%d outside 0..%d", tap, P.n_taps - 1);
    int pools = 0, seen = 0;
    for (int k = 0; k < net->n_ops && seen <= tap; ++k) {
        pools += net->ops[k].kind == MI_LPIPS_POOL;
        seen += net->ops[k].kind == MI_LPIPS_TAP;
    }
    const size_t in_img = (size_t)H * W * net->cin0, out_img = (size_t)(H >> pools) * (W >> pools) * P.tap_c[tap];
    for (int64_t i = 0; i < n; ++i)
        if (int rc = run(net, P, S, (const float*)blob, img + i * in_img, nullptr, 1, H, W, tap, out + i * out_img, nullptr, nullptr, (char*)scratch,
                         (hipStream_t)stream))
            return rc;
    return MI_LPIPS_OK;
}

}  // extern "C"
