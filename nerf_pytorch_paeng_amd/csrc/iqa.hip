// iqa.hip -- libmi_nerf_iqa.so (include/mi_nerf_iqa.h): SSIM of rendered frames against their targets (utils.py:26-29, test.py:71), on the device
// where test() already holds both images.  A library of its own: nothing of libmi_nerf.so is linked in, nothing here is exported from it.
//
// ssim_tile_kernel   one workgroup = one 32 x 64 tile of a frame's SSIM map, all three channels.  The tile and its 10-pixel halo of both images
//                    (42 rows x 74 pixels x 3 channels) go to LDS once, read as the contiguous runs they are in the interleaved [H, W, 3] rows
//                    (average-pooled on the way when downsampling).  Thread j owns interleaved column j of the tile (pixel j / 3, channel j % 3):
//                    the horizontal pass of a row is 11 taps 3 floats apart in LDS -- no de-interleaving, lanes read consecutive words, no bank
//                    conflict -- and the vertical pass stays in registers: a row's five horizontal moments are added, tap-weighted, into the
//                    11 open map rows they belong to (55 fp64 accumulators per thread).  No moment map exists in LDS or HBM.  The tile's sum is reduced in a fixed order.
// ssim_final_kernel  one workgroup per frame adds that frame's tile partials in a fixed order and divides.
// Arithmetic: fp64 moments of the fp32 pixels (mi_nerf_iqa.h says why); the kernel is bound by its fp64 FMAs, not by HBM.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/mi_nerf_iqa.h"
#include "abi_error.h"
#include "block_scan.h"

namespace miiqa {

// ---- error plumbing (abi_error.h) ----------------------------------------------------------------------
ABI_ERROR_STATE(static, MI_IQA_EHIP)
#define IQA_CHECK_ARG(cond, ...) ABI_CHECK_ARG(::miiqa, MI_IQA_EINVAL, cond, __VA_ARGS__)
#define IQA_LAUNCH_CHECK(name) ABI_LAUNCH_CHECK(::miiqa, name)

// ---- geometry ----------------------------------------------------------------------------------
constexpr int TAPS = MI_IQA_SSIM_TAPS;      // 11
constexpr int HALO = TAPS - 1;              // 10
constexpr int TH = 32;                      // map rows of a tile
constexpr int TW = 64;                      // map pixels of a tile row
constexpr int NT = TW * 3;                  // threads = interleaved columns of the tile's map (3 waves)
constexpr int IN_ROWS = TH + HALO;          // 42
constexpr int IN_COLS = (TW + HALO) * 3;    // 222 interleaved floats per tile row
constexpr int MAX_FRAMES_PER_LAUNCH = 65535;
static_assert(NT % 64 == 0, "whole waves");

struct Window { double g[TAPS]; };

static Window make_window() {
    Window w;
    double s = 0.0;
    for (int i = 0; i < TAPS; ++i) {
        const double d = (double)(i - TAPS / 2);
        w.g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += w.g[i];
    }
    for (int i = 0; i < TAPS; ++i) w.g[i] /= s;
    return w;
}

struct Geom {
    int H, W;           // of the images in memory
    int f;              // pooling factor (1: none)
    int Hp, Wp;         // pooled size
    int Mh, Mw;         // map size
    int tiles_x, tiles_y;
};

using miblock::block_sum;                    // deterministic block sum in fp64, NT / 64 waves; valid on thread 0

// one pooled pixel-channel of frame `img` (f == 1: the pixel itself); fixed summation order, fp64 sum, rounded to fp32 like a pooled image
__device__ __forceinline__ float pooled_at(const float* __restrict__ img, const Geom& G, int pr, int px, int ch) {
    if (G.f == 1) return img[((long long)pr * G.W + px) * 3 + ch];
    double s = 0.0;
    for (int dy = 0; dy < G.f; ++dy) {
        const float* row = img + ((long long)(pr * G.f + dy) * G.W + (long long)px * G.f) * 3 + ch;
        for (int dx = 0; dx < G.f; ++dx) s += (double)row[dx * 3];
    }
    return (float)(s / (double)(G.f * G.f));
}

__global__ __launch_bounds__(NT) void ssim_tile_kernel(const float* __restrict__ pred, const float* __restrict__ target, Geom G, Window win,
                                                       int clamp_cs, long long frame0, float* __restrict__ map, double* __restrict__ partial) {
    __shared__ float sx[IN_ROWS * IN_COLS];
    __shared__ float sy[IN_ROWS * IN_COLS];
    __shared__ double red[NT / 64];
    const long long frame = frame0 + blockIdx.z;
    const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;       // first map row / pixel of the tile == first pooled row / pixel it reads
    const long long frame_floats = (long long)G.H * G.W * 3;
    const float* px_img = pred + frame * frame_floats;
    const float* py_img = target + frame * frame_floats;

    // tile + halo -> LDS; what lies outside the pooled image is 0 and only ever feeds map pixels that are masked below
    for (int idx = threadIdx.x; idx < IN_ROWS * IN_COLS; idx += NT) {
        const int r = idx / IN_COLS, c = idx - r * IN_COLS;
        const int pr = oy0 + r, pp = ox0 + c / 3, ch = c % 3;
        float vx = 0.0f, vy = 0.0f;
        if (pr < G.Hp && pp < G.Wp) {
            vx = pooled_at(px_img, G, pr, pp, ch);
            vy = pooled_at(py_img, G, pr, pp, ch);
        }
        sx[idx] = vx;
        sy[idx] = vy;
    }
    __syncthreads();

    const int j = threadIdx.x;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const bool col_ok = ox0 + j / 3 < G.Mw;
    const long long map_row_floats = (long long)G.Mw * 3;
    float* mp = map ? map + (frame * G.Mh + oy0) * map_row_floats + (long long)ox0 * 3 + j : nullptr;
    double sum = 0.0;

    // Vertical pass in registers.  Map row o is built in slot o % 11 of q: input row r adds its horizontal moments, weighted g[r - o], to the 11
    // rows o = r-10 .. r that are open (a fresh row starts by assignment), and row r-10 is then complete.  The row loop runs in blocks of 11
    // so that slot and tap are compile-time for each of a block's rows: the slots rotate by name, nothing is moved.
    double q[TAPS][5];
#pragma unroll
    for (int s = 0; s < TAPS; ++s)
#pragma unroll
        for (int m = 0; m < 5; ++m) q[s][m] = 0.0;

#pragma unroll 1
    for (int base = 0; base < IN_ROWS; base += TAPS) {
        const float* bx = sx + base * IN_COLS + j;
        const float* by = sy + base * IN_COLS + j;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int r = base + t;
            if (r < IN_ROWS) {                                              // uniform: the last block is short
                double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                    // horizontal moments of input row r at column j: x, y, xx, yy, xy
#pragma unroll
                for (int k = 0; k < TAPS; ++k) {
                    const double x = (double)bx[t * IN_COLS + 3 * k];
                    const double y = (double)by[t * IN_COLS + 3 * k];
                    const double gx = win.g[k] * x, gy = win.g[k] * y;
                    h[0] += gx;
                    h[1] += gy;
                    h[2] = __builtin_fma(gx, x, h[2]);
                    h[3] = __builtin_fma(gy, y, h[3]);
                    h[4] = __builtin_fma(gx, y, h[4]);
                }
#pragma unroll
                for (int s = 0; s < TAPS; ++s) {
                    const int k = t - s < 0 ? t - s + TAPS : t - s;         // tap of row r in the map row that lives in slot s
#pragma unroll
                    for (int m = 0; m < 5; ++m) q[s][m] = k == 0 ? win.g[0] * h[m] : __builtin_fma(win.g[k], h[m], q[s][m]);
                }
                if (r >= HALO) {                                            // map row o = r - 10 is complete, in slot (t + 1) % 11
                    const double* a = q[(t + 1) % TAPS];
                    const int o = r - HALO;
                    const double mx = a[0], my = a[1];
                    const double vx = a[2] - mx * mx, vy = a[3] - my * my, cov = a[4] - mx * my;
                    const double n_l = 2.0 * mx * my + C1, d_l = mx * mx + my * my + C1;
                    const double n_cs = 2.0 * cov + C2, d_cs = vx + vy + C2;
                    double v;
                    if (clamp_cs) {
                        double cs = n_cs / d_cs;
                        cs = cs < 0.0 ? 0.0 : cs;                           // a NaN fails the comparison and stays
                        v = (n_l / d_l) * cs;
                    } else {
                        v = (n_l * n_cs) / (d_l * d_cs);
                    }
                    if (col_ok && oy0 + o < G.Mh) {
                        sum += v;
                        if (mp) mp[o * map_row_floats] = (float)v;
                    }
                }
            }
        }
    }
    sum = block_sum(sum, red);
    if (threadIdx.x == 0)
        partial[(frame * G.tiles_y + blockIdx.y) * G.tiles_x + blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ partial, int tiles, double count, float* __restrict__ out) {
    __shared__ double red[4];
    const double* p = partial + (long long)blockIdx.x * tiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) s += p[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s / count);
}

// ---- host side -----------------------------------------------------------------------------------
static int resolve(int64_t n_frames, int H, int W, int downsample, Geom* out) {
    IQA_CHECK_ARG(n_frames >= 1, "ssim needs at least one frame (n_frames=%lld)", (long long)n_frames);
    IQA_CHECK_ARG(H >= 1 && W >= 1 && H <= MI_IQA_MAX_DIM && W <= MI_IQA_MAX_DIM, "bad image size H=%d W=%d (1..%d)", H, W, MI_IQA_MAX_DIM);
    IQA_CHECK_ARG(downsample >= 0, "downsample must be >= 1, or 0 for the MATLAB rule (got %d)", downsample);
    Geom G;
    G.H = H;
    G.W = W;
    const int m = H < W ? H : W;
    G.f = downsample > 0 ? downsample : ((m + 128) / 256 > 1 ? (m + 128) / 256 : 1);       // max(1, round(min(H, W) / 256))
    G.Hp = H / G.f;
    G.Wp = W / G.f;
    IQA_CHECK_ARG(G.Hp >= TAPS && G.Wp >= TAPS, "image %d x %d pooled by %d is %d x %d: below the %d-tap window", H, W, G.f, G.Hp, G.Wp, TAPS);
    G.Mh = G.Hp - HALO;
    G.Mw = G.Wp - HALO;
    G.tiles_x = (G.Mw + TW - 1) / TW;
    G.tiles_y = (G.Mh + TH - 1) / TH;
    IQA_CHECK_ARG(n_frames <= ((int64_t)1 << 40) / ((int64_t)G.tiles_x * G.tiles_y), "n_frames=%lld too large", (long long)n_frames);
    *out = G;
    return MI_IQA_OK;
}

static int ssim(const float* pred, const float* target, int64_t n_frames, int H, int W, int downsample, uint32_t flags, float* out, float* map,
                void* scratch, size_t scratch_bytes, hipStream_t st) {
    Geom G;
    if (int rc = resolve(n_frames, H, W, downsample, &G)) return rc;
    IQA_CHECK_ARG((flags & ~MI_IQA_SSIM_CLAMP_CS) == 0, "unknown flag bits 0x%x (MI_IQA_SSIM_CLAMP_CS = 1 is the only flag)", flags);
    IQA_CHECK_ARG(pred && target && out && scratch, "NULL pointer (pred, target, out and scratch are required)");
    const int tiles = G.tiles_x * G.tiles_y;
    const size_t need = (size_t)n_frames * tiles * sizeof(double);
    IQA_CHECK_ARG(scratch_bytes >= need, "scratch too small: %zu < %zu", scratch_bytes, need);
    IQA_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    const Window win = make_window();
    for (int64_t f0 = 0; f0 < n_frames; f0 += MAX_FRAMES_PER_LAUNCH) {
        const int nz = (int)(n_frames - f0 < MAX_FRAMES_PER_LAUNCH ? n_frames - f0 : MAX_FRAMES_PER_LAUNCH);
        hipLaunchKernelGGL(ssim_tile_kernel, dim3(G.tiles_x, G.tiles_y, nz), dim3(NT), 0, st, pred, target, G, win,
                           (int)(flags & MI_IQA_SSIM_CLAMP_CS), (long long)f0, map, (double*)scratch);
        IQA_LAUNCH_CHECK("ssim_tile_kernel");
    }
    const double count = (double)G.Mh * (double)G.Mw * 3.0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 1 << 30) {
        const int nb = (int)(n_frames - f0 < (1 << 30) ? n_frames - f0 : (1 << 30));
        hipLaunchKernelGGL(ssim_final_kernel, dim3(nb), dim3(256), 0, st, (const double*)scratch + f0 * tiles, tiles, count, out + f0);
        IQA_LAUNCH_CHECK("ssim_final_kernel");
    }
    return MI_IQA_OK;
}

}  // namespace miiqa

extern "C" {

int mi_iqa_abi_version(void) { return MI_IQA_ABI_VERSION; }
const char* mi_iqa_last_error(void) { return miiqa::g_err; }

int mi_iqa_ssim_window(double* taps_host) {
    IQA_CHECK_ARG(taps_host, "NULL pointer");
    const miiqa::Window w = miiqa::make_window();
    for (int i = 0; i < miiqa::TAPS; ++i) taps_host[i] = w.g[i];
    return MI_IQA_OK;
}

int mi_iqa_ssim_downsample_factor(int H, int W, int downsample) {
    miiqa::Geom G;
    return miiqa::resolve(1, H, W, downsample, &G) == MI_IQA_OK ? G.f : 0;
}

size_t mi_iqa_ssim_scratch_bytes(int64_t n_frames, int H, int W, int downsample) {
    miiqa::Geom G;
    if (miiqa::resolve(n_frames, H, W, downsample, &G) != MI_IQA_OK) return 0;
    return (size_t)n_frames * G.tiles_x * G.tiles_y * sizeof(double);
}

int mi_iqa_ssim(const float* pred, const float* target, int64_t n_frames, int H, int W, int downsample, uint32_t flags, float* out, float* map,
                void* scratch, size_t scratch_bytes, void* stream) {
    return miiqa::ssim(pred, target, n_frames, H, W, downsample, flags, out, map, scratch, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
