/*
 * mi_nerf_lpips.h -- C ABI of libmi_nerf_lpips.so: the LPIPS perceptual distance for the evaluation harness, MI355X (gfx950).
 *
 * A library of its own BESIDE the path, like libmi_nerf_iqa.so: nothing here is declared in another header of the project, and the library
 * exports no other mi_* symbol and imports none.  Same conventions: plain C99, raw device pointers, the caller allocates everything
 * including scratch, int status (0 = ok), hipStream_t passed as void*, no host synchronisation, every argument checked before any HIP
 * call, error text through mi_lpips_last_error().
 *
 * LPIPS (Zhang, Isola, Efros, Shechtman, Wang 2018; VGG-16 variant, v0.1) is the fourth number the reference prints per frame
 * (utils.py:31-34, test.py:75).  It is computed here from the definition below, with weights the caller supplies like a checkpoint, and
 * NOT through the third-party package the reference imports (IQA_pytorch.LPIPSvgg): agreement with that package is not verified, because
 * neither that package nor any trained weights are on the build machine.
 *
 *   inputs    pred, target: [n_pairs, H, W, cin0] fp32 (cin0 = 3 for VGG-16), channel last, contiguous, nominally in [0, 1].  No clamping.
 *   affine    x' = a_c * x + b_c per channel; a and b are part of the weights.  Zero padding is applied to x', i.e. after the affine.
 *   network   a table mi_lpips_net of at most MI_LPIPS_MAX_OPS operations, each one of
 *               MI_LPIPS_CONV  3x3 convolution, padding 1 (zeros), stride 1, bias, ReLU; `cout` output channels
 *               MI_LPIPS_POOL  2x2 max-pool, stride 2, floor: the remainder row / column is dropped and never read
 *               MI_LPIPS_TAP   the features at this point enter the distance
 *             mi_lpips_vgg16() fills the standard plan: 13 convolutions with channels 64,64 | 128,128 | 256,256,256 | 512,512,512 |
 *             512,512,512, a pool after convolutions 2, 4, 7 and 10, and a tap after convolutions 2, 4, 7, 10 and 13 (before the pool).
 *             Accepted: 1 <= n_ops <= MI_LPIPS_MAX_OPS; the first operation is a CONV and cin0 is 1..4 (every later convolution reads the
 *             previous one's cout channels); every cout is a multiple of 32 and at most 512; 1..MI_LPIPS_MAX_TAPS taps, each directly
 *             after a CONV; H and W at least 2^(number of pools) and at most MI_LPIPS_MAX_DIM.  Everything else is refused with a
 *             message.  The table exists so that a narrow network can be run at small shapes.
 *   distance  at each tap t with features f in R^{C_t} per pixel (x: pred, y: target):
 *               fhat   = f / (sqrt(sum_c f_c^2) + 1e-10)
 *               d_t    = mean over pixels of sum_c w_{t,c} * (fhat_x_c - fhat_y_c)^2
 *               LPIPS  = sum_t d_t
 *             The w are used as given: no clamping.
 *   arith     Convolutions: fp32 operands, fp32 accumulation (v_mfma_f32_32x32x2_f32; the first, cin0-channel layer is an fmaf chain).
 *             From the fp32 features on everything is fp64: the channel sums, the normalisation, the weighted squared difference, the
 *             spatial mean and the sum over taps; d_t and LPIPS are rounded to fp32 once.  Reductions are fixed-order, no atomics: the
 *             result is bit-identical from run to run and on any stream, and a pair's value does not depend on what it is batched with.
 *   NaN       a NaN in any pixel that is read gives NaN for that pair and for no other: ReLU and max-pool propagate NaN.
 *   identical inputs give exactly 0.0f (so do all-zero features: the 1e-10).
 */
#ifndef MI_NERF_LPIPS_H
#define MI_NERF_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_LPIPS_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_LPIPS_OK 0
#define MI_LPIPS_EINVAL 1   /* bad argument / unsupported shape */
#define MI_LPIPS_EHIP 2     /* HIP runtime error (launch) */

#define MI_LPIPS_CONV 1
#define MI_LPIPS_POOL 2
#define MI_LPIPS_TAP 3

#define MI_LPIPS_MAX_OPS 32
#define MI_LPIPS_MAX_TAPS 8
#define MI_LPIPS_MAX_COUT 512
#define MI_LPIPS_MAX_DIM 8192     /* largest H or W accepted */

typedef struct mi_lpips_op {
    int32_t kind;    /* MI_LPIPS_CONV / MI_LPIPS_POOL / MI_LPIPS_TAP */
    int32_t cout;    /* CONV: output channels; ignored otherwise */
} mi_lpips_op;

typedef struct mi_lpips_net {
    int32_t n_ops;
    int32_t cin0;    /* channels of the images, 1..4 */
    mi_lpips_op ops[MI_LPIPS_MAX_OPS];
} mi_lpips_net;

int mi_lpips_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_lpips_last_error(void);

/* Host only: the VGG-16 plan stated above (cin0 = 3, 22 operations). */
int mi_lpips_vgg16(mi_lpips_net* net);

/* Bytes of the packed weight blob of this network; 0 (and an error text) if the network is refused. */
size_t mi_lpips_packed_bytes(const mi_lpips_net* net);

/* Host only: arrange the weights the way the kernels consume them.  conv_w[i]: convolution i's weight [cout, cin, 3, 3] (OIHW, row major),
 * conv_b[i]: its bias [cout]; tap_w[t]: tap t's channel weights [C_t]; a, b: the input affine [cin0].  blob_host receives
 * mi_lpips_packed_bytes(net) bytes, which the caller copies to the device (256-byte aligned there).
 * Refused: a NULL pointer (also inside the arrays), a refused network, bytes below mi_lpips_packed_bytes(net). */
int mi_lpips_pack_weights(const mi_lpips_net* net, const float* const* conv_w, const float* const* conv_b, const float* const* tap_w,
                          const float* a, const float* b, void* blob_host, size_t bytes);

/* Bytes of device scratch for ONE pair of H x W images (two ping-pong feature maps for two images, the tap partials): pairs are processed
 * one after another inside a call, so the scratch does not grow with n_pairs.  0 (and an error text) if the arguments are refused. */
size_t mi_lpips_scratch_bytes(const mi_lpips_net* net, int H, int W);

/* out_dev[i] = LPIPS(pred_dev[i], target_dev[i]).  per_tap_dev: NULL, or [n_pairs, n_taps] fp32 for the d_t.
 * Refused with MI_LPIPS_EINVAL: a NULL net / blob / pred / target / out / scratch, a refused network, n_pairs < 1, H or W below
 * 2^(number of pools) or above MI_LPIPS_MAX_DIM, blob_bytes below mi_lpips_packed_bytes(net), scratch_bytes below
 * mi_lpips_scratch_bytes(net, H, W), a blob or scratch that is not 256-byte aligned, images that are not 4-byte aligned. */
int mi_lpips_distance(const mi_lpips_net* net, const void* blob_dev, size_t blob_bytes, const float* pred_dev, const float* target_dev,
                      int64_t n_pairs, int H, int W, float* out_dev, float* per_tap_dev, void* scratch_dev, size_t scratch_bytes,
                      void* stream);

/* The un-normalised features at tap `tap` (0-based) of n images: out_dev [n, H_t, W_t, C_t] fp32, where H_t = H >> (pools before the tap).
 * Refusals as mi_lpips_distance, and a tap outside 0 .. n_taps - 1. */
int mi_lpips_features(const mi_lpips_net* net, const void* blob_dev, size_t blob_bytes, const float* img_dev, int64_t n, int H, int W,
                      int tap, float* out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_LPIPS_H */
