/*
 * mi_nerf_iqa.h -- C ABI of libmi_nerf_iqa.so: image-quality metrics for the evaluation harness, MI355X (gfx950).
 *
 * A library of its own BESIDE the path: include/mi_nerf.h is the drop-in boundary of the reference's hot path
 * and stays what it is; nothing here is declared there, and libmi_nerf_iqa.so exports no mi_nerf_* symbol.  Same conventions: plain C99,
 * raw device pointers, the caller allocates everything, int status (0 = ok), hipStream_t passed as void*, no host synchronisation, every
 * argument checked before any HIP call, error text through mi_iqa_last_error().
 *
 * SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) in the form image-quality packages use for float images with data range 1.  It is the
 * number the reference prints per frame next to PSNR (utils.py:26-29, test.py:71), computed here from the definition below and NOT
 * through the third-party package the reference imports: agreement with that package is not verified, and the two options are the
 * points at which SSIM packages are known to differ.
 *
 *   inputs   pred, target: [n_frames, H, W, 3] fp32, channel last, contiguous.  No clamping.
 *   window   11 taps g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), normalised to sum 1, applied separably (rows, then columns), 'valid' support:
 *            the map is (H-10) x (W-10) per channel.
 *   per channel and map pixel, under the window:  mu_x, mu_y, E[x^2], E[y^2], E[xy];
 *            var_x = E[x^2] - mu_x^2,  var_y likewise,  cov = E[xy] - mu_x mu_y;   C1 = 0.01^2, C2 = 0.03^2;
 *            ssim = ((2 mu_x mu_y + C1) (2 cov + C2)) / ((mu_x^2 + mu_y^2 + C1) (var_x + var_y + C2))
 *   result   the mean over all channels and map pixels: one float per frame.
 *   options  downsample f >= 1: f > 1 average-pools both images by f x f first (the remainder rows and columns are dropped and never
 *            read); f = 0 is the MATLAB rule f = max(1, round(min(H, W) / 256)).  MI_IQA_SSIM_CLAMP_CS: the contrast-structure
 *            factor (2 cov + C2) / (var_x + var_y + C2) is clamped at 0 from below before the product.  Both are off by default.
 *   NaN      a NaN in any pixel that is read gives a NaN result for that frame (and for no other frame).  It is never hidden.
 *
 * The moments are accumulated in fp64 from the fp32 pixels: var = E[x^2] - mu^2 cancels, and in fp32 the rounding of a flat region's
 * moments is of the size of C2.  The result is rounded to fp32 once, at the end.  It is bit-identical from run to run, on any stream,
 * and a frame's value does not depend on the frames it is batched with (fixed-order reductions, no atomics).
 */
#ifndef MI_NERF_IQA_H
#define MI_NERF_IQA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_IQA_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_IQA_OK 0
#define MI_IQA_EINVAL 1   /* bad argument / unsupported shape */
#define MI_IQA_EHIP 2     /* HIP runtime error (launch) */

/* flags of mi_iqa_ssim */
#define MI_IQA_SSIM_CLAMP_CS 1u   /* clamp the contrast-structure factor at 0 from below */

#define MI_IQA_SSIM_TAPS 11       /* window length; the map loses MI_IQA_SSIM_TAPS - 1 rows and columns */
#define MI_IQA_MAX_DIM 262144     /* largest H or W accepted */

int mi_iqa_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_iqa_last_error(void);

/* Host only: the MI_IQA_SSIM_TAPS normalised window taps the kernel uses, in fp64. */
int mi_iqa_ssim_window(double* taps_host);

/* The factor mi_iqa_ssim pools by: `downsample` itself if >= 1, the MATLAB rule if 0; 0 (and an error text) if the arguments are refused. */
int mi_iqa_ssim_downsample_factor(int H, int W, int downsample);

/* Bytes of device scratch mi_iqa_ssim needs for these sizes (one fp64 partial per map tile and frame); 0 (and an error text) if the
 * arguments are refused. */
size_t mi_iqa_ssim_scratch_bytes(int64_t n_frames, int H, int W, int downsample);

/* SSIM of n_frames image pairs in one launch (utils.py:26-29, test.py:71): out_dev[i] = SSIM(pred_dev[i], target_dev[i]).
 * map_dev: NULL, or [n_frames, Hp-10, Wp-10, 3] fp32 for the SSIM map (Hp = H / f, Wp = W / f: the pooled size).
 * Refused with MI_IQA_EINVAL: a NULL pred / target / out / scratch, n_frames < 1, pooled H or W below MI_IQA_SSIM_TAPS, H or W above
 * MI_IQA_MAX_DIM, a negative downsample, unknown flag bits, scratch_bytes below mi_iqa_ssim_scratch_bytes(). */
int mi_iqa_ssim(const float* pred_dev, const float* target_dev, int64_t n_frames, int H, int W, int downsample, uint32_t flags,
                float* out_dev, float* map_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_IQA_H */
