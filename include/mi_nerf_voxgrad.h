/*
 * mi_nerf_voxgrad.h -- C ABI of libmi_nerf_voxgrad.so: the backward pass of the radiance-grid renderer on the MI355X (gfx950).  Gradients
 * of a loss on rgb, acc and depth with respect to the grid's sigma plane and its coefficient records, so that a grid can be trained
 * against images.
 *
 * A library of its own BESIDE the path and beside the grid's library: nothing here is declared in another header, this header includes
 * no header of the project, and libmi_nerf_voxgrad.so exports no symbol of the other libraries and links against none of them.  Same
 * conventions: plain C99, raw device pointers, the caller allocates everything, int status (0 = ok), hipStream_t passed as void*, every
 * argument checked before any HIP call, error text through mi_voxgrad_last_error().  No entry synchronises with the host, copies or
 * allocates.
 *
 * THE EXCEPTION to the project's habit: contributions to one gradient element are summed with fp32 hardware atomic adds (one
 * global_atomic_add_f32 each, no compare-and-swap loop).  The gradient therefore depends on the order in which the adds arrive in its
 * last bits and is NOT bit-identical from run to run.  Its distance from the exact sum of the same contributions is bounded by
 * c * 2^-24 * A for an element that receives c contributions whose absolute values sum to A, whatever the order.
 *
 * What is differentiated is THE RENDER RULE of include/mi_nerf_vox.h, with THE GRID, THE LATTICE and the basis Y_b of that header; the
 * two structs below have the layout of its grid and configuration structs (36 and 32 bytes). Dense fp32 grids only: sigma float [P_z, P_y, P_x], coef float
 * [P_z, P_y, P_x, R] with R = 4 / 16 / 32 for B = 1 / 4 / 9, skip uint8 per block of 8^3 cells.  d_sigma and d_coef have the shapes of
 * sigma and coef.
 *
 * THE BACKWARD RULE, per ray.  All arithmetic is fp32, every operation rounded once (no contraction).  The forward quantities are those
 * of THE RENDER RULE: the slab, the intervals a_k, b_k, m_k, delta_k, the cell and its trilinear weights w_e, sigma_s, alpha_k, the
 * pre-clamp colour q[c] (the interpolation of q_e[c]), colour[c] = fminf(fmaxf(q[c], 0), 1), T, w = T alpha_k.  (G . x) stands for
 * (G[0] x[0] + G[1] x[1]) + G[2] x[2].
 *   Upstream.    G[3] the gradient of rgb, ga of acc, gd of depth (an absent array is all zeros).  disp and the rays carry no gradient.
 *   Background.  rgb = C + (1 - acc) bg, so the effective gradient of acc is ga' = ga - (G . bg).
 *   Sample.      s_k = ((G . colour_k) + ga') + gd * m_k.  The colour is evaluated at EVERY sample the backward visits, also where
 *                sigma_s == 0 (the forward skips it there only because w = 0 makes it irrelevant): density can grow where there is
 *                none.  Records of inactive points are zero, so the colour there is 0.
 *   Total.       S = sum over k of w_k * s_k, in increasing k, over the samples the forward evaluates: the same k range, the same stop
 *                after a sample that leaves T < T_min, the same bound on k.  (A sample with sigma_s == 0 has w_k = 0 and adds nothing.)
 *   Density.     dL/d sigma_s,k = delta_k * (T_k * s_k - (S - P_k)),  P_k = sum over j < k of w_j * s_j in increasing j (the running
 *                prefix of S), T_k the transmittance BEFORE sample k.  This is d w_k / d sigma_s,k = delta_k (T_k - w_k) and
 *                d w_j / d sigma_s,k = -delta_k w_j for j > k; there is no division by 1 - alpha.
 *                d_sigma[corner e] += w_e * dL/d sigma_s,k.
 *   Colour.      dL/d q_k[c] = w_k * G[c] when 0 <= q_k[c] <= 1 (the ends included: a zero record can start to learn), else 0.
 *                d_coef[corner e][3 b + c] += w_e * Y_b(u) * dL/d q_k[c].  The padding floats of a record are never written.
 *   Skipping.    With use_skip, a sample whose cell's block byte is 0 contributes nothing.  This is a rule per sample: the backward
 *                does not jump, it looks at the byte of every sample's cell.  With use_skip = 0 the gradient is the exact derivative of
 *                the rendered function away from its kinks (the clamps, the cell boundaries); the stop at T_min is treated as fixed.
 *   Misses.      A miss (THE RENDER RULE, step 1) contributes nothing.
 *   Sums.        The entry ADDS into d_sigma and d_coef: the caller zeroes them, or accumulates over batches.  An element no sample
 *                touches is not written; a contribution that is exactly 0 is not added.  Consecutive samples of a ray that share a cell
 *                are summed in registers first, the coefficient sums as sum over k of w_e * dL/d q_k[c], multiplied by Y_b(u) once per
 *                cell: a reordering inside the bound above.
 *   Signed.      The rule's domain is A SIGNED GRID of include/mi_nerf_vox.h as well: sigma of any sign, with
 *                sigma_s = fmaxf(the interpolation of sigma, 0) in both marches, and skip that header's signed skip plane.
 *                d_sigma[corner e] += w_e * dL/d sigma_s,k only where the interpolation is >= 0; where it is negative nothing flows
 *                through the ReLU and nothing is added.  A value of exactly 0 keeps the one-sided derivative written above, so an
 *                all-zero grid can still learn.  On a plane that is >= 0 everywhere fmaxf(x, 0) = x and this is the rule as written
 *                above: the check outputs are the unsigned renderer's bits there, and the signed renderer's bits on a signed plane.
 */
#ifndef MI_NERF_VOXGRAD_H
#define MI_NERF_VOXGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_VOXGRAD_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_VOXGRAD_OK 0
#define MI_VOXGRAD_EINVAL 1   /* bad argument / unsupported shape */
#define MI_VOXGRAD_EHIP 2     /* HIP runtime error */

#define MI_VOXGRAD_MAX_RES 512        /* largest res[i] */
#define MI_VOXGRAD_BLOCK 8            /* cells per axis of one skip block */
#define MI_VOXGRAD_MAX_STEPS 65536    /* largest bound on the samples of one ray: ceil(|hi - lo| / step) + 1, formed in double */

int mi_voxgrad_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_voxgrad_last_error(void);

/* Axis-aligned box cut into res[0] x res[1] x res[2] cells (x, y, z).  lo_i < hi_i, both finite, with a finite fp32 step > 0. */
typedef struct mi_voxgrad_grid {
    float lo[3];
    float hi[3];
    int32_t res[3];
} mi_voxgrad_grid;

/* What the renderer reads beside the grid and the rays.  step > 0; t_near < t_far, not NaN (they may be infinite); 0 <= T_min < 1; bg
 * finite; use_skip 0 or 1. */
typedef struct mi_voxgrad_render_cfg {
    float step;
    float t_near, t_far;
    float T_min;
    float bg[3];
    int32_t use_skip;
} mi_voxgrad_render_cfg;

/* THE BACKWARD RULE.  B = 1, 4 or 9.  rays [n, 6], g_rgb [n, 3]; g_acc and g_depth [n] may each be NULL (zeros); d_sigma and d_coef are
 * added into; rgb_check [n, 3], acc_check and depth_check [n] may each be NULL, and receive the forward values the backward recomputed
 * for its totals (the renderer's own rgb, acc and depth, bit for bit).  skip_dev may be NULL when use_skip is 0; coef_dev and d_coef_dev
 * 16-byte aligned, every other array 4-byte aligned; n >= 0 (0: nothing is launched and the arrays are not looked at).  Refused when the
 * bound on the samples of one ray exceeds MI_VOXGRAD_MAX_STEPS. */
int mi_voxgrad_render_backward(const mi_voxgrad_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev,
                               const float* rays_dev, int64_t n, const mi_voxgrad_render_cfg* cfg, const float* g_rgb_dev, const float* g_acc_dev,
                               const float* g_depth_dev, float* d_sigma_dev, float* d_coef_dev, float* rgb_check_dev, float* acc_check_dev,
                               float* depth_check_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_VOXGRAD_H */
