/*
 * mi_nerf_pose.h -- C ABI of libmi_nerf_pose.so: gradients of the MI355X (gfx950) NeRF training path with respect to rays and camera poses.
 *
 * A library of its own BESIDE the path: include/mi_nerf.h and the other side headers stay what they are, nothing here is declared there,
 * and libmi_nerf_pose.so exports no mi_nerf_*, mi_occ_*, mi_iqa_*, mi_scene_*, mi_mesh_* or mi_geo_* symbol and links against no other
 * library of the project.  Same conventions: plain C99, raw device pointers, the caller allocates everything, int status (0 = ok),
 * hipStream_t passed as void*, every argument checked before any HIP call, error text through mi_pose_last_error().  No entry synchronises
 * with the host, allocates, or uses an atomic: every sum is taken in a fixed order, so results are bit-reproducible run to run.
 *
 * The backward of the training path (mi_nerf_mlp_backward_mode, include/mi_nerf.h) leaves the pre-activation gradients of every layer in its
 * workspace.  Three more steps take them to the rays and from there to the camera:
 *
 *   mi_pose_input_grad          delta rows -> d rays      (the layers that read gamma(x) / gamma(d), transposed; positional-encoding backward;
 *                                                          per-ray reduction)
 *   mi_pose_ndc_rays_backward   d ndc rays -> d rays      (backward of mi_nerf_ndc_rays, nerf_process.py:8-28)
 *   mi_pose_make_o_d_backward   d rays -> d pose, d K     (backward of mi_nerf_make_o_d / mi_nerf_make_o_d_pixels, rays.py:20-34)
 *
 * THE INPUT-GRADIENT RULE.  in_x = 3 + 6 L_x, in_d = 3 + 6 L_d, P = n S, point p = r S + s of ray r = (o, d), x = o + z d, v = d / |d|:
 *     g_gx[p] = delta_x0[p] . Wx0  +  delta_skip[p] . Wskip[:, :in_x]                              [in_x]
 *     g_gd[p] = delta_d[p] . Wd[:, W : W + in_d]                                                   [in_d]
 *     gamma(x) = (x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x))                  3 components each
 *     g_x[p]  = g_g[0:3] + sum_k 2^k ( cos(2^k x) * g_sin_k  -  sin(2^k x) * g_cos_k )             likewise g_v from g_gd with v
 *     G_o = sum_s g_x;   G_v = sum_s g_v
 *     G_d = sum_s z_s g_x  +  (G_v - v (v . G_v)) / |d|  +  v (1 / |d|) sum_s d_raw[s][3] relu(raw[s][3])
 * The last term is the |d| in dist_i = (z_{i+1} - z_i) |d| of alpha compositing (nerf_process.py:101): d alpha_i / d|d| = sigma_i dist_i
 * exp(-sigma_i dist_i) / |d|, and d_raw[i][3] already is dL/dalpha_i dist_i exp(-sigma_i dist_i) for sigma_i > 0.  Depths are constants.
 */
#ifndef MI_NERF_POSE_H
#define MI_NERF_POSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_POSE_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_POSE_OK 0
#define MI_POSE_EINVAL 1   /* bad argument / unsupported shape */
#define MI_POSE_EHIP 2     /* HIP runtime error */

#define MI_POSE_MAX_LX 10            /* largest L_x / L_d: what the training kernels evaluate */
#define MI_POSE_MAX_LD 4
#define MI_POSE_REDUCE_BLOCKS 256    /* most block partials mi_pose_make_o_d_backward writes */

int mi_pose_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_pose_last_error(void);

/* THE INPUT-GRADIENT RULE for one network.
 *   rays [n,6], z [n,S], raw [n,S,4], d_raw [n,S,4] (both 16-byte aligned)
 *   delta_x0 [P][W], delta_skip [P][W] or NULL (no layer concatenates gamma(x)), delta_d [P][W/2]          (16-byte aligned)
 *   w_x0   = linear_x[0].weight       [W][ld_x0],   ld_x0 >= in_x
 *   w_skip = linear_x[skip+1].weight  [W][ld_skip], ld_skip >= in_x: its FIRST in_x columns are read  (NULL exactly when delta_skip is)
 *   w_d    = linear_d.weight          [W/2][ld_d],  ld_d >= W + in_d: columns W .. W + in_d are read
 *   W in {128, 256}; 0 <= L_x <= MI_POSE_MAX_LX; 0 <= L_d <= MI_POSE_MAX_LD; S >= 1; n >= 0
 * -> d_rays [n,6] (every element written); optionally d_pts [P][3] = g_x, d_view [n,3] = G_v, d_emb [P][in_x + in_d] = (g_gx, g_gd): each is
 * written when not NULL and costs nothing when NULL.  One wavefront owns a ray and walks its samples in order; sin / cos are recomputed
 * from the rays with the forward's routine.  n == 0: nothing is launched and the device pointers may be NULL. */
int mi_pose_input_grad(const float* rays, const float* z, const float* raw, const float* d_raw, int64_t n, int S, const float* delta_x0,
                       const float* delta_skip, const float* delta_d, const float* w_x0, int ld_x0, const float* w_skip, int ld_skip,
                       const float* w_d, int ld_d, int W, int L_x, int L_d, float* d_rays, float* d_pts, float* d_view, float* d_emb,
                       void* stream);

/* Backward of mi_nerf_ndc_rays (same H, W, focal, near and the same strided inputs: o_stride / d_stride in floats, 3 or, for a broadcast
 * row, 0): gradients g_o_ndc [n,3], g_d_ndc [n,3] (either may be NULL, which means zero) -> g_o [n,3], g_d [n,3], written per ray also when
 * the origin is broadcast (the caller sums).  The warped origin lies on the plane z = -near whatever the ray, so no gradient flows through
 * its third component. */
int mi_pose_ndc_rays_backward(int H, int W, float focal, float near_, const float* rays_o, int64_t o_stride, const float* rays_d,
                              int64_t d_stride, int64_t n, const float* g_o_ndc, const float* g_d_ndc, float* g_o, float* g_d, void* stream);

/* bytes of scratch mi_pose_make_o_d_backward needs (16-byte aligned) */
size_t mi_pose_reduce_scratch_bytes(void);

/* Backward of mi_nerf_make_o_d_pixels (pix != NULL: n pixel indices y * W + x, int64) or of mi_nerf_make_o_d (pix == NULL: the n = n_rows * W
 * pixels of rows [row0, row0 + n_rows)).  k4 = (fx, fy, cx, cy) and pose12 = the 3 x 4 pose row-major, HOST arrays as in the forward.
 * g_o [n,3] (may be NULL: zero), g_d [n,3] -> d_pose12 [12] (row-major 3 x 4: d_R[a][b] = sum_p g_d[p][a] dirs[p][b], d_t = sum_p g_o[p]) and
 * d_k4 [4] = (d_fx, d_fy, d_cx, d_cy), both DEVICE pointers, each optional.  dirs[p] = ((x - cx) / fx, -(y - cy) / fy, -1).
 * Sixteen sums: fixed-order block partials in `scratch`, then one final block.  n == 0 writes zeros. */
int mi_pose_make_o_d_backward(int W, int H, const float k4[4], const float pose12[12], const int64_t* pix, int row0, int64_t n,
                              const float* g_o, const float* g_d, float* d_pose12, float* d_k4, void* scratch, size_t scratch_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_POSE_H */
