/*
 * mi_nerf_geo.h -- C ABI of libmi_nerf_geo.so: geometry losses and grid regularisers for the MI355X (gfx950) training paths.
 *
 * A library of its own BESIDE the path: include/mi_nerf.h and the other side headers stay what they are, nothing here is declared there,
 * and libmi_nerf_geo.so exports no mi_nerf_*, mi_occ_*, mi_iqa_*, mi_scene_* or mi_mesh_* symbol and links against no other library of
 * the project.  Same conventions: plain C99, raw device pointers, the caller allocates everything, int status (0 = ok), hipStream_t
 * passed as void*, every argument checked before any HIP call, error text through mi_geo_last_error().  No entry synchronises with the
 * host, allocates, or uses an atomic.
 *
 * mi_nerf_composite_backward (include/mi_nerf.h) differentiates alpha compositing with respect to rgb_map alone.  The entries here are
 * the compositing pair for losses that also read the accumulated opacity, the expected depth, the per-sample weights and the
 * mip-NeRF 360 distortion regulariser (Barron et al., CVPR 2022, eq. 15): a forward that returns what mi_nerf_composite returns plus the
 * distortion loss per ray, and one fused backward for all five gradients.
 *
 * Notation (post_process, nerf_process.py:89-140, as mi_nerf_composite states it; all arithmetic fp32):
 *     dist_i = (z_{i+1} - z_i) |d|,  1e10 |d| for the last sample;   a_i = 1 - expf(-relu(sigma_i) dist_i);   S == 1: a_0 = 0
 *     u_i = 1 - a_i + 1e-10;   T_i = prod_{k<i} u_k;   w_i = a_i T_i;   c_i = sigmoid(raw_i[0..2])
 *     rgb = sum_i w_i c_i + 1 - sum_i w_i;   acc = sum_i w_i;   depth = sum_i w_i z_i
 * Depths and rays are constants.  With q_i := dL/dw_i,
 *     dL/da_i     = q_i T_i - (sum_{k>i} q_k w_k) / u_i
 *     d_raw[i][3] = dL/da_i * dist_i expf(-relu(sigma_i) dist_i)   for sigma_i > 0, else 0
 *     d_raw[i][ch] = G_rgb[ch] w_i c_i,ch (1 - c_i,ch)             ch = 0, 1, 2
 *     q_i = sum_ch G_rgb[ch] (c_i,ch - 1)  +  G_acc  +  G_depth z_i  +  G_w[i]  +  G_dist qd_i
 * disp is not differentiable (it passes through a max, a NaN filter and a clamp).
 *
 * THE DISTORTION RULE (per ray; z ascending, as stratified depths and the sorted merge of the fine depths are):
 *     t_i     = (z_i - near) / (far - near)
 *     delta_i = t_{i+1} - t_i,   delta_{S-1} = 0       (the 1e10 last distance of post_process is not an interval)
 *     m_i     = t_i + delta_i / 2
 *     distortion = sum_i sum_j w_i w_j |m_i - m_j|  +  (1/3) sum_i w_i^2 delta_i
 * m is non-decreasing, so the pair sum needs only scans.  With the exclusive prefix / suffix sums
 *     W<_i = sum_{k<i} w_k,  W>_i = sum_{k>i} w_k,  M<_i = sum_{k<i} w_k m_k,  M>_i = sum_{k>i} w_k m_k:
 *     qd_i       = d distortion / d w_i = 2 ( m_i (W<_i - W>_i) - (M<_i - M>_i) ) + (2/3) w_i delta_i
 *     distortion = sum_i w_i ( m_i (W<_i - W>_i) - (M<_i - M>_i) ) + (1/3) sum_i w_i^2 delta_i
 * (a z that is not ascending is not refused: the scan forms are then what is computed, not the absolute values).
 *
 * THE LATTICE REGULARISERS (since ABI 2): a total variation and a Cauchy sparsity prior over the arrays of a radiance grid (the sigma plane
 * and the records of include/mi_nerf_vox.h), value and gradient.  All arithmetic is fp32, every operation rounded once, nothing contracted;
 * sqrtf and division are correctly rounded (the promise include/mi_nerf_optim.h makes).
 *   The array.  v is float [P_z, P_y, P_x, R], channel-last, with 1 <= C <= R counted channels; P = {P_z, P_y, P_x}.  The channels c >= C
 *     are padding: their values enter no result and they are never written (a row that is moved whole is read with them).  The sigma plane
 *     is R = C = 1; the records are R = 4 / 16 / 32 with C = 3 / 12 / 27.  2 <= P_a <= 513.  v and d_v are 16-byte aligned when R > 1,
 *     4-byte aligned otherwise, and do not overlap.
 *   The mask.  mask is uint8 [ceil((P_z-1)/8), ceil((P_y-1)/8), ceil((P_x-1)/8)] -- the shape of the grid's skip plane -- or NULL.  The
 *     term of point p is COUNTED iff mask is NULL or mask[block(p)] != 0, with block(p)_a = min(p_a, P_a - 2) >> 3.
 *   Total variation.  For p = (z, y, x) and channel c < C:
 *     d_a(p) = v[p + e_a][c] - v[p][c]   for a = x, y, z where p_a + 1 < P_a, otherwise exactly 0
 *     t(p)   = sqrtf(((eps + d_x d_x) + d_y d_y) + d_z d_z),   eps > 0 and finite
 *     TV     = sum of t(p, c) over the counted p and c < C
 *     g      = ((own + b_x) + b_y) + b_z                       per element of d_v, where
 *       own  = -(((d_x(p) + d_y(p)) + d_z(p)) / t(p))          when p is counted, otherwise 0
 *       b_a  = d_a(p - e_a) / t(p - e_a)                       when p_a >= 1 and p - e_a is counted, otherwise 0
 *     d_v[p][c] = d_v[p][c] + scale g
 *     A gather: one thread owns one element of d_v, reads the 13-point stencil around it and issues no atomic.  An element with own and
 *     every b_a absent is not written.
 *   Sparsity (Cauchy), on a plane with R = C = 1:
 *     SP = sum of log1p(2 sigma^2) over the counted points;   g = (4 sigma) / (1 + (2 sigma) sigma);   d_sigma[p] = d_sigma[p] + scale g
 *     for the counted p.  At sigma = 4096 g is 4.9e-4, near sigma = 0.7 it peaks at 1.41: fog is charged, a saturated surface is left alone.
 *   Values.  Each term is widened to double (t(p, c) as the fp32 number it is; sigma before 2 sigma^2 is formed, so the argument of log1p
 *     is exact, and log1p is taken in double) and the sum is taken in a FIXED order: one partial per workgroup into the caller's scratch,
 *     then a finishing launch that adds the partials in index order and by a fixed tree.  One double is written to value_dev, bit-identical
 *     from run to run; so are the gradients.  A workgroup whose blocks of the mask -- and, for the gradient, the three backward neighbour
 *     blocks -- are all zero reads nothing of v or d_v and writes nothing but its zero partial.
 */
#ifndef MI_NERF_GEO_H
#define MI_NERF_GEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_GEO_ABI_VERSION 2

/* status codes (the values of mi_nerf.h) */
#define MI_GEO_OK 0
#define MI_GEO_EINVAL 1   /* bad argument / unsupported shape */
#define MI_GEO_EHIP 2     /* HIP runtime error */

#define MI_GEO_MAX_SAMPLES 1024 /* largest S, as for mi_nerf_composite */
#define MI_GEO_LATTICE_MAX_POINTS 513 /* largest P_a of THE LATTICE REGULARISERS */

int mi_geo_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_geo_last_error(void);

/* raw [n,S,4] (16-byte aligned), z [n,S], rays [n,ray_stride] (ray_stride 6: (o, d); 3: d alone) -> rgb [n,3], disp [n], acc [n],
 * weights [n,S], depth [n]: the numbers mi_nerf_composite writes, bit for bit, and distortion [n] under THE DISTORTION RULE.  Any of the
 * six outputs may be NULL (it is then not written).  One wavefront per ray.
 * n >= 0; 1 <= S <= MI_GEO_MAX_SAMPLES; near_ < far_, both finite.  n == 0: nothing is launched and the device pointers may be NULL. */
int mi_geo_composite(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int S, float near_, float far_,
                     float* rgb, float* disp, float* acc, float* weights, float* depth, float* distortion, void* stream);

/* The backward of mi_geo_composite: gradients with respect to rgb [n,3], acc [n], depth [n], distortion [n] and weights [n,S] ->
 * d_raw [n,S,4] (16-byte aligned).  Each of the five gradient pointers may be NULL, which means zero; every element of d_raw is written
 * (all five NULL: zeros).  The forward quantities are recomputed; one wavefront per ray; the scans of the distortion term are run only
 * when g_distortion is given, and with g_rgb alone the arithmetic is that of mi_nerf_composite_backward.
 * Sizes and bounds as for mi_geo_composite; d_raw must not be NULL (n > 0). */
int mi_geo_composite_backward(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int S, float near_,
                              float far_, const float* g_rgb, const float* g_acc, const float* g_depth, const float* g_distortion,
                              const float* g_weights, float* d_raw, void* stream);

/* Bytes of scratch a value of THE LATTICE REGULARISERS needs for this shape (one double per workgroup); 0 for a bad argument:
 * P NULL or a P_a outside 2..MI_GEO_LATTICE_MAX_POINTS, R not in {1, 4, 16, 32}, C outside 1..R. */
size_t mi_geo_lattice_scratch_bytes(const int32_t P[3], int R, int C);

/* Total variation of v [P_z,P_y,P_x,R] under mask (or NULL): TV -> value_dev (one double), and d_v = d_v + scale g.  d_v may be NULL (value
 * only); value_dev may be NULL (gradient only; scratch may then be NULL); both NULL: nothing is launched, the arguments are still checked.
 * scratch: at least the bytes the entry above names, 8-byte aligned, as is value_dev.  eps > 0 and finite; scale finite. */
int mi_geo_lattice_tv(const int32_t P[3], int R, int C, const float* v, const uint8_t* mask, float eps, float scale, float* d_v,
                      double* value_dev, void* scratch, size_t scratch_bytes, void* stream);

/* The Cauchy sparsity prior of the plane sigma [P_z,P_y,P_x] under mask (or NULL): SP -> value_dev, and d_sigma = d_sigma + scale g.  NULL
 * outputs and scratch as for the entry above; the scratch size is that of R = C = 1. */
int mi_geo_lattice_sparsity(const int32_t P[3], const float* sigma, const uint8_t* mask, float scale, float* d_sigma, double* value_dev,
                            void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_GEO_H */
