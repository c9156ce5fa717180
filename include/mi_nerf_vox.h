/*
 * mi_nerf_vox.h -- C ABI of libmi_nerf_vox.so: a trained NeRF baked into a radiance grid, and frames rendered from the grid alone, on the
 * MI355X (gfx950).
 *
 * A library of its own BESIDE the path: include/mi_nerf.h and the other side headers stay what they are, nothing here is declared there,
 * and libmi_nerf_vox.so exports no symbol of the other libraries and links against none of them.  Same conventions: plain C99, raw device
 * pointers, the caller allocates everything, int status (0 = ok), hipStream_t passed as void*, every argument checked before any HIP call,
 * error text through mi_vox_last_error().  No entry synchronises with the host, copies, allocates, or uses an atomic.
 * All arithmetic below is fp32, every operation rounded once (no contraction), evaluated as it is written.
 *
 * THE LATTICE is the one of include/mi_nerf_mesh.h: res_i cells and P_i = res_i + 1 points per axis, 1 <= res_i <= MI_VOX_MAX_RES,
 *     step_i = (hi_i - lo_i) / (float)res_i,   x_i(j) = lo_i + (float)j_i * step_i,   flat(j) = (j_z * P_y + j_y) * P_x + j_x,
 * so the density lattice of that header, after a ReLU, is this grid's sigma plane.  inv_i = (float)res_i / (hi_i - lo_i).
 *
 * THE GRID.
 *   sigma   float [P_z, P_y, P_x], finite and >= 0.
 *   coef    float [P_z, P_y, P_x, R]: B = 1, 4 or 9 real spherical-harmonic functions (degree 0, 1, 2) per colour channel; coefficient b of
 *           channel c at 3 b + c; the record padded with zeros to R = mi_vox_record_floats(B) = 4 / 16 / 32 floats, so that a record is
 *           one aligned piece of 16 / 64 / 128 bytes.  The padding is written as zero and never read into a result.
 *   skip    uint8 [ceil(res_z / 8), ceil(res_y / 8), ceil(res_x / 8)], one byte per block of 8^3 cells: 0 iff sigma == 0 at every lattice
 *           point of the block's cells EXTENDED BY ONE CELL on every side (clipped to the lattice), i.e. at the points
 *           max(8 b_i - 1, 0) .. min(min(8 b_i + 8, res_i) + 1, res_i) per axis; 1 otherwise.
 *   THE COMPACT GRID keeps sigma and skip as they are and stores records only where the render rule can read one.
 *   active  a lattice point is active iff it or one of its 26 neighbours (clipped to the lattice) has sigma > 0.  The rule reads a record
 *           only when sigma_s > 0; weights are >= 0, so a corner of the sample's cell has sigma > 0, and all eight corners are then active.
 *   slot    int32 [P_z, P_y, P_x]: at an active point the number of active points with a smaller flat index, -1 at any other.  Record
 *           numbers follow flat lattice order: active x neighbours have consecutive slots.  M is the number of active points.
 *   table   M records, 16-byte aligned, in one of two formats:
 *           MI_VOX_FMT_F32  the R = 4 / 16 / 32 floats of the dense record, unchanged;
 *           MI_VOX_FMT_F16  the same R values as IEEE binary16 (8 / 32 / 64 bytes), converted from fp32 by round-to-nearest-even, a value
 *                           beyond the binary16 range becoming +-inf as that conversion gives it; the padding is zero.
 *   The compact render rule (mi_vox_render_sparse) is THE RENDER RULE with one change in step 3: corner e's record is table[slot[corner]],
 *   a binary16 record widened to fp32 (exactly) before any arithmetic.  A corner whose slot is < 0 or >= M contributes a zero record and
 *   loads nothing: a hand-made slot plane cannot make the renderer read outside the table.
 *   The basis at a unit vector (x, y, z):
 *       Y_0 = 0.28209479
 *       Y_1 = -0.48860251 y      Y_2 = 0.48860251 z      Y_3 = -0.48860251 x
 *       Y_4 = 1.0925484 (x y)    Y_5 = -1.0925484 (y z)  Y_6 = 0.31539157 (((2 z) z - x x) - y y)
 *       Y_7 = -1.0925484 (x z)   Y_8 = 0.54627422 (x x - y y)
 *
 * THE RENDER RULE (mi_vox_render), per ray (o, d) of rays [n, 6]:
 *   1. Slab.    L = sqrtf((d_x d_x + d_y d_y) + d_z d_z).  entry = -inf, exit = +inf; per axis in the order x, y, z: when d_i != 0,
 *               ta = (lo_i - o_i) / d_i, tb = (hi_i - o_i) / d_i, entry = fmaxf(entry, fminf(ta, tb)), exit = fminf(exit, fmaxf(ta, tb));
 *               when d_i == 0 the axis bounds nothing if lo_i <= o_i <= hi_i and makes the ray a miss otherwise.
 *               t0 = fmaxf(t_near, entry), t1 = fminf(t_far, exit).  A ray with a non-finite component, L == 0 or not t1 > t0 is a MISS:
 *               rgb = bg, acc = depth = disp = 0, visited = 0.
 *   2. Intervals.  dt = step / L.  For k = 0, 1, ... while a_k < t1 and k < mi_vox_max_steps(grid, step):
 *               a_k = t0 + (float)k * dt,  b_k = fminf(t0 + (float)(k + 1) * dt, t1),  m_k = 0.5f * (a_k + b_k),
 *               delta_k = (b_k - a_k) * L.
 *               The last interval is truncated at t1, not dropped and not overshot: the result is continuous in the ray.
 *   3. Sample.  p_i = o_i + m_k * d_i;  g_i = (p_i - lo_i) * inv_i;  c_i = min(max((int)floorf(g_i), 0), res_i - 1);
 *               f_i = fminf(fmaxf(g_i - (float)c_i, 0), 1).  Corner e = 0..7 is the lattice point c + (e & 1, (e >> 1) & 1, e >> 2) with
 *               weight w_e = (wx wy) wz, w = f_i on the far side of axis i and 1 - f_i on the near side.  Interpolation of a quantity q:
 *               v_e = w_e q_e, summed in pairs: x neighbours first, then y, then z:
 *               ((v_0 + v_1) + (v_2 + v_3)) + ((v_4 + v_5) + (v_6 + v_7)).
 *               sigma_s = the interpolation of sigma;  alpha_k = 1 - expf(-(sigma_s * delta_k)).
 *               Only when sigma_s > 0: with u = d / L and q_e[c] = sum over b of coef_e[3 b + c] * Y_b(u), in increasing b from
 *               coef_e[c] * Y_0, colour[c] = fminf(fmaxf(interpolation of q[c], 0), 1).  (Interpolation and the sum over b commute: this
 *               is the basis applied to the interpolated coefficients, evaluated corner by corner.)
 *   4. Compositing.  T = 1, sums 0.  w = T alpha_k;  rgb += w colour (skipped when sigma_s == 0);  acc += w;  depth += w m_k;
 *               T = T (1 - alpha_k).  Marching stops after a sample that leaves T < T_min (T_min = 0 never stops).  Then
 *               rgb += (1 - acc) bg, and disp as the path forms it from depth and acc: q = depth / acc, 1 / fmaxf(1e-10, q) with a NaN
 *               q kept, NaN -> 0, capped at 5.
 *               Unlike the path's compositing there is no 1e-10 inside the transmittance product and no 1e10 last interval: density at
 *               the far clip does not become opaque.
 *   5. Skipping.  With use_skip, a sample whose cell's block byte is 0 is not fetched: its eight sigma values are 0, so it adds exactly
 *               nothing.  The march may then jump ahead to a later k, never past a sample whose cell lies outside that block extended by
 *               one cell; positions are functions of the integer k alone, so rgb, disp, acc and depth are BIT-IDENTICAL with use_skip
 *               0 and 1.  visited counts the samples whose sigma was fetched; it is the only output that differs.  A ray whose fp32
 *               position error could reach an eighth of a cell (a far origin) never jumps.
 *
 * THE PROJECTION (mi_vox_project).  raw [M, D, 4] is a network's answer at M lattice points for D directions, proj [B, D] a matrix:
 *     sigma[index[m]] = fmaxf(raw[m, 0, 3], 0)                                    (a NaN becomes 0)
 *     coef[index[m], 3 b + c] = sum over j of proj[b, j] * s(raw[m, j, c]),  s(x) = 1 / (1 + expf(-x)),  in increasing j from 0;
 * the rest of the record is written as zero.  One thread writes one record; an index outside [0, P_x P_y P_z) is ignored; indices are
 * distinct.
 *
 * THE RESAMPLING RULE (mi_vox_resample) moves a grid's content to another lattice.  A source grid (lo_s, hi_s, res_s; sigma_s, coef_s) and
 * a destination grid with a lo_d, hi_d and res_d of its own -- another resolution, and if wanted another box -- share B.  For every
 * destination lattice point j, in THE LATTICE's arithmetic:
 *     x_i = lo_d,i + (float)j_i * step_d,i;   g_i = (x_i - lo_s,i) * inv_s,i;   c_i = min(max((int)floorf(g_i), 0), res_s,i - 1);
 *     f_i = fminf(fmaxf(g_i - (float)c_i, 0), 1);
 * corners, weights w_e = (wx wy) wz and the pairwise sum exactly as in step 3 of THE RENDER RULE: that step applied to the lattice point
 * itself, in the source grid.  A point outside the source box therefore takes the value at the nearest face (edge extension), and a
 * destination box inside the source box crops.
 *     sigma_d[j] = the interpolation of sigma_s;   coef_d[j][t] = the interpolation of coef_s[.][t] for each of the 3 B counted floats t;
 * each padding float of the destination record is written as zero, and no source padding is read into a result.  Every element of sigma_d
 * and coef_d is written; the source is not modified.  Trilinear interpolation reproduces a trilinear function, so on the same box a
 * res_d that is a multiple of res_s represents the identical field (up to rounding): refining does not change the picture.
 *
 * THE PRUNING RULE (mi_vox_prune), with a threshold tau >= 0: a lattice point is KEPT iff it or one of its 26 neighbours (clipped to the
 * lattice) has sigma_in > tau -- the active stencil above with a threshold; tau = 0 is exactly active.
 *     sigma_out[j] = kept ? sigma_in[j] : 0;   the record of a point that is not kept is written as R zeros, in place;
 * the record of a kept point is not written at all, and sigma_in is not modified.  Afterwards the records of the points that are not
 * active (under sigma_out) are zero: the state a bake leaves, which training by include/mi_nerf_voxgrad.h relies on and does not keep.
 * The result is bit-identical from run to run.
 *
 * PRUNING BY VISIBILITY: what no training camera sees with measurable transmittance is removed.  Three rules, all gathers and plain
 * stores: per view a volume of optical depth along the pixel rays, then every lattice point looks itself up in that volume and keeps the
 * minimum over the views, then the pruning stencil with a second condition on the seed.  A view is the pinhole camera of
 * include/mi_nerf_mesh.h (its Camera paragraph: H rows, W columns, fx, fy, cx, cy, c2w = (R | t) row-major, pixel (i, j) = column i,
 * row j) with a depth range cut into K slices: slice k covers the ray parameters depth_near + k depth_step .. depth_near + (k + 1)
 * depth_step (the parameter t of the pixel's ray x = o + t d, which is that header's camera depth z).
 *
 * THE SHADOW RULE (mi_vox_shadow), per pixel (column i, row j) of a view:
 *     a = ((float)i - cx) / fx,   b = -(((float)j - cy) / fy),   c = -1;     d_r = (R_r0 a + R_r1 b) + R_r2 c;     o = t;
 *     L = sqrtf((d_x d_x + d_y d_y) + d_z d_z);     delta = depth_step * L.
 * For k = 0 .. K - 1 in increasing order, with od_0 = 0:
 *     tvol[j][i][k] = od_k                            the optical depth BEFORE slice k
 *     m_k = depth_near + ((float)k + 0.5f) * depth_step;     p_i = o_i + m_k * d_i;
 *     sigma_s = step 3 of THE RENDER RULE at p (cell, clamps, weights, pairwise sum) when lo_i <= p_i <= hi_i on all three axes;
 *               otherwise 0, and nothing is fetched (a NaN p_i fails the comparison);
 *     od_{k+1} = od_k + sigma_s * delta.
 * With a skip plane, a sample whose cell's block byte is 0 takes sigma_s = 0 without a fetch: its eight values are 0, so tvol is
 * BIT-IDENTICAL with and without the plane.  Every element of tvol [H, W, K] is written.  There is no exponential anywhere: the rule
 * can be restated bit for bit.  exp(-od) is the transmittance with which the view sees the front of the slice.
 *
 * THE VISIBILITY RULE (mi_vox_seen), per lattice point x (THE LATTICE's arithmetic) and one view with its tvol:
 *     e_k = x_k - t_k;   q_i = (R_0i e_0 + R_1i e_1) + R_2i e_2;   z = -q_z;   sx = cx + (fx * q_x) / z;   sy = cy - (fy * q_y) / z;
 *     fi = rintf(sx),  fj = rintf(sy)                 (ties to even: the nearest pixel)
 * The point is LOOKED AT iff z > 0, z is finite, 0 <= fi <= (float)(W - 1) and 0 <= fj <= (float)(H - 1), compared as floats (a NaN
 * fails).  A point that is not looked at is left alone.  Otherwise
 *     k = (int)floorf((z - depth_near) / depth_step) - bias          (formed without overflow: a quotient beyond +-2^40 counts as that)
 *     k < 0: od = 0;     k >= K: the point is left alone;     otherwise od = tvol[(int)fj][(int)fi][k];
 *     od_plane[x] = fminf(od_plane[x], od).
 * The caller fills od_plane with +inf and runs one mi_vox_shadow + mi_vox_seen pair per view, on one stream, through the same tvol.  A
 * minimum does not depend on the order of the views, and each element is read and written by one thread: no atomic, bit-identical from
 * run to run.  Afterwards od_plane is the smallest optical depth under which any view sees the point, +inf where none looks.  bias is
 * the shadow-map bias in slices: a point is not to be hidden by the shell of density it belongs to.
 *
 * THE SEEN PRUNING RULE (mi_vox_prune_seen), with tau >= 0 and od_max >= 0: a lattice point is a SEED iff sigma_in > tau and
 * od_plane <= od_max (a NaN od fails); it is KEPT iff it or one of its 26 neighbours (clipped to the lattice) is a seed.  The writes are
 * THE PRUNING RULE's.  With od_max = +inf and an od_plane without NaN the result is that rule's bit for bit.
 *
 * THE RAY GRADIENT RULE (mi_vox_render_backward_rays, mi_vox_render_sparse_backward_rays): the derivative of THE RENDER RULE's rgb, acc
 * and depth with respect to the ray, d_rays [n, 6] = dLoss/d(o, d), under upstream gradients G[3] of rgb, ga of acc and gd of depth (an
 * absent array is all zeros; disp carries nothing).  It is the exact derivative away from the rule's kinks: a sample crossing a cell
 * boundary, a change in the number of intervals, a change of the slab axis that gives entry or exit, the colour clamp, the clamps of c_i
 * and f_i; at a kink it is one of the one-sided values.  The stop at T_min, the bound on k, t_near and t_far are treated as fixed.  All
 * three storages are differentiated: a record is fetched as the render rule (or the compact render rule) fetches it.
 * (G . x) stands for (G[0] x[0] + G[1] x[1]) + G[2] x[2]; every sum below runs in increasing k, over the corners as step 3's pairwise
 * sum, and in increasing b.
 *   Forward.   Steps 1 to 5 as written above, sample by sample; T_k is the transmittance BEFORE sample k, w_k = T_k alpha_k.  The
 *              colour is evaluated only where sigma_s > 0, as the renderer does; elsewhere q_e[c] = q_k[c] = colour_k[c] = 0 below.
 *              ga' = ga - (G . bg);   s_k = ((G . colour_k) + ga') + gd * m_k;   S = sum of w_k * s_k;   P_k = the same sum over j < k.
 *   Sample k.  E_k = T_k * s_k - (S - P_k);   D_k = delta_k * E_k (dLoss/d sigma_s);   Z_k = sigma_s * E_k (dLoss/d delta_k);
 *              Q_k[c] = w_k * G[c] where sigma_s > 0 and 0 <= q_k[c] <= 1 (q_k[c] the interpolation of q_e[c] BEFORE the clamp), else 0;
 *              h_e = D_k * sigma_e + (Q_k . q_e)                         per corner, q_e corner e's own colour before the weight;
 *              v_e,x = +-(wy * wz), v_e,y = +-(wx * wz), v_e,z = +-(wx * wy): + on the far side of the axis, - on the near side, and 0
 *              on an axis where g_i - (float)c_i lies outside [0, 1] (the clamp of f_i is active);
 *              gp_i = inv_i * (the pairwise sum over the corners of v_e,i * h_e)           (dLoss/dp_i at the sample)
 *              go_i += gp_i;   gd_i += m_k * gp_i;   M_k = (d . gp) + gd * w_k             (dLoss/dm_k)
 *              an interval that is not cut (not t1 < t0 + (float)(k + 1) * dt):   g_t0 += M_k;   g_dt += ((float)k + 0.5f) * M_k;
 *              the cut last interval:   r = 0.5f * M_k - L * Z_k;   g_t0 += r;   g_dt += (float)k * r;   g_t1 += 0.5f * M_k + L * Z_k;
 *                                       g_L += (t1 - a_k) * Z_k;
 *              y_e,b += (Q_k . (w_e * coef_e[3 b + .]))                  per corner and b: the corner's share of dLoss/dY_b.
 *   The end.   gY_b = the pairwise sum over the corners of y_e,b;  du = sum over b >= 1 of gY_b * grad Y_b(u), the basis differentiated
 *              as the polynomials written above, component by component in increasing b, each term as (constant * u_j) * gY_b
 *              (degree 1: constant * gY_b; the doubled constants 0.63078314, 1.26156628, 1.09254844 for Y_6 and Y_8);
 *              gd_i = ((gd_i + (du_i - u_i * (u . du)) / L) + (g_dt * -(step / ((L * L) * L))) * d_i) + (g_L / L) * d_i;
 *              when entry > t_near, with i the first axis that attains entry:  r = g_t0 / d_i;  go_i -= r;  gd_i -= r * t0;
 *              when exit < t_far, with i the first axis that attains exit:     r = g_t1 / d_i;  go_i -= r;  gd_i -= r * t1.
 *              d_rays = (go, gd).  A MISS gives six zeros.
 * d_rays is WRITTEN, not added; one lane stores a ray's six floats and no other ray touches them: no atomic, BIT-IDENTICAL from run to
 * run.  A sample whose eight sigma_e are all 0 contributes exactly nothing (h_e = 0, w_k = 0, Z_k = 0), so the march jumps over empty
 * blocks exactly as step 5 lets the renderer: d_rays with use_skip 0 and 1 are EQUAL.  The check outputs rgb_check, acc_check and
 * depth_check receive the forward values, the renderer's own bit for bit.  expf is the one operation a restatement in another fp32
 * arithmetic cannot be held to bit for bit, as in the render rule.
 *
 * A SIGNED GRID (mi_vox_build_skip_signed, mi_vox_render_signed, mi_vox_render_sparse_signed) stores the density BEFORE its ReLU and
 * applies the ReLU after the interpolation.  The zero crossing of a trilinear function can lie anywhere inside a cell, so a surface is
 * no longer bound to lattice planes and a cell with one dense corner is no longer fogged; a negative value is "empty, with headroom".
 *   sigma   float [P_z, P_y, P_x], finite, of any sign.  coef, the compact grid's slot and table, and active are what they are above.
 *   render  Step 3 of THE RENDER RULE becomes sigma_s = fmaxf(the interpolation of sigma, 0).  Everything else of steps 1 to 5 stays
 *           word for word; the compact render rule changes in the same one place.
 *   skip    the signed skip plane's byte is 0 iff sigma <= 0 at every lattice point of the block's cells extended by one cell: the points
 *           of THE GRID's skip, the test sigma > 0 in the place of sigma != 0.
 *   Skipping stays exact.  Weights are >= 0, so a sample whose eight corners are <= 0 interpolates to a value <= 0 and has sigma_s = 0:
 *           it adds exactly nothing.  The jump never passes a sample whose cell lies outside the block extended by one cell.  So rgb,
 *           disp, acc and depth are BIT-IDENTICAL with use_skip 0 and 1, and visited is the only output that differs.
 *   On a plane that is >= 0 everywhere fmaxf(x, 0) = x: every output of the three entries, visited and the skip plane included, is
 *           bit-identical to that of mi_vox_build_skip, mi_vox_render and mi_vox_render_sparse.
 *   There is no gain factor: the plane is in the units of sigma.
 * The rest of the tool chain reads a signed plane as it is:
 *   Activity and compact storage.  A sample with sigma_s > 0 has a corner with sigma > 0 (weights are >= 0), so all eight corners are
 *           active (mi_vox_index tests sigma > 0): the compact signed renderer equals the dense signed renderer bit for bit.
 *   mi_vox_prune at tau = 0.  A point that is not kept has sigma <= 0 itself and at its 26 neighbours, so every corner of every cell it
 *           touches is <= 0 before and after: every sample there has sigma_s = 0 either way, and no output bit changes.
 *   Invisible negatives.  A point that is <= 0 with all 26 neighbours <= 0 may hold any negative number without changing a bit of any
 *           render, for the same reason.
 *   mi_vox_resample is linear in sigma: an integer refinement on the same box represents the identical field (up to rounding), and the
 *           ReLU is applied to it afterwards as before.
 * THE SHADOW RULE, THE VISIBILITY RULE, THE SEEN PRUNING RULE and THE RAY GRADIENT RULE read sigma without the ReLU: they are not defined
 * on a signed plane.
 */
#ifndef MI_NERF_VOX_H
#define MI_NERF_VOX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_VOX_ABI_VERSION 2

/* status codes (the values of mi_nerf.h) */
#define MI_VOX_OK 0
#define MI_VOX_EINVAL 1   /* bad argument / unsupported shape */
#define MI_VOX_EHIP 2     /* HIP runtime error */

#define MI_VOX_MAX_RES 512        /* largest res[i] */
#define MI_VOX_BLOCK 8            /* cells per axis of one skip block */
#define MI_VOX_MAX_DIRS 256       /* largest D of mi_vox_project */
#define MI_VOX_MAX_STEPS 65536    /* largest mi_vox_max_steps that mi_vox_render takes */
#define MI_VOX_FMT_F32 0          /* record formats of THE COMPACT GRID */
#define MI_VOX_FMT_F16 1

int mi_vox_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_vox_last_error(void);

/* Axis-aligned box cut into res[0] x res[1] x res[2] cells (x, y, z).  lo_i < hi_i, both finite, with a finite fp32 step > 0. */
typedef struct mi_vox_grid {
    float lo[3];
    float hi[3];
    int32_t res[3];
} mi_vox_grid;

/* What a render reads beside the grid and the rays.  step > 0 is the world length of an interval; t_near < t_far, not NaN (they may be
 * infinite); 0 <= T_min < 1; bg finite; use_skip 0 or 1. */
typedef struct mi_vox_render_cfg {
    float step;
    float t_near, t_far;
    float T_min;
    float bg[3];
    int32_t use_skip;
} mi_vox_render_cfg;

/* The two sizes a caller needs: floats per record (4 / 16 / 32 for B = 1 / 4 / 9, 0 for any other B) and bytes of the skip plane
 * (0 + error text if the grid is refused). */
int mi_vox_record_floats(int B);
size_t mi_vox_skip_bytes(const mi_vox_grid* grid);
/* The bound on the samples of one ray: ceil(|hi - lo| / step) + 1, |hi - lo| the box's diagonal, formed in double.  0 + error text if
 * the grid is refused or step is not a positive finite number. */
int64_t mi_vox_max_steps(const mi_vox_grid* grid, float step);

/* THE PROJECTION.  B <= D <= MI_VOX_MAX_DIRS; raw_dev and coef_dev 16-byte aligned, index_dev (int64) 8-byte aligned; M >= 0 (0: nothing
 * is launched and the arrays are not looked at).  sigma_dev may be NULL: the density is then not written (a caller that filled the sigma plane from a density lattice). */
int mi_vox_project(const mi_vox_grid* grid, int B, int D, const float* raw_dev, const float* proj_dev, const int64_t* index_dev, int64_t M,
                   float* sigma_dev, float* coef_dev, void* stream);

/* skip from sigma by the rule of THE GRID. */
int mi_vox_build_skip(const mi_vox_grid* grid, const float* sigma_dev, uint8_t* skip_dev, void* stream);

/* THE RENDER RULE.  rays [n, 6], rgb [n, 3]; disp, acc, depth [n] float and visited [n] uint32 may each be NULL; skip_dev may be NULL when
 * use_skip is 0; coef_dev 16-byte aligned; n >= 0 (0: nothing is launched and the arrays are not looked at).  Refused when mi_vox_max_steps exceeds MI_VOX_MAX_STEPS. */
int mi_vox_render(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev, const float* rays_dev,
                  int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev,
                  uint32_t* visited_dev, void* stream);

/* THE COMPACT GRID.  Bytes of one record of the table: 16 / 64 / 128 for MI_VOX_FMT_F32, 8 / 32 / 64 for MI_VOX_FMT_F16; 0 for any other
 * B or fmt. */
size_t mi_vox_record_bytes(int B, int fmt);

/* slot and M from sigma: per-workgroup counts of the active flag, an exclusive scan of the counts, the slot write -- deterministic, the
 * sums in LDS.  slot_dev int32 [P_z, P_y, P_x] 4-byte aligned, count_dev one int64 (8-byte aligned) that receives M, scratch_dev 16-byte
 * aligned with at least mi_vox_index_scratch_bytes(grid) bytes (0 + error text if the grid is refused).  The caller reads count_dev back. */
size_t mi_vox_index_scratch_bytes(const mi_vox_grid* grid);
int mi_vox_index(const mi_vox_grid* grid, const float* sigma_dev, int32_t* slot_dev, int64_t* count_dev, void* scratch_dev, size_t scratch_bytes,
                 void* stream);

/* The table from fp32 records, in format fmt.  With slot_dev, src_dev is a dense coef array [P_z, P_y, P_x, R]: the record of every point
 * with 0 <= slot < M goes to table[slot].  With slot_dev NULL, src_dev is M fp32 records, converted one to one.  src_dev and table_dev
 * 16-byte aligned; M >= 0 (0: nothing is launched and the arrays are not looked at). */
int mi_vox_pack(const mi_vox_grid* grid, int B, int fmt, const float* src_dev, const int32_t* slot_dev, int64_t M, void* table_dev, void* stream);

/* The compact render rule.  Everything as mi_vox_render, with slot_dev (4-byte aligned) and table_dev (16-byte aligned; may be NULL when
 * M is 0) in the place of coef_dev. */
int mi_vox_render_sparse(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev, int64_t M,
                         const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev,
                         float* acc_dev, float* depth_dev, uint32_t* visited_dev, void* stream);

/* THE RESAMPLING RULE, dense fp32 grids (added within ABI 2: nothing earlier changed).  sigma_src_dev [P_z, P_y, P_x] and coef_src_dev
 * [P_z, P_y, P_x, R] of src, sigma_dst_dev and coef_dst_dev of dst; the coef arrays 16-byte aligned, none NULL.  Refused when a
 * destination array shares a byte with a source array or with the other destination array. */
int mi_vox_resample(const mi_vox_grid* src, const mi_vox_grid* dst, int B, const float* sigma_src_dev, const float* coef_src_dev, float* sigma_dst_dev,
                    float* coef_dst_dev, void* stream);

/* THE PRUNING RULE.  tau finite and >= 0; sigma_out_dev must not be sigma_in_dev (refused: the stencil reads a point's neighbours);
 * coef_dev [P_z, P_y, P_x, R], 16-byte aligned, is edited in place.  The caller rebuilds the skip plane from sigma_out_dev. */
int mi_vox_prune(const mi_vox_grid* grid, int B, float tau, const float* sigma_in_dev, float* sigma_out_dev, float* coef_dev, void* stream);

/* PRUNING BY VISIBILITY (added within ABI 2: nothing earlier changed).  One view: the camera and its slices. */
typedef struct mi_vox_view {
    int32_t H, W;              /* 1 .. 8192 */
    float fx, fy, cx, cy;      /* finite; fx and fy not 0 */
    float c2w[12];             /* [3,4] row-major (R | t), finite */
    float depth_near;          /* finite, >= 0 */
    float depth_step;          /* finite, > 0: the depth of one slice, in units of the pixel ray's parameter t (= camera depth) */
    int32_t slices;            /* K: a multiple of 8, 8 .. MI_VOX_MAX_STEPS */
} mi_vox_view;

/* Bytes of a view's tvol: H * W * K * 4 (0 + error text if the view is refused). */
size_t mi_vox_shadow_bytes(const mi_vox_view* view);

/* THE SHADOW RULE.  tvol_dev float [H, W, K], 32-byte aligned, every element written; skip_dev may be NULL (no plane is used).  Refused
 * when tvol shares a byte with sigma. */
int mi_vox_shadow(const mi_vox_grid* grid, const float* sigma_dev, const uint8_t* skip_dev, const mi_vox_view* view, float* tvol_dev, void* stream);

/* THE VISIBILITY RULE.  od_dev float [P_z, P_y, P_x] is read and written; bias >= 0.  Refused when od shares a byte with tvol. */
int mi_vox_seen(const mi_vox_grid* grid, const mi_vox_view* view, const float* tvol_dev, int32_t bias, float* od_dev, void* stream);

/* THE SEEN PRUNING RULE.  Everything as mi_vox_prune, with od_max >= 0 (it may be +inf, not NaN) and od_dev float [P_z, P_y, P_x], which
 * is read only and shares no byte with sigma_out_dev or coef_dev. */
int mi_vox_prune_seen(const mi_vox_grid* grid, int B, float tau, float od_max, const float* sigma_in_dev, const float* od_dev, float* sigma_out_dev,
                      float* coef_dev, void* stream);

/* THE RAY GRADIENT RULE (added within ABI 2: nothing earlier changed).  grid, B, sigma_dev, coef_dev, skip_dev, rays_dev, n and cfg as
 * mi_vox_render takes them, with its NULL, alignment and n == 0 conventions.  g_rgb_dev [n, 3]; g_acc_dev and g_depth_dev [n] may each be
 * NULL (zeros); d_rays_dev [n, 6] is written and shares no byte with rays_dev; rgb_check_dev [n, 3], acc_check_dev and depth_check_dev [n]
 * may each be NULL.  Every float array 4-byte aligned. */
int mi_vox_render_backward_rays(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev,
                                const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, const float* g_rgb_dev, const float* g_acc_dev,
                                const float* g_depth_dev, float* d_rays_dev, float* rgb_check_dev, float* acc_check_dev, float* depth_check_dev,
                                void* stream);

/* The same for THE COMPACT GRID: fmt, slot_dev, table_dev and M as mi_vox_render_sparse takes them. */
int mi_vox_render_sparse_backward_rays(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev,
                                       int64_t M, const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg,
                                       const float* g_rgb_dev, const float* g_acc_dev, const float* g_depth_dev, float* d_rays_dev, float* rgb_check_dev,
                                       float* acc_check_dev, float* depth_check_dev, void* stream);

/* A SIGNED GRID (added within ABI 2: nothing earlier changed).  Each entry takes the arguments of its unsigned counterpart -- of
 * mi_vox_build_skip, mi_vox_render and mi_vox_render_sparse in this order -- with the same NULL, alignment and n == 0 conventions and the
 * same refusals; sigma_dev is a signed plane and skip_dev a signed skip plane. */
int mi_vox_build_skip_signed(const mi_vox_grid* grid, const float* sigma_dev, uint8_t* skip_dev, void* stream);

int mi_vox_render_signed(const mi_vox_grid* grid, int B, const float* sigma_dev, const float* coef_dev, const uint8_t* skip_dev, const float* rays_dev,
                         int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev,
                         uint32_t* visited_dev, void* stream);

int mi_vox_render_sparse_signed(const mi_vox_grid* grid, int B, int fmt, const float* sigma_dev, const int32_t* slot_dev, const void* table_dev, int64_t M,
                                const uint8_t* skip_dev, const float* rays_dev, int64_t n, const mi_vox_render_cfg* cfg, float* rgb_dev,
                                float* disp_dev, float* acc_dev, float* depth_dev, uint32_t* visited_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_VOX_H */
