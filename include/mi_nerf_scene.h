/*
 * mi_nerf_scene.h -- C ABI of libmi_nerf_scene.so: procedural solid-object scenes for the MI355X (gfx950) NeRF path.
 *
 * A library of its own BESIDE the path: include/mi_nerf.h, include/mi_nerf_occ.h and their libraries stay what they are, nothing here is
 * declared there, and libmi_nerf_scene.so exports no mi_nerf_*, mi_occ_* or mi_iqa_* symbol.  It includes no other header of the project
 * and links against no other library of it.  Same conventions: plain C99, raw device pointers, the caller allocates everything, int
 * status (0 = ok), hipStream_t passed as void*, every argument checked before any HIP call, error text through mi_scene_last_error().
 *
 * A SCENE is a short list of opaque solids (spheres, axis-aligned boxes, capped axis-aligned cylinders) in empty space.  It answers the
 * question a NeRF network answers -- raw (r, g, b, sigma) at a point -- in closed form, so it stands in for a network wherever the staged
 * tools take one (mi_scene_field_rays has the tensor shapes of mi_nerf_mlp_rays), and mi_scene_render forms the image of it through the
 * reference's own image-formation model (post_process, nerf_process.py:89-140): ground truth to train on and to measure against.
 *
 * THE FIELD RULE (mi_scene_field_rays is its public statement; all arithmetic fp32, every operation rounded once, no contraction):
 *     p_i = o_i + d_i * z                   product rounded, then sum rounded (nerf_process.py:69-70)
 *     q_i = p_i - c_i                       per primitive, c its centre
 *     sphere   : inside iff (q_x*q_x + q_y*q_y) + q_z*q_z <= r*r                       r = h[0]
 *     box      : inside iff fabsf(q_i) <= h_i for i = x, y, z
 *     cylinder : inside iff fabsf(q_axis) <= h[1] and q_b*q_b + q_c*q_c <= h[0]*h[0]   b < c the two other axes
 *     (a NaN coordinate is outside: every comparison with it is false)
 *     The FIRST primitive in list order that contains p gives raw = (rgb_raw[colour][0..2], sigma), with
 *         colour = 0                                      if freq == 0
 *         colour = ((int)k_x + (int)k_y + (int)k_z) & 1   if freq > 0, k_i = floorf(q_i * freq)   (a checker in the primitive's own frame;
 *                                                          two's complement, so -1 & 1 = 1; |q_i * freq| is assumed below 2^31)
 *     No primitive contains p: raw = (0, 0, 0, 0) -- the zero post_process turns into weight 0 exactly.
 */
#ifndef MI_NERF_SCENE_H
#define MI_NERF_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SCENE_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_SCENE_OK 0
#define MI_SCENE_EINVAL 1   /* bad argument / unsupported shape */
#define MI_SCENE_EHIP 2     /* HIP runtime error */

#define MI_SCENE_MAX_PRIMS 16     /* primitives of one scene */
#define MI_SCENE_MAX_SAMPLES 4096 /* largest S of mi_scene_render */

#define MI_SCENE_SPHERE 0
#define MI_SCENE_BOX 1
#define MI_SCENE_CYLINDER 2

int mi_scene_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_scene_last_error(void);

/* One solid, 64 bytes.  A scene is an array of 1 .. MI_SCENE_MAX_PRIMS of them IN HOST MEMORY: every entry copies it into its kernel's
 * arguments, nothing of it has to live on the device. */
typedef struct mi_scene_prim {
    int32_t kind;          /* MI_SCENE_SPHERE / _BOX / _CYLINDER */
    int32_t axis;          /* cylinder: its axis, 0 = x, 1 = y, 2 = z.  0, 1 or 2 for every kind (not read for the others) */
    float c[3];            /* centre, finite */
    float h[3];            /* box: half-extents.  sphere: h[0] radius.  cylinder: h[0] radius, h[1] half-height.  Every entry the kind reads
                              is finite and > 0 (and its square is finite); the others are not read */
    float sigma;           /* raw density inside, finite, > 0 */
    float rgb_raw[2][3];   /* two colours as raw logits: what sigmoid in post_process consumes.  finite */
    float freq;            /* 0: solid colour 0.  > 0: checker of colours 0 and 1 with cells of 1 / freq.  finite, >= 0 */
} mi_scene_prim;

/* Validation alone (host): MI_SCENE_OK, or MI_SCENE_EINVAL with a text that names the primitive and the field. */
int mi_scene_check(const mi_scene_prim* prims, int n_prims);

/* rays [n,6] (o, d), z [n,S] -> raw [n,S,4] under THE FIELD RULE: the shapes of mi_nerf_mlp_rays, so a scene is a stand-in "network" for
 * the staged path (raw -> mi_nerf_composite).  One thread per sample, one 16-byte store.  raw_dev 16-byte aligned; n >= 0, S >= 1,
 * n * S < 2^39. */
int mi_scene_field_rays(const mi_scene_prim* prims, int n_prims, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                        float* raw_dev, void* stream);

/* The ground-truth renderer, fused: rays [n,6] -> rgb [n,3], disp [n], acc [n], depth [n]; disp_dev, acc_dev and depth_dev may be NULL.
 * Depths are the bin centres, without jitter:
 *     step = (far - near) / (float)S        fp32, on the host
 *     z_k  = near + ((float)k + 0.5f) * step,   k = 0 .. S - 1
 * Per sample THE FIELD RULE, then post_process (nerf_process.py:89-140) as mi_nerf_composite states it: dist_k = z_{k+1} - z_k, 1e10 for
 * the last sample, times |d|; alpha = 1 - expf(-relu(sigma) * dist); weight = alpha * T with the exclusive transmittance
 * T = prod (1 - alpha + 1e-10); rgb = sum weight * sigmoid(rgb_raw) + (1 - acc) (white background, always); depth = sum weight * z;
 * disp = 1 / max(1e-10, depth / acc) with NaN -> 0, clamped to 5.  S == 1 renders white with acc 0, as the reference's slice of an empty
 * distance tensor does (and as mi_nerf_composite does).  The result is mi_scene_field_rays on these z_k followed by mi_nerf_composite up
 * to summation order.  A ray that meets no primitive gives rgb (1, 1, 1), acc 0, depth 0, disp 0 exactly.
 * One ray per lane, samples in sequence; nothing goes through device memory but the rays in and the four outputs out.
 * near < far, both finite; 1 <= S <= MI_SCENE_MAX_SAMPLES; n >= 0, n < 2^39.  n == 0: nothing is launched, and the device pointers (of
 * mi_scene_field_rays too) may be NULL, as those of empty buffers are. */
int mi_scene_render(const mi_scene_prim* prims, int n_prims, const float* rays_dev, int64_t n_rays, float near_, float far_, int S,
                    float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_SCENE_H */
