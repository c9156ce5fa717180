/*
 * mi_nerf_occ.h -- C ABI of libmi_nerf_occ.so: occupancy-grid rendering for the MI355X (gfx950) NeRF path.
 *
 * A library of its own ON TOP of the path: include/mi_nerf.h stays what it is, nothing here is declared there, and libmi_nerf_occ.so
 * exports no mi_nerf_* symbol.  It links against libmi_nerf.so (rpath $ORIGIN) and runs the networks and the stages ONLY through public
 * entries of that library: mi_nerf_mlp_rays / mi_nerf_mlp_rays_f16s / mi_nerf_mlp_rays_bf16 for the networks, mi_nerf_fill_uniform,
 * mi_nerf_stratified_z, mi_nerf_composite and mi_nerf_fine_z for the stages.  Same conventions: plain C99, raw device pointers, the caller
 * allocates everything, int status (0 = ok), hipStream_t passed as void*, every argument checked before any HIP call, error text through
 * mi_occ_last_error().
 *
 * SEMANTICS.  A sample that the grid marks empty is not evaluated: its raw network output is (0, 0, 0, 0).  post_process then gives it
 * alpha = 1 - exp(-relu(0) * dist) = 0 exactly (nerf_process.py:97-104), so it has weight 0.  The occupancy render is therefore the
 * staged reference path (stratified depths | network | composite | resample | network | composite) with raw zeroed at the samples
 * mi_occ_mark() answers 0 for, and every other number untouched.  With a grid that is conservative for the network the result is the
 * full render.
 *
 * THE CELL RULE (mi_occ_mark is its public statement; all arithmetic fp32, no contraction):
 *     p_i     = o_i + d_i * z                 product rounded, then sum rounded (nerf_process.py:69-70)
 *     scale_i = (float)res_i / (hi_i - lo_i)  fp32 difference, fp32 division, computed on the host
 *     c_i     = floorf((p_i - lo_i) * scale_i)
 *     inside  = 0 <= c_i < res_i for i = x, y, z   (a NaN coordinate is outside)
 *     inside : the sample is evaluated iff bit (c_z * res_y + c_y) * res_x + c_x is set (bit b: word b / 32, bit b % 32 of uint32 words)
 *     outside: the sample is evaluated iff grid.outside_occupied != 0
 * The grid lives in whatever space the rays live in: NDC rays (mi_nerf_ndc_rays) work unchanged with a box in NDC.
 */
#ifndef MI_NERF_OCC_H
#define MI_NERF_OCC_H

#include <stddef.h>
#include <stdint.h>

#include "mi_nerf.h"   /* mi_nerf_net, mi_nerf_render_cfg, MI_NERF_MODE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OCC_ABI_VERSION 2

/* status codes (the values of mi_nerf.h) */
#define MI_OCC_OK 0
#define MI_OCC_EINVAL 1   /* bad argument / unsupported shape or mode */
#define MI_OCC_EHIP 2     /* HIP runtime error, or a failed call into libmi_nerf.so (its text is carried over) */

#define MI_OCC_MAX_RES 512      /* largest res[i] */
#define MI_OCC_MAX_SUB 4        /* largest bake sub-lattice per cell and axis */
#define MI_OCC_MAX_RADIUS 2     /* largest dilation radius */
#define MI_OCC_TILE 32          /* samples of one compacted tile: one pseudo-ray of the network launch */

int mi_occ_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_occ_last_error(void);

/* Axis-aligned box [lo, hi) cut into res[0] x res[1] x res[2] cells (x, y, z), one bit per cell.  lo_i < hi_i, both finite;
 * 1 <= res_i <= MI_OCC_MAX_RES. */
typedef struct mi_occ_grid {
    float lo[3];
    float hi[3];
    int32_t res[3];
    int32_t outside_occupied;   /* samples outside the box: != 0 evaluated (conservative), 0 skipped */
} mi_occ_grid;

/* uint32 words of the bitfield: ceil(res_x res_y res_z / 32); 0 (and an error text) if the grid is refused. */
size_t mi_occ_grid_words(const mi_occ_grid* grid);

/* ------------------------------------------------------------------------------------------------
 * Baking.  The density of ONE network on a regular sub^3 lattice of every cell, 1 <= sub <= MI_OCC_MAX_SUB: with
 *     step_i = (hi_i - lo_i) / (float)(res_i * sub)     (fp32, on the host)
 * lattice point (jx, jy, jz), 0 <= j_i < res_i * sub, lies at lo_i + ((float)j_i + 0.5f) * step_i -- the points
 * lo + (i + (a + 1/2) / sub) * cell of cell i = j / sub, a = j % sub.  A lattice row along x is laid out as ONE ray: origin
 * (lo_x, y_jy, z_jz), direction (1, 0, 0), depths ((float)jx + 0.5f) * step_x; row (jy, jz) is ray jz * (res_y * sub) + jy.  The rows
 * run through the public fused entry of `mode` in slabs as large as the scratch allows (below 2^31 points each), and a cell's bit is set iff any of its sub^3
 * samples has raw density (channel 3 of the network output, before the ReLU) > sigma_min; a NaN density does not set a bit.
 * accumulate == 0: the bitfield is cleared first; != 0: the new bits are ORed into it (coarse and fine network sharing one grid).
 * mode: MI_NERF_MODE_F32 / _F16S / _BF16 -- the blob is the one of that family's packer, as for mi_nerf_mlp_rays*.
 * No host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
/* Smallest scratch mi_occ_bake accepts (one slab of about 4M lattice points, or the whole lattice if smaller); 0 + error text if refused. */
size_t mi_occ_bake_scratch_bytes(const mi_occ_grid* grid, int sub);
int mi_occ_bake(const mi_occ_grid* grid, uint32_t* bits_dev, const mi_nerf_net* net, const void* packed_dev, int mode, int sub,
                float sigma_min, int accumulate, void* scratch_dev, size_t scratch_bytes, void* stream);

/* out bit = OR of the in bits of the (2 radius + 1)^3 cells around it that lie inside the grid (radius 1: the cell and its 26
 * neighbours), 0 <= radius <= MI_OCC_MAX_RADIUS: makes a sampled grid conservative.  Out of place: bits_out_dev != bits_in_dev. */
int mi_occ_dilate(const mi_occ_grid* grid, const uint32_t* bits_in_dev, uint32_t* bits_out_dev, int radius, void* stream);

/* count_dev[0] (uint64 on the device) = number of set bits among the grid's cells. */
int mi_occ_count(const mi_occ_grid* grid, const uint32_t* bits_dev, uint64_t* count_dev, void* stream);

/* rays [n,6] (o, d), z [n,S] -> mask [n,S] uint8: 1 where the sample is evaluated under THE CELL RULE above, 0 where it is skipped. */
int mi_occ_mark(const mi_occ_grid* grid, const uint32_t* bits_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                uint8_t* mask_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The compaction as an entry of its own, with a REPRODUCIBLE tile order -- what the training path (occupancy_train.py) is built on: it
 * drives the networks itself (mi_nerf_mlp_rays_train / mi_nerf_mlp_backward on the tiles as pseudo-rays with S = 32) between these entries.
 * THE COMPACTION RULE (THE CELL RULE above decides what survives):
 *     ray r has k_r survivors, in sample order, and owns t_r = ceil(k_r / 32) tiles starting at base_r = sum of t_q over q < r
 *     tile base_r + j holds survivors 32 j .. 32 j + 31: tile_z their depths, tile_src = r * S + s; the padding lanes of a ray's last tile
 *     repeat the ray's last surviving depth and carry tile_src = -1
 *     slot[r, s] = 32 * (base_r + j) + lane of a survivor, -1 of a skipped sample;  tile_rays[base_r + j] = rays[r]
 *     counts_dev (uint32 [2]) = (sum of t_r, sum of k_r)
 * Three passes -- count (one wave per ray), exclusive scan of t_r, emit -- and NO atomic: every output is a function of the input, so two
 * calls give identical bytes.  The caller sizes tile_rays [T,6], tile_z [T,32], tile_src int32 [T,32] for T = n_rays * ceil(S / 32) tiles;
 * only the first counts[0] tiles are written.  1 <= S <= 1024, n_rays * ceil(S / 32) * 32 < 2^31.  scratch_dev: 256-byte aligned,
 * mi_occ_compact_scratch_bytes(n_rays) bytes (0 + error text if n_rays is refused).  NO host synchronisation: the entry may be recorded
 * into a graph; reading counts_dev is the caller's.  n_rays == 0 writes counts = (0, 0) and nothing else.
 * ---------------------------------------------------------------------------------------------- */
size_t mi_occ_compact_scratch_bytes(int64_t n_rays);
int mi_occ_compact(const mi_occ_grid* grid, const uint32_t* bits_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                   float* tile_rays_dev, float* tile_z_dev, int32_t* tile_src_dev, int32_t* slot_dev, uint32_t* counts_dev, void* scratch_dev,
                   size_t scratch_bytes, void* stream);

/* tile_vals [T,32,4], slot int32 [n,S] -> out [n,S,4]: EVERY element is written, tile_vals[slot] of a survivor, (0,0,0,0) where slot = -1.
 * Same size limits as mi_occ_compact; tile_vals_dev and out_dev 16-byte aligned. */
int mi_occ_scatter_raw(const float* tile_vals_dev, const int32_t* slot_dev, int64_t n_rays, int S, float* out_dev, void* stream);

/* The inverse, for the gradient of raw: src [n,S,4], tile_src int32 [T,32] -> out [T,32,4] = src[tile_src] per lane, exact zeros where
 * tile_src = -1.  A padding lane evaluates a real point with d_raw = 0 and so adds exactly zero to every weight-gradient and bias sum.
 * n_tiles * 32 < 2^31; src_dev and out_dev 16-byte aligned. */
int mi_occ_gather_raw(const float* src_dev, const int32_t* tile_src_dev, int64_t n_tiles, float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * render_rays with a grid.  The arguments of mi_nerf_render_rays plus the grid, one bitfield per network (bits_coarse_dev and
 * bits_fine_dev may be the same pointer) and host statistics.  Per network pass:
 *   1. cull + compact  one wave per ray: each lane looks its sample up, a ballot and a prefix count compact the surviving depths in
 *                      order, padded to a multiple of MI_OCC_TILE with the ray's last survivor; emitted as tiles rays'[n',6],
 *                      z'[n',32] with a source index per lane (ray * S + sample; -1: padding).  The tile count n' reaches the host
 *                      through a pinned 8-byte copy and a stream synchronisation (mi_nerf_mlp_rays takes its count from the host)
 *   2. evaluate        mi_nerf_mlp_rays* (n', S = 32) of cfg->mode
 *   3. scatter         writes EVERY raw[ray, sample]: the gathered value of a survivor, zeros otherwise
 *   4. composite (+ resample)   mi_nerf_composite, then mi_nerf_fine_z after the coarse pass
 * THIS ENTRY SYNCHRONISES ITS STREAM ONCE PER NETWORK PASS (twice when Nf > 0) and therefore refuses a stream that is being captured
 * into a graph (MI_OCC_EINVAL).  The first call of a thread allocates 8 bytes of pinned host memory (portable: usable from every device)
 * that the thread keeps; it is never freed.
 * Jitter: t_rand [n,Sc] / u [n,Nf] as for mi_nerf_render_rays; NULL: mi_nerf_fill_uniform(cfg->seed, stream 0 / 1, cfg->ray_offset, ...)
 * into the workspace -- the values mi_nerf_render_rays draws.  u is ignored when det != 0.
 * Modes: MI_NERF_MODE_F32, MI_NERF_MODE_F16S, MI_NERF_MODE_BF16; every other mode is refused.
 * Limits: n_rays * (Sc + Nf + 31) < 2^31; Sc + Nf <= 1024 (mi_nerf_composite).  workspace_dev 256-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mi_occ_stats {               /* samples per pass: in all, run through the network as survivors, run as padding */
    int64_t total_c, evaluated_c, padded_c;
    int64_t total_f, evaluated_f, padded_f; /* zeros when Nf == 0 */
} mi_occ_stats;

/* Offsets (bytes) inside the workspace.  T = n_rays * ceil(max(Sc, Sc + Nf) / 32) tiles at most, Smax = Sc + Nf. */
typedef struct mi_occ_workspace_layout {
    size_t z_c, raw_c, weights_c, z_f, raw_f;   /* the intermediates of mi_nerf_workspace_layout, same shapes */
    size_t t_rand, u;                           /* [n,Sc], [n,Nf]: drawn jitter (unused when the caller passes its own) */
    size_t slot;                                /* int32 [n,Smax]: flat tile lane of each sample, -1 = skipped */
    size_t tile_rays, tile_z, tile_src, tile_raw;   /* [T,6], [T,32], int32 [T,32], [T,32,4] */
    size_t counters;                            /* uint32 [2]: tiles, survivors of the last pass */
    size_t total;
} mi_occ_workspace_layout;
size_t mi_occ_render_workspace_bytes(const mi_nerf_render_cfg* cfg, int64_t n_rays);
int mi_occ_render_workspace_layout(const mi_nerf_render_cfg* cfg, int64_t n_rays, mi_occ_workspace_layout* out);

int mi_occ_render_rays(const mi_nerf_net* net, const void* packed_coarse_dev, const void* packed_fine_dev, const mi_nerf_render_cfg* cfg,
                       const mi_occ_grid* grid, const uint32_t* bits_coarse_dev, const uint32_t* bits_fine_dev, const float* rays_dev,
                       int64_t n_rays, const float* t_rand_dev, const float* u_dev, void* workspace_dev, size_t workspace_bytes,
                       float* rgb_c_dev, float* disp_c_dev, float* rgb_f_dev, float* disp_f_dev, mi_occ_stats* stats_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_OCC_H */
