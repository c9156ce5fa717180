/*
 * mi_nerf_mesh.h -- C ABI of libmi_nerf_mesh.so: triangle meshes from a density lattice on the MI355X (gfx950).
 *
 * A library of its own ON TOP of the path: include/mi_nerf.h stays what it is, nothing here is declared there, and libmi_nerf_mesh.so
 * exports no mi_nerf_*, mi_occ_*, mi_iqa_* or mi_scene_* symbol.  It links against libmi_nerf.so (rpath $ORIGIN) and calls ONLY
 * mi_nerf_mlp_rays / mi_nerf_mlp_rays_f16s / mi_nerf_mlp_rays_bf16 and mi_nerf_last_error of it; mi_nerf.h is included for the types.
 * Same conventions: plain C99, raw device pointers, the caller allocates everything, int status (0 = ok), hipStream_t passed as void*,
 * every argument checked before any HIP call, error text through mi_mesh_last_error().  NO ENTRY SYNCHRONISES THE HOST: the caller
 * reads the two counters of mi_mesh_count back itself, between the two phases of an extraction.
 *
 * THE LATTICE.  res_i counts cells, P_i = res_i + 1 lattice points per axis.  All arithmetic fp32, every operation rounded once (no
 * contraction):
 *     step_i = (hi_i - lo_i) / (float)res_i            fp32 difference, fp32 division, computed on the host
 *     x_i(j) = lo_i + (float)j_i * step_i              product rounded, then sum rounded
 * The field f is a float array of P_z P_y P_x values, flat(j) = (j_z * P_y + j_y) * P_x + j_x.
 *
 * THE RULE: marching tetrahedra on the Kuhn split of each cell (mi_mesh_count and mi_mesh_emit are its public statement).
 *   Inside.     Point j is inside iff f[j] > iso.  A NaN is outside.
 *   Edges.      From each point j there are seven edges e = 0..6 to j + d_e, d_e = ((e+1) & 1, ((e+1) >> 1) & 1, ((e+1) >> 2) & 1): three
 *               axes, three face diagonals, the body diagonal.  An edge exists when j + d_e is a lattice point; its id is 7 flat(j) + e;
 *               it is crossed iff exactly one endpoint is inside.
 *   Vertices.   One per crossed edge, numbered in increasing edge id.  With a = j, b = j + d_e:
 *                   t   = (iso - f_a) / (f_b - f_a);  t = fminf(fmaxf(t, 0.f), 1.f)      (a NaN t becomes 0)
 *                   v_i = x_i(a) + t * (x_i(b) - x_i(a))
 *   Tetrahedra. In cell c (0 <= c_i < res_i) tetrahedron q = 0..5 belongs to the q-th permutation p of the axes (0, 1, 2) in
 *               lexicographic order; its corners are c, c + e_p0, c + e_p0 + e_p1, c + (1, 1, 1), in that order.
 *   Triangles   per tetrahedron, by the number of inside corners:
 *               1 or 3 -- A is the lone corner (the lone OUTSIDE corner when three are inside), B, C, D the others in corner order:
 *                         one triangle on the vertices of the edges AB, AC, AD;
 *               2      -- A < B the inside pair, C < D the outside pair: two triangles (AC, AD, BD) and (AC, BD, BC);
 *               0 or 4 -- none.
 *   Winding.    Decided on the lattice: with each triangle vertex at the midpoint of its edge (doubled integer coordinates),
 *               n = (m1 - m0) x (m2 - m0) must satisfy n . (centroid of the outside corners - centroid of the inside corners) > 0;
 *               otherwise the triangle's last two vertices are swapped.  Normals point towards lower density.
 *   Order.      Triangles by flat cell index (c_z * res_y + c_y) * res_x + c_x, then q, then first or second; int32 vertex numbers.
 * The same split in every cell makes faces match across cells: where the surface does not reach the lattice boundary the mesh is a closed
 * oriented manifold (every directed edge once, its reverse once).  A surface that reaches the boundary is left open there.
 *
 * NORMALS (optional).  g(j), the gradient of f at a lattice point: (f[j + 1] - f[j - 1]) / (2.f * step_i) per axis, one-sided
 * (f[1] - f[0]) / step_i and (f[P - 1] - f[P - 2]) / step_i at the lattice boundary.  At a vertex g_i = g_i(a) + t * (g_i(b) - g_i(a)),
 * len = sqrtf((g_x g_x + g_y g_y) + g_z g_z), and the normal is -g_i / len, or (0, 0, 0) when len is 0 or not finite.
 */
#ifndef MI_NERF_MESH_H
#define MI_NERF_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "mi_nerf.h"   /* mi_nerf_net, MI_NERF_MODE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_MESH_ABI_VERSION 1

/* status codes (the values of mi_nerf.h) */
#define MI_MESH_OK 0
#define MI_MESH_EINVAL 1   /* bad argument / unsupported shape or mode */
#define MI_MESH_EHIP 2     /* HIP runtime error, or a failed call into libmi_nerf.so (its text is carried over) */

#define MI_MESH_MAX_RES 512             /* largest res[i] */
#define MI_MESH_MIN_SLAB_POINTS 1024    /* mi_mesh_density: the smallest slab holds at least this many lattice points (or the whole lattice) */
#define MI_MESH_SCAN_TILE 1024          /* elements of one block of the prefix sums */

int mi_mesh_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_mesh_last_error(void);

/* Axis-aligned box cut into res[0] x res[1] x res[2] cells (x, y, z).  lo_i < hi_i, both finite, with a finite fp32 step > 0;
 * 1 <= res_i <= MI_MESH_MAX_RES. */
typedef struct mi_mesh_grid {
    float lo[3];
    float hi[3];
    int32_t res[3];
} mi_mesh_grid;

/* ------------------------------------------------------------------------------------------------
 * Network -> lattice.  f[flat(j)] = raw density (channel 3 of the network output, before the ReLU) of ONE network at x(j).  A lattice
 * row along x is laid out as one ray: origin (lo_x, x_y(j_y), x_z(j_z)), direction (1, 0, 0), depths (float)j_x * step_x, S = P_x; row
 * (j_y, j_z) is ray j_z * P_y + j_y.  The rows run through the public fused entry of `mode` (MI_NERF_MODE_F32 / _F16S / _BF16, the
 * blob being that family's; every other mode is refused) in slabs of R rows, R the largest the scratch holds (below 2^31 points):
 *     slab_bytes(R) = a256(24 R) + a256(4 R P_x) + a256(16 R P_x)          rays [R,6], depths [R,P_x], raw [R,P_x,4];  a256 rounds up to 256
 *     mi_mesh_density_scratch_bytes = slab_bytes(min(P_y P_z, ceil(MI_MESH_MIN_SLAB_POINTS / P_x)))
 * The smallest scratch is for memory-starved callers; a slab of a few million points keeps the network kernels busy.
 * scratch_dev 256-byte aligned.  No host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t mi_mesh_density_scratch_bytes(const mi_mesh_grid* grid);   /* 0 + error text if the grid is refused */
int mi_mesh_density(const mi_mesh_grid* grid, const mi_nerf_net* net, const void* packed_dev, int mode, float* f_dev, void* scratch_dev,
                    size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lattice -> indexed mesh, in two phases around ONE read-back by the caller.  With N = P_x P_y P_z points and C = res_x res_y res_z cells:
 *     mi_mesh_extract_scratch_bytes = a256(N) + a256(4 N) + a256(4 C) + a256(4 ceil(N / MI_MESH_SCAN_TILE))
 *         uint8  mask[N]      bit e: edge e of the point exists and is crossed
 *         uint32 vfirst[N]    vertex number of the point's first crossed edge (exclusive prefix sum of popcount(mask))
 *         uint32 tfirst[C]    triangle number of the cell's first triangle (exclusive prefix sum of the cells' triangle counts)
 *         uint32 block sums of the prefix sums
 * mi_mesh_count fills the scratch and writes counts_dev[0] = vertices, counts_dev[1] = triangles (uint64 on the device, 8-byte aligned).
 * mi_mesh_emit takes the SAME grid, f, iso and scratch, after mi_mesh_count on the same stream (or after the caller synchronised), and
 * the counts the caller read back as capacities: it fills verts [n_verts,3] float, tris [n_tris,3] int32 and, when normals_dev is not
 * NULL, normals [n_verts,3] float, and writes nothing beyond them.  Counts above 2^31 - 1 are refused.  A count of 0 takes a NULL array.
 * scratch_dev 256-byte aligned; iso not NaN.  No host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t mi_mesh_extract_scratch_bytes(const mi_mesh_grid* grid);   /* 0 + error text if the grid is refused */
int mi_mesh_count(const mi_mesh_grid* grid, const float* f_dev, float iso, void* scratch_dev, size_t scratch_bytes, uint64_t* counts_dev,
                  void* stream);
int mi_mesh_emit(const mi_mesh_grid* grid, const float* f_dev, float iso, const void* scratch_dev, size_t scratch_bytes, uint64_t n_verts,
                 uint64_t n_tris, float* verts_dev, int32_t* tris_dev, float* normals_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_MESH_H */
