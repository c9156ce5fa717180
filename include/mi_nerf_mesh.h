/*
 * mi_nerf_mesh.h -- C ABI of libmi_nerf_mesh.so: triangle meshes from a density lattice on the MI355X (gfx950), and views of them.
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
 *
 * THE VIEW: a rasteriser for the meshes above (mi_mesh_project, mi_mesh_raster and mi_mesh_shade are its public statement).  All fp32
 * arithmetic is rounded once per operation (no contraction); coverage is integer arithmetic and has no rounding at all.
 *   Camera.     The pinhole camera of make_o_d: H rows, W columns, fx, fy, cx, cy and the pose c2w [3,4] = (R | t), row-major.  For a
 *               vertex v:   d_k = v_k - t_k;   p_i = (R_0i d_0 + R_1i d_1) + R_2i d_2   (p = R^T d: three products, two sums, in this order)
 *                   z  = -p_z                        the parameter t of the pixel's ray x = o + t d: the project's `depth`
 *                   sx = cx + (fx * p_x) / z         column
 *                   sy = cy - (fy * p_y) / z         row (downwards)
 *               Pixel (i, j) -- column i, row j, element j W + i of every output -- has its centre at screen position (i, j): the ray
 *               make_o_d gives pixel (i, j) passes through exactly that point.
 *   Snap.       X = rint(256 sx), Y = rint(256 sy) as int32 (24.8 fixed point, ties to even).
 *   Validity.   A vertex is valid iff z > near, z is finite, |256 sx| <= 2^22 and |256 sy| <= 2^22 (the guard band; a NaN fails every
 *               test).  An invalid vertex is stored as z = 0, X = Y = INT32_MIN.  mi_mesh_raster and mi_mesh_shade take any arrays and
 *               hold a vertex valid iff 0 < z < inf, |X| <= 2^22 and |Y| <= 2^22.  THERE IS NO NEAR-PLANE CLIPPING: a triangle with an
 *               invalid vertex, or with a vertex number outside [0, V), is not drawn (and nothing is read out of bounds for it).
 *   Coverage.   orient(a, b, p) = (X_b - X_a)(Y_p - Y_a) - (Y_b - Y_a)(X_p - X_a) on int64.  A2 = orient(v0, v1, v2), the doubled signed area.
 *               A2 == 0: not drawn.  A triangle is FRONT iff A2 < 0: rows grow downwards, so that is counter-clockwise on the screen,
 *               which is how mi_mesh_emit's winding (normals towards lower density) looks from outside.  cull 0 draws both, 1 drops
 *               back faces (A2 > 0), 2 drops front faces.  With s = sign(A2) and P = (256 i, 256 j):
 *                   e_0 = s orient(v1, v2, P), e_1 = s orient(v2, v0, P), e_2 = s orient(v0, v1, P), a2 = s A2 = e_0 + e_1 + e_2 > 0
 *               The edge of e_k runs from a to b with (dx, dy) = s (X_b - X_a, Y_b - Y_a); it is a TOP-LEFT edge iff dy < 0, or dy == 0
 *               and dx > 0.  Pixel (i, j) is covered iff every e_k > 0, or e_k == 0 on a top-left edge.  Two triangles that share an
 *               edge cover each pixel centre on it exactly once.  No anti-aliasing.  |e_k| < 2^48 for H, W <= MI_MESH_VIEW_MAX_DIM.
 *   Depth.      Perspective-correct: b_k = (float)e_k / (float)a2 (int64 -> fp32 rounded to nearest even), w_k = b_k / z_k,
 *               inv = (w_0 + w_1) + w_2, depth = 1.f / inv.
 *   Visibility. The triangle with the smallest depth wins the pixel (fp32 comparison; depth > 0); ties go to the smaller triangle
 *               number.  The result does not depend on the order in which triangles are processed: every output is the same bit for
 *               bit from run to run.
 *   Shade.      From the winner's number alone: e_k, b_k, w_k and depth as above, then per channel
 *                   c = ((w_0 c_0 + w_1 c_1) + w_2 c_2) * depth;   c < 0 -> 0, c > 1 -> 1 (a NaN stays a NaN)
 *               with the per-vertex colours c_k.  Normals: n the same expression of the per-vertex normals (not clamped),
 *               len = sqrtf((n_x n_x + n_y n_y) + n_z n_z), output n_i / len, or (0, 0, 0) when len is 0 or not finite.  disp = 1.f / depth.
 * Not in THE VIEW: anti-aliasing, near-plane clipping, textures and lighting, gradients, NDC scenes, triangles beyond the guard band.
 */
#ifndef MI_NERF_MESH_H
#define MI_NERF_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "mi_nerf.h"   /* mi_nerf_net, MI_NERF_MODE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_MESH_ABI_VERSION 2

/* status codes (the values of mi_nerf.h) */
#define MI_MESH_OK 0
#define MI_MESH_EINVAL 1   /* bad argument / unsupported shape or mode */
#define MI_MESH_EHIP 2     /* HIP runtime error, or a failed call into libmi_nerf.so (its text is carried over) */

#define MI_MESH_MAX_RES 512             /* largest res[i] */
#define MI_MESH_MIN_SLAB_POINTS 1024    /* mi_mesh_density: the smallest slab holds at least this many lattice points (or the whole lattice) */
#define MI_MESH_SCAN_TILE 1024          /* elements of one block of the prefix sums */
#define MI_MESH_VIEW_MAX_DIM 16384      /* largest H and W of a view: 256 W <= 2^22, the guard band */
#define MI_MESH_VIEW_GUARD 4194304      /* 2^22: the guard band of the snapped coordinates */
#define MI_MESH_VIEW_LARGE_BOX 32       /* pixels in a triangle's clipped bounding box above which a whole wave walks it (mesh_view.hip: measured) */
#define MI_MESH_VIEW_QUEUE 65536        /* large triangles the queue holds; the ones beyond it are walked by their own lane */

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

/* ------------------------------------------------------------------------------------------------
 * THE VIEW.  Three entries, one per stage, so that each can be tested on the inputs of the next; none synchronises the host.  Every
 * pointer but `cam` and `bg` is a device pointer, 4-byte aligned (scratch: 256).  H and W: 1..MI_MESH_VIEW_MAX_DIM (0 is refused);
 * V and T: 0..2^31 - 1; V == 0 takes NULL vertex arrays, T == 0 a NULL tris.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mi_mesh_camera {
    int32_t H, W;
    float fx, fy, cx, cy;     /* finite; fx and fy not 0 */
    float c2w[12];            /* [3,4] row-major, finite */
} mi_mesh_camera;

/* One thread per vertex: verts [V,3] -> X, Y int32 [V] and z float [V] (Camera, Snap, Validity).  near > 0.  V == 0 launches nothing. */
int mi_mesh_project(const mi_mesh_camera* cam, float near, const float* verts_dev, int64_t V, int32_t* X_dev, int32_t* Y_dev, float* z_dev,
                    void* stream);

/* The visibility pass (Coverage, Depth, Visibility): tri_out int32 [H,W] = the winner's number or -1, depth_out float [H,W] = its depth or 0;
 * either may be NULL, not both.  One 64-bit word per pixel, depth bits << 32 | triangle number (a positive float's bits order as the float
 * does), cleared to all ones and lowered by a 64-bit unsigned atomic minimum; a last kernel resolves the words into the outputs.  One lane
 * takes one triangle and walks its clipped bounding box; a triangle whose box holds more than large_box pixels is queued, and a second
 * kernel walks it with a whole wave.  large_box == 0 takes MI_MESH_VIEW_LARGE_BOX, the measured choice; any other value (> 0) exists for
 * measurements and changes no output.
 *     mi_mesh_raster_scratch_bytes = a256(8 H W) + a256(24 + 4 MI_MESH_VIEW_QUEUE)
 *         uint64 word[H W]
 *         uint32 counters[6]   0: large triangles met   1: triangles drawn by a lane   2, 3: atomic updates issued (low, high word)
 *                              4, 5: the updates among them that lowered their word
 *         int32  queue[MI_MESH_VIEW_QUEUE]
 * The counters are there to be read back by whoever measures.  T == 0 or V == 0: clear and resolve only. */
size_t mi_mesh_raster_scratch_bytes(int H, int W);   /* 0 + error text if H or W is refused */
int mi_mesh_raster(int H, int W, int cull, int large_box, const int32_t* X_dev, const int32_t* Y_dev, const float* z_dev, int64_t V,
                   const int32_t* tris_dev, int64_t T, void* scratch_dev, size_t scratch_bytes, int32_t* tri_out_dev, float* depth_out_dev,
                   void* stream);

/* One thread per pixel (Shade), from tri_in int32 [H,W]: a pixel is covered iff 0 <= tri_in < T, the triangle's vertex numbers are in
 * [0, V), its vertices valid and its A2 != 0 (coverage itself is NOT tested again).  colors [V,3] is required when rgb_dev is given, normals [V,3] when
 * normal_dev is given, bg is 3 floats on the host.  Outputs, any of them NULL but not all:
 *     rgb [H,W,3]   c | bg        disp [H,W]   1 / depth | 0        acc [H,W]   1 | 0        depth [H,W]   depth | 0        normal [H,W,3]   n | 0 */
int mi_mesh_shade(int H, int W, const int32_t* X_dev, const int32_t* Y_dev, const float* z_dev, int64_t V, const int32_t* tris_dev, int64_t T,
                  const int32_t* tri_in_dev, const float* colors_dev, const float* normals_dev, const float* bg, float* rgb_dev, float* disp_dev,
                  float* acc_dev, float* depth_dev, float* normal_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_MESH_H */
