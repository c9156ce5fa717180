/* A plain-C consumer of include/mi_nerf_mesh.h: the header (and mi_nerf.h, which it includes) is valid C99, libmi_nerf_mesh.so links from C
 * with nothing but the headers and finds libmi_nerf.so beside itself, and the argument checks answer before any GPU call (this program
 * runs on a box without a GPU).  Built and run by tests/test_mesh_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_mesh.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_mesh_last_error()); return 1; } } while (0)

int main(void) {
    mi_mesh_grid g;
    mi_nerf_net net;
    float dummy[8];
    int32_t idx[8];
    uint64_t counts[2];
    size_t need;
    int i;
    for (i = 0; i < 3; ++i) { g.lo[i] = -1.0f; g.hi[i] = 1.0f; g.res[i] = 1; }
    net.D = 8; net.W = 256; net.skip = 4; net.L_x = 10; net.L_d = 4;
    EXPECT(mi_mesh_abi_version() == MI_MESH_ABI_VERSION);
    /* one cell: 8 points, 1 cell, 1 block of sums -> four regions of 256 bytes */
    EXPECT(mi_mesh_extract_scratch_bytes(&g) == 4 * 256);
    /* 2 x 2 x 2 points: 4 rows of 2 points, the whole lattice in one slab */
    EXPECT(mi_mesh_density_scratch_bytes(&g) == 3 * 256);
    g.res[0] = MI_MESH_MAX_RES + 1;
    EXPECT(mi_mesh_extract_scratch_bytes(&g) == 0 && strstr(mi_mesh_last_error(), "res") != NULL);
    g.res[0] = 128; g.res[1] = 128; g.res[2] = 128;
    need = mi_mesh_extract_scratch_bytes(&g);
    EXPECT(need > (size_t)129 * 129 * 129 * 5 + (size_t)128 * 128 * 128 * 4);
    EXPECT(mi_mesh_count(&g, dummy, 0.5f, NULL, need, counts, NULL) == MI_MESH_EINVAL && strlen(mi_mesh_last_error()) > 0);
    EXPECT(mi_mesh_count(&g, dummy, 0.5f, (void*)0x100000, need - 1, counts, NULL) == MI_MESH_EINVAL && strstr(mi_mesh_last_error(), "scratch") != NULL);
    EXPECT(mi_mesh_emit(&g, dummy, 0.5f, (void*)0x100000, need, (uint64_t)1 << 31, 4, dummy, idx, NULL, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "2^31") != NULL);
    EXPECT(mi_mesh_density(&g, &net, dummy, MI_NERF_MODE_F16_BF16, dummy, (void*)0x100000, (size_t)1 << 40, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "mode") != NULL);
    EXPECT(mi_mesh_density(&g, &net, dummy, MI_NERF_MODE_F32, dummy, (void*)0x100000, mi_mesh_density_scratch_bytes(&g) - 1, NULL) == MI_MESH_EINVAL);
    printf("mesh c_abi consumer ok: ABI %d\n", mi_mesh_abi_version());
    return 0;
}
