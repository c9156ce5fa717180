/* A plain-C consumer of THE VIEW of include/mi_nerf_mesh.h: the camera struct and the three entries are valid C99, the library links from C, the
 * scratch formula is the header's, and the argument checks answer before any GPU call (this program runs on a box without a GPU).  Built and
 * run by tests/test_mesh_view_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_mesh.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_mesh_last_error()); return 1; } } while (0)

int main(void) {
    mi_mesh_camera cam;
    float dummy[16];
    int32_t idx[16];
    float bg[3] = {1.0f, 1.0f, 1.0f};
    void* scratch = (void*)0x100000;
    size_t need;
    int i;
    cam.H = 64; cam.W = 48; cam.fx = 70.0f; cam.fy = 70.0f; cam.cx = 23.5f; cam.cy = 31.5f;
    for (i = 0; i < 12; ++i) cam.c2w[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    EXPECT(mi_mesh_abi_version() == MI_MESH_ABI_VERSION && MI_MESH_ABI_VERSION == 2);
    need = mi_mesh_raster_scratch_bytes(64, 48);
    EXPECT(need == (size_t)8 * 64 * 48 + 256 + (size_t)4 * MI_MESH_VIEW_QUEUE);
    EXPECT(mi_mesh_raster_scratch_bytes(1, 1) == 256 + 256 + (size_t)4 * MI_MESH_VIEW_QUEUE);
    EXPECT(mi_mesh_raster_scratch_bytes(0, 48) == 0 && strstr(mi_mesh_last_error(), "H=0") != NULL);
    EXPECT(mi_mesh_raster_scratch_bytes(64, MI_MESH_VIEW_MAX_DIM + 1) == 0);
    EXPECT(256 * MI_MESH_VIEW_MAX_DIM == MI_MESH_VIEW_GUARD);
    EXPECT(mi_mesh_project(&cam, 0.0f, dummy, 4, idx, idx, dummy, NULL) == MI_MESH_EINVAL && strstr(mi_mesh_last_error(), "near") != NULL);
    EXPECT(mi_mesh_project(NULL, 0.1f, dummy, 4, idx, idx, dummy, NULL) == MI_MESH_EINVAL && strstr(mi_mesh_last_error(), "cam") != NULL);
    EXPECT(mi_mesh_project(&cam, 0.1f, dummy, 0, NULL, NULL, NULL, NULL) == MI_MESH_OK);      /* V == 0 launches nothing */
    EXPECT(mi_mesh_raster(64, 48, 3, 0, idx, idx, dummy, 4, idx, 2, scratch, need, idx, dummy, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "cull") != NULL);
    EXPECT(mi_mesh_raster(64, 48, 0, 0, idx, idx, dummy, 4, idx, 2, scratch, need - 1, idx, dummy, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "scratch") != NULL);
    EXPECT(mi_mesh_raster(64, 48, 0, 0, idx, idx, dummy, 4, idx, 2, scratch, need, NULL, NULL, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "no output") != NULL);
    EXPECT(mi_mesh_shade(64, 48, idx, idx, dummy, 4, idx, 2, idx, dummy, NULL, bg, NULL, NULL, NULL, NULL, NULL, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "no output") != NULL);
    EXPECT(mi_mesh_shade(64, 48, idx, idx, dummy, (int64_t)1 << 31, idx, 2, idx, dummy, NULL, bg, dummy, NULL, NULL, NULL, NULL, NULL) == MI_MESH_EINVAL);
    EXPECT(strstr(mi_mesh_last_error(), "2^31") != NULL);
    printf("mesh view c_abi consumer ok: ABI %d\n", mi_mesh_abi_version());
    return 0;
}
