/* A plain-C consumer of include/mi_nerf_scene.h: the header is valid C99 on its own, libmi_nerf_scene.so links from C with nothing but the
 * header, and the argument checks answer before any GPU call (this program runs on a box without a GPU).  Built and run by
 * tests/test_scene_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_scene.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_scene_last_error()); return 1; } } while (0)

int main(void) {
    mi_scene_prim p[2];
    float dummy[8];
    memset(p, 0, sizeof p);
    EXPECT(sizeof(mi_scene_prim) == 64);
    EXPECT(mi_scene_abi_version() == MI_SCENE_ABI_VERSION);
    p[0].kind = MI_SCENE_SPHERE; p[0].h[0] = 0.5f; p[0].sigma = 64.0f;
    p[1].kind = MI_SCENE_CYLINDER; p[1].axis = 2; p[1].h[0] = 0.25f; p[1].h[1] = 0.5f; p[1].sigma = 64.0f; p[1].freq = 4.0f;
    EXPECT(mi_scene_check(p, 2) == MI_SCENE_OK);
    EXPECT(mi_scene_check(p, 0) == MI_SCENE_EINVAL && strstr(mi_scene_last_error(), "n_prims") != NULL);
    EXPECT(mi_scene_check(p, MI_SCENE_MAX_PRIMS + 1) == MI_SCENE_EINVAL);
    EXPECT(mi_scene_check(NULL, 1) == MI_SCENE_EINVAL);
    p[1].axis = 3;
    EXPECT(mi_scene_check(p, 2) == MI_SCENE_EINVAL && strstr(mi_scene_last_error(), "axis") != NULL);
    EXPECT(mi_scene_check(p, 1) == MI_SCENE_OK);                           /* the first one alone is still fine */
    p[1].axis = 2; p[1].sigma = 0.0f;
    EXPECT(mi_scene_check(p, 2) == MI_SCENE_EINVAL && strstr(mi_scene_last_error(), "sigma") != NULL);
    p[1].sigma = 64.0f;
    EXPECT(mi_scene_render(p, 2, NULL, 4, 2.0f, 6.0f, 64, dummy, NULL, NULL, NULL, NULL) == MI_SCENE_EINVAL);
    EXPECT(mi_scene_render(p, 2, dummy, 4, 2.0f, 6.0f, MI_SCENE_MAX_SAMPLES + 1, dummy, NULL, NULL, NULL, NULL) == MI_SCENE_EINVAL);
    EXPECT(strstr(mi_scene_last_error(), "S=") != NULL);
    EXPECT(mi_scene_render(p, 2, dummy, 4, 6.0f, 2.0f, 64, dummy, NULL, NULL, NULL, NULL) == MI_SCENE_EINVAL);
    EXPECT(mi_scene_field_rays(p, 2, dummy, dummy, -1, 8, dummy, NULL) == MI_SCENE_EINVAL);
    printf("scene c_abi consumer ok: ABI %d\n", mi_scene_abi_version());
    return 0;
}
