/* A C99 program that sees include/mi_nerf_voxgrad.h alone and links against libmi_nerf_voxgrad.so: the header compiles on its own, the
 * entries resolve, the structs have their sizes, and refusals come back as MI_VOXGRAD_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_voxgrad.h"

int main(void) {
    float word[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint8_t byte[1] = {0};
    mi_voxgrad_grid grid;
    mi_voxgrad_render_cfg cfg;
    int i;
    for (i = 0; i < 3; ++i) {
        grid.lo[i] = -1.0f;
        grid.hi[i] = 1.0f;
        grid.res[i] = 20;
    }
    memset(&cfg, 0, sizeof(cfg));
    cfg.step = 0.05f;
    cfg.t_near = 0.0f;
    cfg.t_far = 10.0f;
    cfg.bg[0] = cfg.bg[1] = cfg.bg[2] = 1.0f;
    if (mi_voxgrad_abi_version() != MI_VOXGRAD_ABI_VERSION) {
        printf("ABI mismatch: library %d, header %d\n", mi_voxgrad_abi_version(), MI_VOXGRAD_ABI_VERSION);
        return 1;
    }
    if (sizeof(mi_voxgrad_grid) != 36 || sizeof(mi_voxgrad_render_cfg) != 32) return 2;
    /* no work: nothing is launched, no pointer is looked at */
    if (mi_voxgrad_render_backward(&grid, 9, NULL, NULL, NULL, NULL, 0, &cfg, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != MI_VOXGRAD_OK) return 3;
    cfg.step = -1.0f;
    if (mi_voxgrad_render_backward(&grid, 9, word, word, byte, word, 1, &cfg, word, NULL, NULL, word, word, NULL, NULL, NULL, NULL) != MI_VOXGRAD_EINVAL ||
        strlen(mi_voxgrad_last_error()) == 0) {
        printf("a negative step was not refused: %s\n", mi_voxgrad_last_error());
        return 4;
    }
    cfg.step = 0.05f;
    if (mi_voxgrad_render_backward(&grid, 2, word, word, byte, word, 1, &cfg, word, NULL, NULL, word, word, NULL, NULL, NULL, NULL) != MI_VOXGRAD_EINVAL) return 5;
    grid.res[1] = 513;
    if (mi_voxgrad_render_backward(&grid, 9, word, word, byte, word, 1, &cfg, word, NULL, NULL, word, word, NULL, NULL, NULL, NULL) != MI_VOXGRAD_EINVAL) return 6;
    grid.res[1] = 20;
    if (mi_voxgrad_render_backward(&grid, 9, word, word, byte, word, 1, &cfg, word, NULL, NULL, NULL, word, NULL, NULL, NULL, NULL) != MI_VOXGRAD_EINVAL) return 7;
    printf("voxgrad c_abi consumer ok: ABI %d\n", mi_voxgrad_abi_version());
    return 0;
}
