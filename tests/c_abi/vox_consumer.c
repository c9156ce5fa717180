/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: the header compiles on its own, the entries
 * resolve, the sizes answer, and refusals come back as MI_VOX_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    float word[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint8_t byte[1] = {0};
    int64_t index[1] = {0};
    mi_vox_grid grid;
    mi_vox_render_cfg cfg;
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
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    if (mi_vox_record_floats(1) != 4 || mi_vox_record_floats(4) != 16 || mi_vox_record_floats(9) != 32 || mi_vox_record_floats(2) != 0) return 2;
    if (mi_vox_skip_bytes(&grid) != 27) return 3;
    /* the diagonal is 2 sqrt(3) = 3.4641: 70 intervals of 0.05 and one more */
    if (mi_vox_max_steps(&grid, 0.05f) != 71) return 4;
    if (mi_vox_max_steps(&grid, 0.0f) != 0 || strlen(mi_vox_last_error()) == 0) return 5;
    cfg.step = -1.0f;
    if (mi_vox_render(&grid, 9, word, word, byte, word, 1, &cfg, word, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL || strlen(mi_vox_last_error()) == 0) {
        printf("a negative step was not refused: %s\n", mi_vox_last_error());
        return 6;
    }
    cfg.step = 0.05f;
    if (mi_vox_render(&grid, 2, word, word, byte, word, 1, &cfg, word, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL) return 7;
    grid.res[1] = 513;
    if (mi_vox_build_skip(&grid, word, byte, NULL) != MI_VOX_EINVAL) return 8;
    grid.res[1] = 20;
    if (mi_vox_project(&grid, 9, 8, word, word, index, 1, word, word, NULL) != MI_VOX_EINVAL) return 9;
    printf("vox c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
