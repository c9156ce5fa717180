/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: the entries of the compact grid resolve, the
 * record and scratch sizes answer, and refusals come back as MI_VOX_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    float word[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint8_t byte[1] = {0};
    int32_t slot[1] = {0};
    int64_t count[1] = {0};
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
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION || MI_VOX_ABI_VERSION < 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    if (mi_vox_record_bytes(1, MI_VOX_FMT_F32) != 16 || mi_vox_record_bytes(4, MI_VOX_FMT_F32) != 64 || mi_vox_record_bytes(9, MI_VOX_FMT_F32) != 128) return 2;
    if (mi_vox_record_bytes(1, MI_VOX_FMT_F16) != 8 || mi_vox_record_bytes(4, MI_VOX_FMT_F16) != 32 || mi_vox_record_bytes(9, MI_VOX_FMT_F16) != 64) return 3;
    if (mi_vox_record_bytes(2, MI_VOX_FMT_F32) != 0 || mi_vox_record_bytes(9, 2) != 0 || mi_vox_record_bytes(9, -1) != 0) return 4;
    /* 21^3 = 9261 points: at least one count per point would be more than any sane scratch, and none is too little */
    if (mi_vox_index_scratch_bytes(&grid) == 0 || mi_vox_index_scratch_bytes(&grid) % 16 != 0 || mi_vox_index_scratch_bytes(&grid) > 4 * 9261) return 5;
    if (mi_vox_index_scratch_bytes(NULL) != 0 || strlen(mi_vox_last_error()) == 0) return 6;
    if (mi_vox_index(&grid, word, slot, count, word, 0, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "scratch") == NULL) {
        printf("a scratch of no bytes was not refused: %s\n", mi_vox_last_error());
        return 7;
    }
    if (mi_vox_pack(&grid, 9, 2, word, slot, 1, word, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "fmt") == NULL) return 8;
    if (mi_vox_pack(&grid, 9, MI_VOX_FMT_F16, NULL, NULL, 0, NULL, NULL) != MI_VOX_OK) return 9;        /* M = 0: nothing to do */
    if (mi_vox_render_sparse(&grid, 9, MI_VOX_FMT_F16, word, NULL, word, 1, byte, word, 1, &cfg, word, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strlen(mi_vox_last_error()) == 0) {
        printf("a NULL slot plane was not refused: %s\n", mi_vox_last_error());
        return 10;
    }
    if (mi_vox_render_sparse(&grid, 9, MI_VOX_FMT_F32, word, slot, word, -1, byte, word, 1, &cfg, word, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL) return 11;
    printf("vox sparse c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
