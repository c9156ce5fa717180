/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: the three entries of A SIGNED GRID resolve
 * within ABI 2, and their refusals come back as MI_VOX_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    /* never dereferenced: every call below is refused on its arguments, or has no work */
    static float sigma[64], rays[6], rgb[3];
    static float coef_a[8 * 32 + 4];
    static uint8_t skip[8];
    static int32_t slot[64];
    float* coef = coef_a;
    mi_vox_grid g;
    mi_vox_render_cfg cfg;
    int i;
    for (i = 0; i < 3; ++i) {
        g.lo[i] = -1.0f;
        g.hi[i] = 1.0f;
        g.res[i] = 1;
        cfg.bg[i] = 1.0f;
    }
    cfg.step = 0.5f; cfg.t_near = 0.0f; cfg.t_far = 6.0f; cfg.T_min = 0.0f; cfg.use_skip = 1;
    while (((size_t)coef & 15) != 0) ++coef;                                 /* 16-byte aligned records */
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION || MI_VOX_ABI_VERSION != 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    if (mi_vox_build_skip_signed(NULL, sigma, skip, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "mi_vox_build_skip_signed") == NULL) return 2;
    if (mi_vox_build_skip_signed(&g, NULL, skip, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "NULL") == NULL) return 3;
    if (mi_vox_build_skip_signed(&g, sigma, NULL, NULL) != MI_VOX_EINVAL) return 4;
    if (mi_vox_render_signed(&g, 5, sigma, coef, skip, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "B=5") == NULL || strstr(mi_vox_last_error(), "mi_vox_render_signed") == NULL)
        return 5;
    if (mi_vox_render_signed(&g, 9, sigma, coef + 1, skip, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "aligned") == NULL)
        return 6;
    if (mi_vox_render_signed(&g, 9, sigma, coef, NULL, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "skip") == NULL) {
        printf("use_skip without a plane was not refused: %s\n", mi_vox_last_error());
        return 7;
    }
    if (mi_vox_render_signed(&g, 9, sigma, coef, skip, rays, 1, NULL, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL) return 8;
    if (mi_vox_render_signed(&g, 9, NULL, NULL, NULL, NULL, 0, &cfg, NULL, NULL, NULL, NULL, NULL, NULL) != MI_VOX_OK) return 9;   /* no work */
    if (mi_vox_render_sparse_signed(&g, 9, 2, sigma, slot, coef, 1, skip, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "fmt=2") == NULL || strstr(mi_vox_last_error(), "mi_vox_render_sparse_signed") == NULL)
        return 10;
    if (mi_vox_render_sparse_signed(&g, 9, MI_VOX_FMT_F16, sigma, slot, coef, 9, skip, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "M=9") == NULL)
        return 11;
    if (mi_vox_render_sparse_signed(&g, 9, MI_VOX_FMT_F32, sigma, NULL, coef, 1, skip, rays, 1, &cfg, rgb, NULL, NULL, NULL, NULL, NULL) != MI_VOX_EINVAL) return 12;
    if (mi_vox_render_sparse_signed(&g, 9, MI_VOX_FMT_F32, NULL, NULL, NULL, 0, NULL, NULL, 0, &cfg, NULL, NULL, NULL, NULL, NULL, NULL) != MI_VOX_OK) return 13;
    printf("vox signed c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
