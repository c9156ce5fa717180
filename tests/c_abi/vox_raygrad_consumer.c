/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: the two entries of THE RAY GRADIENT RULE
 * resolve within ABI 2, an empty ray set is no work, and refusals come back as MI_VOX_EINVAL with a message, before any device is
 * touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    /* never dereferenced: every call below is refused on its arguments or has no work */
    static float sigma[8], rays[12], g_rgb[6], g_acc[2], d_rays[12], rgb[6];
    static float coef_a[8 * 32 + 4];
    static int32_t slot[8];
    float* ca = coef_a;
    mi_vox_grid grid;
    mi_vox_render_cfg cfg;
    int i;
    for (i = 0; i < 3; ++i) {
        grid.lo[i] = -1.0f;
        grid.hi[i] = 1.0f;
        grid.res[i] = 1;
        cfg.bg[i] = 1.0f;
    }
    cfg.step = 0.5f; cfg.t_near = 0.0f; cfg.t_far = 6.0f; cfg.T_min = 0.0f; cfg.use_skip = 0;
    while (((size_t)ca & 15) != 0) ++ca;                                     /* 16-byte aligned records */
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION || MI_VOX_ABI_VERSION != 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    /* n == 0: nothing is launched and the arrays are not looked at */
    if (mi_vox_render_backward_rays(&grid, 9, NULL, NULL, NULL, NULL, 0, &cfg, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != MI_VOX_OK) return 2;
    if (mi_vox_render_sparse_backward_rays(&grid, 9, MI_VOX_FMT_F16, NULL, NULL, NULL, 0, NULL, NULL, 0, &cfg, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) !=
        MI_VOX_OK)
        return 3;
    if (mi_vox_render_backward_rays(NULL, 9, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "grid") == NULL)
        return 4;
    if (mi_vox_render_backward_rays(&grid, 7, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "B=7") == NULL)
        return 5;
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca, NULL, rays, 2, &cfg, NULL, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "NULL") == NULL) {
        printf("a NULL g_rgb was not refused: %s\n", mi_vox_last_error());
        return 6;
    }
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, NULL, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "NULL") == NULL)
        return 7;
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca + 1, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "aligned") == NULL)
        return 8;
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "overlaps") == NULL) {
        printf("d_rays == rays was not refused: %s\n", mi_vox_last_error());
        return 9;
    }
    cfg.use_skip = 1;
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "skip") == NULL)
        return 10;
    cfg.use_skip = 0;
    if (mi_vox_render_sparse_backward_rays(&grid, 9, 2, sigma, slot, ca, 8, NULL, rays, 2, &cfg, g_rgb, NULL, NULL, d_rays, NULL, NULL, NULL, NULL) !=
            MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "fmt") == NULL)
        return 11;
    if (mi_vox_render_sparse_backward_rays(&grid, 9, MI_VOX_FMT_F32, sigma, slot, ca, 9, NULL, rays, 2, &cfg, g_rgb, NULL, NULL, d_rays, NULL, NULL, NULL,
                                           NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "M=9") == NULL)
        return 12;
    if (mi_vox_render_sparse_backward_rays(&grid, 9, MI_VOX_FMT_F32, sigma, NULL, ca, 8, NULL, rays, 2, &cfg, g_rgb, NULL, NULL, d_rays, NULL, NULL, NULL,
                                           NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "NULL") == NULL)
        return 13;
    cfg.step = 0.0f;
    if (mi_vox_render_backward_rays(&grid, 9, sigma, ca, NULL, rays, 2, &cfg, g_rgb, g_acc, NULL, d_rays, rgb, NULL, NULL, NULL) != MI_VOX_EINVAL ||
        strstr(mi_vox_last_error(), "step") == NULL)
        return 14;
    printf("vox raygrad c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
