/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: mi_vox_view and the four entries of pruning by
 * visibility resolve within ABI 2, the size formula answers, and refusals come back as MI_VOX_EINVAL with a message, before any device is
 * touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    /* never dereferenced: every call below is refused on its arguments */
    static float sigma_a[64], sigma_b[64], od[64];
    static float coef_a[8 * 32 + 4], tvol_a[4 * 4 * 8 + 8];
    float *ca = coef_a, *tv = tvol_a;
    mi_vox_grid grid;
    mi_vox_view view;
    int i;
    for (i = 0; i < 3; ++i) {
        grid.lo[i] = -1.0f;
        grid.hi[i] = 1.0f;
        grid.res[i] = 1;
    }
    memset(&view, 0, sizeof view);
    view.H = 4; view.W = 4;
    view.fx = view.fy = 4.0f; view.cx = view.cy = 2.0f;
    view.c2w[0] = view.c2w[5] = view.c2w[10] = 1.0f;
    view.c2w[11] = 4.0f;
    view.depth_near = 3.0f; view.depth_step = 0.25f; view.slices = 8;
    while (((size_t)ca & 15) != 0) ++ca;                                     /* 16-byte aligned records */
    while (((size_t)tv & 31) != 0) ++tv;                                     /* 32-byte aligned tvol */
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION || MI_VOX_ABI_VERSION != 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    if (sizeof(mi_vox_view) != 84) {
        printf("sizeof(mi_vox_view) = %u\n", (unsigned)sizeof(mi_vox_view));
        return 2;
    }
    if (mi_vox_shadow_bytes(&view) != (size_t)(4 * 4 * 8 * 4)) return 3;
    view.slices = 12;
    if (mi_vox_shadow_bytes(&view) != 0 || strstr(mi_vox_last_error(), "slices") == NULL) {
        printf("12 slices were not refused: %s\n", mi_vox_last_error());
        return 4;
    }
    if (mi_vox_shadow(&grid, sigma_a, NULL, &view, tv, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "slices") == NULL) return 5;
    view.slices = 8;
    if (mi_vox_shadow(&grid, sigma_a, NULL, &view, tv + 1, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "aligned") == NULL) return 6;
    if (mi_vox_shadow(&grid, sigma_a, NULL, NULL, tv, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "view") == NULL) return 7;
    if (mi_vox_shadow(NULL, sigma_a, NULL, &view, tv, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "grid") == NULL) return 8;
    if (mi_vox_seen(&grid, &view, tv, -1, od, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "bias") == NULL) {
        printf("a negative bias was not refused: %s\n", mi_vox_last_error());
        return 9;
    }
    if (mi_vox_seen(&grid, &view, tv, 2, tv, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "overlaps") == NULL) return 10;
    if (mi_vox_seen(&grid, &view, NULL, 2, od, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "NULL") == NULL) return 11;
    if (mi_vox_prune_seen(&grid, 9, 0.5f, -1.0f, sigma_a, od, sigma_b, ca, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "od_max") == NULL) {
        printf("a negative od_max was not refused: %s\n", mi_vox_last_error());
        return 12;
    }
    if (mi_vox_prune_seen(&grid, 9, 0.5f, 6.9f, sigma_a, od, sigma_a, ca, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "sigma_out") == NULL) return 13;
    if (mi_vox_prune_seen(&grid, 7, 0.5f, 6.9f, sigma_a, od, sigma_b, ca, NULL) != MI_VOX_EINVAL) return 14;
    if (mi_vox_prune_seen(&grid, 9, -0.5f, 6.9f, sigma_a, od, sigma_b, ca, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "tau") == NULL) return 15;
    printf("vox seen c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
