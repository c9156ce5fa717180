/* A C99 program that sees include/mi_nerf_vox.h alone and links against libmi_nerf_vox.so: mi_vox_resample and mi_vox_prune resolve within
 * ABI 2, and their refusals come back as MI_VOX_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_vox.h"

int main(void) {
    /* never dereferenced: every call below is refused on its arguments */
    static float sigma_a[64], sigma_b[64];
    static float coef_a[8 * 32 + 4], coef_b[8 * 32 + 4];
    float *ca = coef_a, *cb = coef_b;
    mi_vox_grid src, dst;
    int i;
    for (i = 0; i < 3; ++i) {
        src.lo[i] = dst.lo[i] = -1.0f;
        src.hi[i] = dst.hi[i] = 1.0f;
        src.res[i] = 1;
        dst.res[i] = 1;
    }
    while (((size_t)ca & 15) != 0) ++ca;                                     /* 16-byte aligned records */
    while (((size_t)cb & 15) != 0) ++cb;
    if (mi_vox_abi_version() != MI_VOX_ABI_VERSION || MI_VOX_ABI_VERSION != 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_vox_abi_version(), MI_VOX_ABI_VERSION);
        return 1;
    }
    if (mi_vox_resample(NULL, &dst, 9, sigma_a, ca, sigma_b, cb, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "grid") == NULL) return 2;
    dst.res[1] = MI_VOX_MAX_RES + 1;
    if (mi_vox_resample(&src, &dst, 9, sigma_a, ca, sigma_b, cb, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "destination") == NULL) {
        printf("a destination of %d cells was not refused: %s\n", dst.res[1], mi_vox_last_error());
        return 3;
    }
    dst.res[1] = 1;
    if (mi_vox_resample(&src, &dst, 5, sigma_a, ca, sigma_b, cb, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "B=5") == NULL) return 4;
    if (mi_vox_resample(&src, &dst, 9, sigma_a, ca, sigma_a, cb, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "overlaps") == NULL) {
        printf("a destination that is the source was not refused: %s\n", mi_vox_last_error());
        return 5;
    }
    if (mi_vox_resample(&src, &dst, 9, sigma_a, ca, sigma_b, ca, NULL) != MI_VOX_EINVAL) return 6;
    if (mi_vox_resample(&src, &dst, 9, sigma_a, ca, sigma_b, cb + 1, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "aligned") == NULL) return 7;
    if (mi_vox_resample(&src, &dst, 9, sigma_a, NULL, sigma_b, cb, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "NULL") == NULL) return 8;
    if (mi_vox_prune(&src, 9, -1.0f, sigma_a, sigma_b, ca, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "tau") == NULL) {
        printf("a negative tau was not refused: %s\n", mi_vox_last_error());
        return 9;
    }
    if (mi_vox_prune(&src, 9, 0.5f, sigma_a, sigma_a, ca, NULL) != MI_VOX_EINVAL || strstr(mi_vox_last_error(), "sigma_out") == NULL) {
        printf("sigma_out = sigma_in was not refused: %s\n", mi_vox_last_error());
        return 10;
    }
    if (mi_vox_prune(&src, 7, 0.5f, sigma_a, sigma_b, ca, NULL) != MI_VOX_EINVAL) return 11;
    if (mi_vox_prune(&src, 9, 0.5f, sigma_a, sigma_b, NULL, NULL) != MI_VOX_EINVAL) return 12;
    if (mi_vox_prune(NULL, 9, 0.5f, sigma_a, sigma_b, ca, NULL) != MI_VOX_EINVAL) return 13;
    printf("vox refine c_abi consumer ok: ABI %d\n", mi_vox_abi_version());
    return 0;
}
