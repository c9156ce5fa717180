/* A plain-C consumer of include/mi_nerf_occ.h: the header (and mi_nerf.h, which it includes) is valid C99, libmi_nerf_occ.so links from C
 * with nothing but the headers and finds libmi_nerf.so beside itself, and the argument checks answer before any GPU call (this program
 * runs on a box without a GPU).  Built and run by tests/test_occ_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_occ.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_occ_last_error()); return 1; } } while (0)

int main(void) {
    mi_occ_grid g;
    mi_nerf_render_cfg cfg;
    mi_nerf_net net;
    mi_occ_workspace_layout lay;
    mi_occ_stats stats;
    float dummy[8];
    uint32_t words[4];
    int i;
    for (i = 0; i < 3; ++i) { g.lo[i] = -1.5f; g.hi[i] = 1.5f; g.res[i] = 128; }
    g.outside_occupied = 1;
    memset(&cfg, 0, sizeof cfg);
    cfg.near_ = 2.0f; cfg.far_ = 6.0f; cfg.Sc = 64; cfg.Nf = 128; cfg.mode = MI_NERF_MODE_F32;
    net.D = 8; net.W = 256; net.skip = 4; net.L_x = 10; net.L_d = 4;
    EXPECT(mi_occ_abi_version() == MI_OCC_ABI_VERSION);
    EXPECT(mi_occ_grid_words(&g) == (size_t)128 * 128 * 128 / 32);
    g.res[1] = 3; g.res[2] = 1;
    EXPECT(mi_occ_grid_words(&g) == 12);                                   /* 384 cells */
    g.res[0] = 5;
    EXPECT(mi_occ_grid_words(&g) == 1);                                    /* 15 cells: one word */
    g.res[0] = MI_OCC_MAX_RES + 1;
    EXPECT(mi_occ_grid_words(&g) == 0 && strstr(mi_occ_last_error(), "res") != NULL);
    g.res[0] = 128; g.res[1] = 128; g.res[2] = 128;
    EXPECT(mi_occ_bake_scratch_bytes(&g, 2) > 0 && mi_occ_bake_scratch_bytes(&g, MI_OCC_MAX_SUB + 1) == 0);
    EXPECT(mi_occ_render_workspace_layout(&cfg, 1024, &lay) == MI_OCC_OK && lay.total == mi_occ_render_workspace_bytes(&cfg, 1024));
    EXPECT(lay.z_c == 0 && lay.raw_c == (size_t)1024 * 64 * 4 && lay.total > lay.tile_raw);
    EXPECT(mi_occ_render_rays(NULL, NULL, NULL, &cfg, &g, NULL, NULL, NULL, 1024, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL) == MI_OCC_EINVAL);
    EXPECT(strlen(mi_occ_last_error()) > 0);
    cfg.mode = MI_NERF_MODE_F16_BF16;                                      /* a two-family mode: refused */
    EXPECT(mi_occ_render_rays(&net, dummy, dummy, &cfg, &g, words, words, dummy, 1024, NULL, NULL, dummy, (size_t)1 << 40, dummy, dummy, dummy, dummy, &stats,
                              NULL) == MI_OCC_EINVAL);
    EXPECT(strstr(mi_occ_last_error(), "mode") != NULL);
    EXPECT(mi_occ_mark(&g, NULL, dummy, dummy, 4, 2, NULL, NULL) == MI_OCC_EINVAL);
    EXPECT(mi_occ_dilate(&g, words, words, 1, NULL) == MI_OCC_EINVAL && strstr(mi_occ_last_error(), "out of place") != NULL);
    printf("occ c_abi consumer ok: ABI %d\n", mi_occ_abi_version());
    return 0;
}
