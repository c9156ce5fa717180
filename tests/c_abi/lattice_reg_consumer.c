/* A plain-C consumer of THE LATTICE REGULARISERS of include/mi_nerf_geo.h: the header is valid C99 on its own, the new entries link from C,
 * and their argument checks answer before any GPU call (this program runs on a box without a GPU).  Built and run by
 * tests/test_lattice_reg_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_geo.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_geo_last_error()); return 1; } } while (0)

int main(void) {
    /* 16-byte aligned stand-ins for device buffers, each as large as the 9 x 17 x 5 x 4 array it stands for (the entries refuse arrays that
     * overlap): no call below gets as far as reading them */
    static union { float f[9 * 17 * 5 * 4]; double d[8]; long double align; } a, b, s;
    const int32_t good[3] = {9, 17, 5}, bad[3] = {9, 1, 5}, big[3] = {9, MI_GEO_LATTICE_MAX_POINTS + 1, 5};
    EXPECT(mi_geo_abi_version() == MI_GEO_ABI_VERSION && MI_GEO_ABI_VERSION == 2);
    EXPECT(mi_geo_lattice_scratch_bytes(good, 4, 3) > 0);
    EXPECT(mi_geo_lattice_scratch_bytes(bad, 4, 3) == 0 && mi_geo_lattice_scratch_bytes(big, 4, 3) == 0 && mi_geo_lattice_scratch_bytes(NULL, 4, 3) == 0);
    EXPECT(mi_geo_lattice_tv(bad, 4, 3, a.f, NULL, 1e-8f, 1.0f, b.f, NULL, NULL, 0, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "P=") != NULL);
    EXPECT(mi_geo_lattice_sparsity(big, a.f, NULL, 1.0f, b.f, NULL, NULL, 0, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "mi_geo_lattice_sparsity") != NULL && strstr(mi_geo_last_error(), "P=") != NULL);
    EXPECT(mi_geo_lattice_tv(good, 4, 3, a.f, NULL, 0.0f, 1.0f, b.f, NULL, NULL, 0, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "eps") != NULL);
    EXPECT(mi_geo_lattice_tv(good, 4, 3, a.f, NULL, 1e-8f, 1.0f, b.f, s.d, s.d, 8, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "scratch") != NULL);
    /* no output asked for: the arguments are checked and nothing is launched */
    EXPECT(mi_geo_lattice_tv(good, 4, 3, a.f, NULL, 1e-8f, 1.0f, NULL, NULL, NULL, 0, NULL) == MI_GEO_OK);
    EXPECT(mi_geo_lattice_sparsity(good, a.f, NULL, 1.0f, NULL, NULL, NULL, 0, NULL) == MI_GEO_OK);
    printf("lattice_reg c_abi consumer ok: ABI %d\n", mi_geo_abi_version());
    return 0;
}
