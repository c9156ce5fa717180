/* A plain-C consumer of include/mi_nerf_geo.h: the header is valid C99 on its own, libmi_nerf_geo.so links from C with nothing but the
 * header, and the argument checks answer before any GPU call (this program runs on a box without a GPU).  Built and run by
 * tests/test_geo_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_geo.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_geo_last_error()); return 1; } } while (0)

int main(void) {
    /* 16-byte aligned stand-ins for device buffers: no call below gets as far as reading them */
    static union { float f[16]; long double align; } buf;
    float* dummy = buf.f;
    EXPECT(mi_geo_abi_version() == MI_GEO_ABI_VERSION);
    EXPECT(strcmp(mi_geo_last_error(), "") == 0);
    EXPECT(mi_geo_composite(dummy, dummy, dummy, 6, 4, 0, 2.0f, 6.0f, dummy, dummy, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "S=") != NULL);
    EXPECT(mi_geo_composite(dummy, dummy, dummy, 6, 4, MI_GEO_MAX_SAMPLES + 1, 2.0f, 6.0f, dummy, dummy, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(mi_geo_composite(dummy, dummy, dummy, 4, 4, 64, 2.0f, 6.0f, dummy, dummy, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "ray_stride") != NULL);
    EXPECT(mi_geo_composite(dummy, dummy, dummy, 6, 4, 64, 6.0f, 2.0f, dummy, dummy, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "near") != NULL);
    EXPECT(mi_geo_composite(NULL, dummy, dummy, 6, 4, 64, 2.0f, 6.0f, dummy, dummy, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(mi_geo_composite_backward(dummy, dummy, dummy, 3, 4, 64, 2.0f, 6.0f, dummy, NULL, NULL, NULL, NULL, NULL, NULL) == MI_GEO_EINVAL);
    EXPECT(strstr(mi_geo_last_error(), "d_raw") != NULL);
    EXPECT(mi_geo_composite_backward(dummy, dummy, dummy, 3, -1, 64, 2.0f, 6.0f, dummy, NULL, NULL, NULL, NULL, dummy, NULL) == MI_GEO_EINVAL);
    EXPECT(mi_geo_composite_backward(NULL, NULL, NULL, 3, 0, 64, 2.0f, 6.0f, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == MI_GEO_OK);
    EXPECT(mi_geo_composite(NULL, NULL, NULL, 6, 0, 64, 2.0f, 6.0f, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == MI_GEO_OK);
    printf("geo c_abi consumer ok: ABI %d\n", mi_geo_abi_version());
    return 0;
}
