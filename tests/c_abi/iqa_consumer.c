/* A plain-C consumer of include/mi_nerf_iqa.h: the header is valid C99, libmi_nerf_iqa.so links from C with nothing but the header, and the
 * argument checks answer before any GPU call (this program runs on a box without a GPU).  Built and run by tests/test_iqa_cpu.py. */
#include <stdio.h>
#include <string.h>
#include "mi_nerf_iqa.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi_iqa_last_error()); return 1; } } while (0)

int main(void) {
    double taps[MI_IQA_SSIM_TAPS], sum = 0.0;
    int i;
    float dummy[4];
    EXPECT(mi_iqa_abi_version() == MI_IQA_ABI_VERSION);
    EXPECT(mi_iqa_ssim_window(taps) == MI_IQA_OK);
    for (i = 0; i < MI_IQA_SSIM_TAPS; ++i) sum += taps[i];
    EXPECT(sum > 1.0 - 1e-12 && sum < 1.0 + 1e-12 && taps[0] == taps[MI_IQA_SSIM_TAPS - 1]);
    EXPECT(mi_iqa_ssim_scratch_bytes(1, 800, 800, 1) >= sizeof(double));
    EXPECT(mi_iqa_ssim_downsample_factor(800, 800, 0) == 3 && mi_iqa_ssim_downsample_factor(378, 504, 0) == 1);
    EXPECT(mi_iqa_ssim_scratch_bytes(1, 10, 800, 1) == 0 && strstr(mi_iqa_last_error(), "window") != NULL);
    EXPECT(mi_iqa_ssim(NULL, NULL, 1, 800, 800, 1, 0, NULL, NULL, NULL, 0, NULL) == MI_IQA_EINVAL);
    EXPECT(strlen(mi_iqa_last_error()) > 0);
    EXPECT(mi_iqa_ssim(dummy, dummy, 1, 800, 800, 1, 2u, dummy, NULL, dummy, (size_t)1 << 30, NULL) == MI_IQA_EINVAL);   /* unknown flag */
    EXPECT(strstr(mi_iqa_last_error(), "flag") != NULL);
    printf("iqa c_abi consumer ok: ABI %d\n", mi_iqa_abi_version());
    return 0;
}
