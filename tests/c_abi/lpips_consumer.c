/* A C99 program that sees include/mi_nerf_lpips.h alone and links against libmi_nerf_lpips.so: the header compiles on its own, the entries
 * resolve, and a refusal comes back as MI_LPIPS_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_lpips.h"

int main(void) {
    mi_lpips_net net;
    float word[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    size_t params = 0;
    int k, c = 3, taps = 0;
    if (mi_lpips_abi_version() != MI_LPIPS_ABI_VERSION) {
        printf("ABI mismatch: library %d, header %d\n", mi_lpips_abi_version(), MI_LPIPS_ABI_VERSION);
        return 1;
    }
    if (mi_lpips_vgg16(&net) != MI_LPIPS_OK || net.n_ops != 22 || net.cin0 != 3) return 2;
    for (k = 0; k < net.n_ops; ++k) {
        if (net.ops[k].kind == MI_LPIPS_CONV) {
            params += (size_t)9 * c * net.ops[k].cout + net.ops[k].cout;
            c = net.ops[k].cout;
        } else if (net.ops[k].kind == MI_LPIPS_TAP) {
            params += c;
            ++taps;
        }
    }
    if (taps != 5 || mi_lpips_packed_bytes(&net) < params * sizeof(float)) return 3;
    /* 15 x 15 cannot be halved four times */
    if (mi_lpips_distance(&net, word, 1u << 30, word, word, 1, 15, 15, word, NULL, word, 1u << 30, NULL) != MI_LPIPS_EINVAL ||
        strlen(mi_lpips_last_error()) == 0) {
        printf("a 15 x 15 image was not refused: %s\n", mi_lpips_last_error());
        return 4;
    }
    net.ops[0].kind = MI_LPIPS_TAP;
    if (mi_lpips_packed_bytes(&net) != 0 || strlen(mi_lpips_last_error()) == 0) return 5;
    printf("lpips c_abi consumer ok: ABI %d\n", mi_lpips_abi_version());
    return 0;
}
