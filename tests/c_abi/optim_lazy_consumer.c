/* A C99 program that sees include/mi_nerf_optim.h alone and links against libmi_nerf_optim.so: the lazy entry resolves, takes its gradients
 * writable, and its refusals come back as MI_OPTIM_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_optim.h"

int main(void) {
    float word[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float* params[1];
    float* grads[1];
    float p_min[1] = {0.0f};
    int64_t numel[1] = {4}, off[1] = {0}, step[1] = {1};
    mi_optim_adam_cfg cfg;
    params[0] = word;
    grads[0] = word;
    memset(&cfg, 0, sizeof(cfg));
    cfg.size = (uint32_t)sizeof(cfg);
    cfg.lr = 1e-3;
    cfg.beta1 = 0.9;
    cfg.beta2 = 0.999;
    cfg.eps = 1e-8;
    if (mi_optim_abi_version() != MI_OPTIM_ABI_VERSION || MI_OPTIM_ABI_VERSION < 2) {
        printf("ABI mismatch: library %d, header %d\n", mi_optim_abi_version(), MI_OPTIM_ABI_VERSION);
        return 1;
    }
    /* consume is 0 or 1 */
    if (mi_optim_adam_step_lazy(1, params, grads, numel, off, step, word, word, 4, &cfg, 1, NULL, p_min, 2, NULL) != MI_OPTIM_EINVAL ||
        strlen(mi_optim_last_error()) == 0) {
        printf("consume = 2 was not refused: %s\n", mi_optim_last_error());
        return 2;
    }
    /* a lazy weight decay is not defined */
    cfg.weight_decay = 0.01;
    if (mi_optim_adam_step_lazy(1, params, grads, numel, off, step, word, word, 4, &cfg, 1, NULL, NULL, 1, NULL) != MI_OPTIM_EINVAL) return 3;
    printf("optim lazy c_abi consumer ok: ABI %d\n", mi_optim_abi_version());
    return 0;
}
