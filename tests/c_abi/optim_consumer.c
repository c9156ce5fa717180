/* A C99 program that sees include/mi_nerf_optim.h alone and links against libmi_nerf_optim.so: the header compiles on its own, the entries
 * resolve, and refusals come back as MI_OPTIM_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_optim.h"

int main(void) {
    float word[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float* params[1];
    const float* grads[1];
    int64_t numel[1] = {4}, off[1] = {0}, step[1] = {1};
    int32_t slot[1] = {0};
    mi_optim_adam_cfg cfg;
    params[0] = word;
    grads[0] = word;
    memset(&cfg, 0, sizeof(cfg));
    cfg.size = (uint32_t)sizeof(cfg);
    cfg.lr = 1e-3;
    cfg.beta1 = 0.9;
    cfg.beta2 = 0.999;
    cfg.eps = 1e-8;
    if (mi_optim_abi_version() != MI_OPTIM_ABI_VERSION) {
        printf("ABI mismatch: library %d, header %d\n", mi_optim_abi_version(), MI_OPTIM_ABI_VERSION);
        return 1;
    }
    if (mi_optim_grad_stats_scratch_bytes(1, numel) != 16) return 2;
    /* step 0 is not a step */
    step[0] = 0;
    if (mi_optim_adam_step(1, params, grads, numel, off, step, word, word, 4, &cfg, 1, NULL, NULL) != MI_OPTIM_EINVAL || strlen(mi_optim_last_error()) == 0) {
        printf("step 0 was not refused: %s\n", mi_optim_last_error());
        return 3;
    }
    step[0] = 1;
    cfg.size = 8; /* a caller built against another layout */
    if (mi_optim_adam_step(1, params, grads, numel, off, step, word, word, 4, &cfg, 1, NULL, NULL) != MI_OPTIM_EINVAL) return 4;
    cfg.size = (uint32_t)sizeof(cfg);
    cfg.beta2 = 1.0;
    if (mi_optim_adam_step_guarded(1, params, grads, numel, off, word, word, 4, &cfg, 1, NULL, slot, 1, word, word, NULL) != MI_OPTIM_EINVAL) return 5;
    cfg.beta2 = 0.999;
    if (mi_optim_grad_stats(1, grads, numel, &cfg, 1, NULL, slot, 1, 0.0f, 1, word, word, word, 16, NULL) != MI_OPTIM_EINVAL) return 6;
    if (mi_optim_grad_stats(1, grads, numel, &cfg, 1, NULL, slot, 1, 1.0f, 1, word, word, word, 15, NULL) != MI_OPTIM_EINVAL) return 7;
    printf("optim c_abi consumer ok: ABI %d\n", mi_optim_abi_version());
    return 0;
}
