/* A C99 program that sees include/mi_nerf_pose.h alone and links against libmi_nerf_pose.so: the header compiles on its own, the entries
 * resolve, and refusals come back as MI_POSE_EINVAL with a message, before any device is touched. */
#include <stdio.h>
#include <string.h>

#include "mi_nerf_pose.h"

int main(void) {
    float k4[4] = {500.0f, 500.0f, 200.0f, 200.0f};
    float pose12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float word = 0.0f;
    if (mi_pose_abi_version() != MI_POSE_ABI_VERSION) {
        printf("ABI mismatch: library %d, header %d\n", mi_pose_abi_version(), MI_POSE_ABI_VERSION);
        return 1;
    }
    if (mi_pose_reduce_scratch_bytes() < (size_t)MI_POSE_REDUCE_BLOCKS * 16 * sizeof(float)) return 2;
    /* W = 64 has no training kernel */
    if (mi_pose_input_grad(&word, &word, NULL, NULL, 1, 1, NULL, NULL, NULL, &word, 63, NULL, 0, &word, 91, 64, 10, 4, &word, NULL, NULL, NULL, NULL) !=
            MI_POSE_EINVAL || strlen(mi_pose_last_error()) == 0) {
        printf("W = 64 was not refused: %s\n", mi_pose_last_error());
        return 3;
    }
    if (mi_pose_input_grad(NULL, NULL, NULL, NULL, 0, 64, NULL, NULL, NULL, NULL, 63, NULL, 0, NULL, 283, 256, 10, 4, NULL, NULL, NULL, NULL, NULL) != MI_POSE_OK) {
        printf("an empty batch was refused: %s\n", mi_pose_last_error());
        return 4;
    }
    if (mi_pose_ndc_rays_backward(378, 504, 407.5f, 1.0f, &word, 2, &word, 3, 1, NULL, NULL, &word, &word, NULL) != MI_POSE_EINVAL) return 5;
    if (mi_pose_make_o_d_backward(400, 400, k4, pose12, NULL, 0, 400, NULL, &word, &word, NULL, NULL, 0, NULL) != MI_POSE_EINVAL) return 6;
    printf("pose c_abi consumer ok: ABI %d\n", mi_pose_abi_version());
    return 0;
}
