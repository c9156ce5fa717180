/*
 * mi_nerf_optim.h -- C ABI of libmi_nerf_optim.so: the optimiser step of the MI355X (gfx950) NeRF training loop.
 *
 * A library of its own BESIDE the path: include/mi_nerf.h and the other side headers stay what they are, nothing here is declared there,
 * and libmi_nerf_optim.so exports no symbol of the other libraries and links against none of them.  Same conventions: plain C99, raw device
 * pointers, the caller allocates everything, int status (0 = ok), hipStream_t passed as void*, every argument checked before any HIP call,
 * error text through mi_optim_last_error().  No entry synchronises with the host, copies to or from the device, allocates, or uses an
 * atomic: the per-tensor table of a launch travels as kernel arguments, every sum is taken in a fixed order, results are bit-reproducible.
 *
 * THE UPDATE, per element, in fp32 (Adam as torch.optim.Adam evaluates it; g is the gradient, c the clip coefficient, 1 in plain mode):
 *     g  <- c g                                   (guarded mode)
 *     g  <- g + wd p                              (weight_decay != 0, not decoupled: L2)
 *     p  <- p (1 - lr wd)                         (weight_decay != 0, decoupled: AdamW)
 *     m  <- beta1 m + (1 - beta1) g
 *     v  <- beta2 v + (1 - beta2) g g
 *     p  <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),      bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * evaluated with the fused multiply-adds of PyTorch's CPU kernels: g = fma(wd, p, g), m = fma(1 - beta1, g - m, m) (lerp),
 * v = fma((1 - beta2) g, g, beta2 v); square root and divisions are correctly rounded.
 * The constants 1 - beta1, 1 - beta2, 1 - lr wd, lr / bc1 and sqrt(bc2) are formed in double and then rounded to float -- on the host in
 * plain mode, in the finishing kernel of mi_optim_grad_stats in guarded mode, by the same routine, so both modes use the same bits.
 * (1.0f - 0.999f is off by 1.3e-5 relative; formed in float it alone puts exp_avg_sq tens of times further from the float64 result than
 * PyTorch's own fp32 Adam is.)
 *
 * THE TENSOR LIST.  Every entry takes n separate fp32 tensors as HOST arrays: params[i] / grads[i] (device pointers, 4-byte aligned),
 * numel[i] >= 0 (0: the tensor is a no-op and its pointers may be NULL), state_off[i] (the element at which tensor i's moments start in
 * BOTH flat arenas exp_avg and exp_avg_sq, which hold state_numel floats each), and cfg_of[i] (which of the n_cfg configurations tensor i uses; NULL: all use cfgs[0]).
 * A launch serves at most MI_OPTIM_MAX_TENSORS consecutive tensors of one configuration; a longer or mixed list is split into several
 * launches inside the call.  Each workgroup takes one chunk of MI_OPTIM_CHUNK elements of one tensor; it uses 16-byte accesses when that
 * tensor's four addresses (p, g, m, v) are 16-byte aligned and 4-byte accesses for the whole tensor otherwise.
 *
 * THE LAZY UPDATE (mi_optim_adam_step_lazy), for a table of which a step's gradient reaches a small part.  An element is TOUCHED iff
 * g != 0 as an IEEE comparison: -0.0 is untouched, NaN is touched and propagates as in PyTorch.
 *     untouched:  p, m and v are neither read nor written.  Nothing decays for the skipped step and nothing catches up later: the element
 *                 is exactly what it was when its last gradient arrived.
 *     touched:    THE UPDATE with c = 1, by the same routine as the plain step; the bias corrections come from step[i], the TENSOR's step
 *                 count (not the element's), a host array as in mi_optim_adam_step.  Then the clamp, p = p < p_min[i] ? p_min[i] : p (a NaN
 *                 stays NaN; -inf: no clamp).  With consume = 1 the element's gradient is overwritten with +0.0f in the same pass: after
 *                 the call the gradient tensor compares equal to zero everywhere and the next backward adds into it without a memset
 *                 (the zero is stored per 16-byte piece: a -0.0 that shares a piece with a touched element becomes +0.0 as well).
 *                 With consume = 0 no gradient byte changes.
 * weight_decay != 0 is refused: a lazy decay has more than one meaning and none is chosen here.  The launch shape is THE TENSOR LIST's; a
 * launch is split where p_min changes as it is where the configuration changes.  A thread reads its gradients first and reads p, m, v
 * only for a 16-byte piece (the 4-byte path: an element) in which some g != 0; it stores only such a piece, and inside one the untouched
 * components are stored back with the bits that were loaded.  An untouched chunk costs its 16 KiB of gradient reads and nothing else.
 */
#ifndef MI_NERF_OPTIM_H
#define MI_NERF_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OPTIM_ABI_VERSION 2

/* status codes (the values of mi_nerf.h) */
#define MI_OPTIM_OK 0
#define MI_OPTIM_EINVAL 1   /* bad argument / unsupported shape */
#define MI_OPTIM_EHIP 2     /* HIP runtime error */

#define MI_OPTIM_MAX_TENSORS 80      /* tensors per launch: 48 bytes of kernel arguments each, the whole table stays below 4 KB */
#define MI_OPTIM_CHUNK 4096          /* elements per workgroup */
#define MI_OPTIM_CONTROL_WORDS 8     /* the control block: 8 words of 4 bytes */
#define MI_OPTIM_TSTATE_WORDS 4      /* per-tensor device state: 4 floats */

/* One parameter group's hyper-parameters.  size = sizeof(mi_optim_adam_cfg): a caller built against another layout is refused. */
typedef struct mi_optim_adam_cfg {
    uint32_t size;
    int32_t decoupled;               /* 0: L2 (torch.optim.Adam), 1: decoupled (torch.optim.AdamW) */
    double lr;                       /* doubles, as PyTorch holds them: the constants of THE UPDATE are rounded to float once, after */
    double beta1, beta2;             /* they are formed; betas in [0, 1) */
    double eps;
    double weight_decay;             /* >= 0 */
    uint32_t reserved[2];            /* 0 */
} mi_optim_adam_cfg;

/* THE CONTROL BLOCK of one guarded step, on the device, written by the finishing kernel of mi_optim_grad_stats with ordinary stores:
 *   word 0  float     the global L2 norm of the gradients (summed in double, rounded once)
 *   word 1  float     the clip coefficient c = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; NaN stays NaN); 1 when
 *                     max_norm is +inf
 *   word 2  uint32    how many gradient elements are not finite (saturates at 2^32 - 1)
 *   word 3  uint32    1: this step is skipped (skip_nonfinite and word 2 != 0), 0: applied
 *   word 4  uint32    how many steps have been skipped so far (the caller zeroes the block once; this word accumulates)
 *   words 5-7         0
 * PER-TENSOR DEVICE STATE, tstate[slot] = 4 floats: step (as torch's capturable state keeps it), 1 - beta1^step, sqrt(1 - beta2^step),
 * lr / (1 - beta1^step).  The caller zeroes it once; the finishing kernel advances step and rewrites the other three -- one thread per
 * tensor -- only when the step is applied, so a skipped step advances nothing (PyTorch's found_inf semantics). */

int mi_optim_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* mi_optim_last_error(void);

/* The plain step: THE UPDATE with c = 1 over THE TENSOR LIST; step[i] >= 1 is the number of the step being taken for tensor i (a host
 * array: the bias corrections travel as kernel arguments). */
int mi_optim_adam_step(int n, float* const* params, const float* const* grads, const int64_t* numel, const int64_t* state_off,
                       const int64_t* step, float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                       const int32_t* cfg_of, void* stream);

/* THE LAZY UPDATE over THE TENSOR LIST, grads writable.  p_min: a host array of n floats (NULL: no clamp anywhere; a NaN is refused);
 * consume: 0 / 1; every configuration's weight_decay must be 0. */
int mi_optim_adam_step_lazy(int n, float* const* params, float* const* grads, const int64_t* numel, const int64_t* state_off,
                            const int64_t* step, float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                            const int32_t* cfg_of, const float* p_min, int consume, void* stream);

/* bytes of scratch mi_optim_grad_stats needs for this tensor list (16-byte aligned; one 16-byte partial per workgroup); 0 when an
 * argument is bad */
size_t mi_optim_grad_stats_scratch_bytes(int n, const int64_t* numel);

/* The first half of a guarded step.  Stage 1: one workgroup per chunk writes (sum of squares in double, count of non-finite elements) of
 * its chunk into `scratch`.  The finishing launch, one workgroup: each thread adds a contiguous run of partials in index order, the 256
 * thread sums are added in a fixed tree; then THE CONTROL BLOCK is written and, when the step is applied, the PER-TENSOR DEVICE STATE of
 * slot[i] (distinct, in [0, n_slots)) is advanced with the hyper-parameters of tensor i's configuration.
 * max_norm > 0 (+inf: no clipping); skip_nonfinite 0 / 1. */
int mi_optim_grad_stats(int n, const float* const* grads, const int64_t* numel, const mi_optim_adam_cfg* cfgs, int n_cfg, const int32_t* cfg_of,
                        const int32_t* slot, int n_slots, float max_norm, int skip_nonfinite, float* tstate, void* control, void* scratch,
                        size_t scratch_bytes, void* stream);

/* The second half: THE UPDATE with c, the skip decision and the bias corrections read on the device from `control` and `tstate` as
 * mi_optim_grad_stats left them for the same list.  A skipped step writes nothing. */
int mi_optim_adam_step_guarded(int n, float* const* params, const float* const* grads, const int64_t* numel, const int64_t* state_off,
                               float* exp_avg, float* exp_avg_sq, int64_t state_numel, const mi_optim_adam_cfg* cfgs, int n_cfg,
                               const int32_t* cfg_of, const int32_t* slot, int n_slots, const float* tstate, const void* control, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_NERF_OPTIM_H */
