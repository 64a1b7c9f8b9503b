/* pikazoo_optim.h -- C ABI of libpikazoo_optim.so: the optimizer step of a PPO update -- the global gradient norm, the clip
 * and the Adam / AdamW update of every parameter tensor of one or two nets, with the moments and the step count, in ONE launch.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path, pikazoo_amd.learn, pikazoo_amd.policy,
 * pikazoo_amd.ppo, pikazoo_amd.net or pikazoo_amd.netgrad loads it.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1,
 * PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of the launch).
 *
 * `groups` and `cfg` are HOST structs: they are read at call time and copied into the kernel's arguments, so a captured
 * graph holds them by value and there is no pointer table in device memory that a replay could find changed.  The pointers
 * inside them are caller-owned device memory.  One launch on `stream`, no allocation, no workspace, no synchronisation:
 * graph-capturable.  The parameters are updated in place: pz_mlp_forward reads the same storage.
 *
 * A GROUP is one net's parameters: everything that shares one gradient norm and one step count.  n_groups is 1 or 2 (the two
 * agents' separate nets; a shared net is one group).  A group holds 1..PZ_OPTIM_MAX_TENSORS tensors, each float32, contiguous
 * and 4-byte aligned, of numel >= 1 elements, sum(numel) <= PZ_OPTIM_MAX_ELEMENTS, and
 *     step        device, 2 x int64, 8-byte aligned: step[0] = t, the number of updates made; step[1] = skipped
 *     stats       device, 2 x float32, or NULL: stats[0] = grad_norm, stats[1] = clip_coef of this call
 *     lr_device   device, 1 x float32, or NULL: when non-NULL its value replaces cfg->lr (read by the kernel at run time: the
 *                 way to anneal under a captured graph; it is not range-checked)
 * param, exp_avg and exp_avg_sq must not overlap each other, a gradient, step or stats (not checked here).
 *
 * THE DEFINITION, per group.  G is the concatenation of the group's gradient tensors in their order, N elements.
 *   S      = sum of (double) G[e] * (double) G[e], in float64 (each product is exact), in THIS order: thread j of 1024 adds
 *            its elements e = j, j + 1024, j + 2048, ... in increasing order onto +0; the 64 threads of a wave
 *            (j >> 6) combine by x <- x + x[lane ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; the 16 wave sums are added in index
 *            order, w0 + w1 first.  A float64 sum of float32 squares cannot overflow, so S is non-finite exactly when a
 *            gradient element is.
 *   norm   = (float) sqrt(S)                           (float64 square root, rounded to float32 once)
 *   The hyperparameters are FLOAT64 on the host, the numbers torch's optimizers compute with; each float32 constant of the
 *   update is rounded from float64 ONCE, as torch's scalars are when they meet a float32 tensor:
 *     max_f = (float) max_grad_norm;   omb1 = (float) (1.0 - beta1);   omb2 = (float) (1.0 - beta2);   beta2_f = (float) beta2
 *     eps_f = (float) eps;             wd_f = (float) weight_decay
 *   clipping = max_f > 0 and max_f < +inf              (<= 0, +inf or NaN: no clipping)
 *   coef   = 1.0f without clipping; else c = max_f / (norm + 1e-6f) in float32, coef = c > 1.0f ? 1.0f : c
 *            (torch.nn.utils.clip_grad_norm_, norm_type 2; a NaN c stays NaN, an infinite norm gives coef 0)
 *   stats  = {norm, coef} when stats is non-NULL, in every case.
 *   If skip_nonfinite is set and norm is not finite: skipped += 1 and NOTHING else of the group is written: params, moments
 *   and t keep their bits.
 *   Otherwise t += 1 and, with lr = lr_device ? (double) *lr_device : cfg->lr, in float64 from the int64 t, rounded once:
 *     step_size = (float) (lr / (1.0 - pow(beta1, (double) t)))
 *     bc2       = (float) sqrt(1.0 - pow(beta2, (double) t))
 *     decay     = (float) (1.0 - lr * weight_decay)
 *   and per element (p, g, m, v), in float32, one rounding per operation, nothing contracted:
 *     g1 = coef * g
 *     if weight_decay != 0 and not decoupled:  g1 = fma(wd_f, p, g1)                  (Adam's L2 term)
 *     if weight_decay != 0 and decoupled:      p = p * decay                          (AdamW)
 *     d  = g1 - m;        m' = fma(omb1, d, m)                                        (torch's lerp)
 *     a  = beta2_f * v;   gg = g1 * g1;      v' = fma(omb2, gg, a)
 *     r  = sqrt(v');      q  = r / bc2;      den = q + eps_f                           (sqrt and / correctly rounded)
 *     u  = m' / den;      p' = fma(-step_size, u, p)
 *   This is torch.optim.Adam / AdamW with amsgrad=False, maximize=False.  (eps = 0 and v' = 0 give 0 / 0 = NaN, as there.)
 * WHAT A NaN REACHES follows from these lines.  With skip_nonfinite = 0 and clipping, a NaN gradient element makes norm and
 * coef NaN and thereby every param and moment of its group NaN, as in torch; t advances.  An infinite element gives
 * norm = +inf and coef = 0: that element's 0 * inf is NaN, the others see a zero gradient.  Without clipping coef is 1 and only
 * the element itself is reached.  The other group never sees any of it: the groups are independent, and a group's bits do
 * not depend on the other's presence.
 * GRADIENTS ARE CONST: the clipped gradient is never written back (clip_grad_norm_ scales .grad in place; this call does
 * not), and nothing is zeroed.
 *
 * THE BITS DEPEND ON THE INPUTS ONLY: one workgroup of 1024 threads per group, no atomics, nothing that depends on the
 * device's compute-unit count.  They do not depend on the tensors' addresses either: a tensor whose four bases share their
 * offset within 16 bytes is walked with 16-byte accesses behind a scalar head, any other with 4-byte accesses, and an element's
 * arithmetic is the same on both routes.
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    groups, cfg, a tensor pointer (param, grad, exp_avg, exp_avg_sq) or step is NULL;
 *   PZ_E_SIZE    n_groups outside 1..2, count outside 1..16, a numel < 1, sum(numel) > 2^20;
 *   PZ_E_CONFIG  lr < 0 or NaN; a beta outside [0, 1) (as float64); eps < 0 or NaN; weight_decay < 0 or NaN; decoupled or skip_nonfinite
 *                other than 0 / 1;
 *   PZ_E_ALIGN   a float pointer (stats and lr_device included) not 4-byte aligned, or step not 8-byte aligned.
 */
#ifndef PIKAZOO_OPTIM_H
#define PIKAZOO_OPTIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_OPTIM_ABI_VERSION 1
#define PZ_OPTIM_MAX_TENSORS 16
#define PZ_OPTIM_MAX_GROUPS 2
#define PZ_OPTIM_MAX_ELEMENTS (1 << 20)

typedef struct pz_optim_tensor {
    int64_t numel;
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
} pz_optim_tensor;

typedef struct pz_optim_group {
    int32_t count; /* tensors in use: 1..PZ_OPTIM_MAX_TENSORS */
    pz_optim_tensor tensors[PZ_OPTIM_MAX_TENSORS];
    int64_t *step;          /* {t, skipped} */
    float *stats;           /* {grad_norm, clip_coef}, or NULL */
    const float *lr_device; /* or NULL: cfg->lr */
} pz_optim_group;

typedef struct pz_adam_config {
    double lr, beta1, beta2, eps, weight_decay; /* float64, as Python and torch hold them */
    double max_grad_norm;   /* <= 0, +inf or NaN (as a float32): no clipping */
    int32_t decoupled;      /* 0: Adam's L2 term, 1: AdamW */
    int32_t skip_nonfinite; /* 1: a non-finite norm skips the group's update */
} pz_adam_config;

int pz_optim_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_optim_build_id(void);

int pz_adam_step(const pz_optim_group *groups, int32_t n_groups, const pz_adam_config *cfg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_OPTIM_H */
