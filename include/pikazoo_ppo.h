/* pikazoo_ppo.h -- C ABI of libpikazoo_ppo.so: the PPO update loss over a minibatch of logit rows -- the loss, its logging
 * statistics and its gradients with respect to the logits and the values, from ONE pass over the rows.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path, pikazoo_amd.learn or pikazoo_amd.policy loads it.
 * Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is
 * the hipError_t of a launch).
 *
 * Common to the calls: pointers are caller-owned device memory; every launch goes to `stream`, no allocation, no
 * synchronisation: graph-capturable.  Agent 2's pointers are ALL NULL (one side only) or non-NULL exactly where agent 1's
 * are.  Both agents share the formats, num_actions, the pitches, the coefficients and the launches.  Outputs must not alias
 * any input or each other.  The logit rows, their formats and the action vectors are pikazoo_policy.h's, rule for rule
 * (enum pz_policy_logit_format, enum pz_policy_action_format); the value formats are the logit formats' values.
 *
 * THE REDUCTIONS ARE DETERMINISTIC.  No floating-point atomic accumulates anything: every wave reduces its rows in a fixed
 * order and writes its partial sums into `workspace` with plain stores; a second, small launch on the same stream sums the
 * partials in the order of their index.  Two calls on the same inputs return the same bits, whatever order the workgroups
 * ran in.  `workspace` is caller-owned scratch of pz_ppo_workspace_bytes(n) bytes, aligned to 16 bytes, shared by both
 * agents of a call and by pz_ppo_moments and the pz_ppo_loss behind it on one stream, never by two calls in flight.
 */
#ifndef PIKAZOO_PPO_H
#define PIKAZOO_PPO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_PPO_ABI_VERSION 1

int pz_ppo_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_ppo_build_id(void);

/* bytes of scratch that pz_ppo_moments and pz_ppo_loss need for n rows (of one or both agents); 0 for n <= 0 or n > 2^30 */
int64_t pz_ppo_workspace_bytes(int64_t n);

/* ---- mean and reciprocal scale of a vector: the advantage normalisation -------------------------------------------------
 * x_*: float32[n].  out: float32[2][2], {mean, rscale} per agent (agent 2's pair is not written for one side), with
 *     mean = sum x / n,   rscale = 1 / (std + eps),   std = sqrt(sum (x - mean)^2 / (n - 1))     (the UNBIASED deviation:
 * what (adv - adv.mean()) / (adv.std() + 1e-8) uses).  Accumulated in float64 about the shift K = x[0], as
 * sum (x - K) and sum (x - K)^2 (x - K is exact in float64): a mean far above the spread costs nothing, which a sum of x^2
 * would not survive.  Fixed order; two launches.
 *   PZ_E_NULL    x_p1, out or workspace is NULL;      PZ_E_SIZE   n < 2 (n == 0 is PZ_OK without a launch) or n > 2^30;
 *   PZ_E_CONFIG  eps not finite or < 0;                PZ_E_ALIGN  x, out not aligned to 4 bytes, workspace to 16. */
int pz_ppo_moments(const float *x_p1, const float *x_p2, int64_t n, float eps, float *out, void *workspace, void *stream);

/* ---- the PPO loss, its statistics and its gradients ----------------------------------------------------------------------
 * Inputs per agent: logits [n, num_actions] at logit_pitch and act [n] as in pikazoo_policy.h; old_logp, adv, ret:
 * float32[n] (what pz_sample_actions and pz_gae wrote); values: one element per row at value_pitch ELEMENTS, of
 * value_format -- so the value may be column num_actions of the [n, num_actions + 1] tensor the logits are a view of;
 * old_values: [n] of old_value_format, required iff value_clip > 0 (ignored otherwise); adv_norm: NULL (the advantages
 * are used as they are) or the float32[2][2] that pz_ppo_moments wrote -- a device pointer, so that the two calls sit in
 * one captured graph.
 *
 * Outputs: grad_logits_*: n rows in the logits' format (rounded to nearest even) at grad_pitch >= num_actions, pad columns
 * not written; grad_values_*: one element per row at grad_value_pitch, in value_format (it may be column num_actions of
 * the same gradient tensor); either pair may be NULL.  stats: float32[2][8], per agent
 *     {loss, policy_loss, value_loss, entropy, approx_kl, clip_fraction, +0, +0}      (agent 2's row not written for one side).
 *
 * Per row of an agent, with M = n; lp and H are what pz_action_log_probs returns for the row (the same row statistics, the
 * same bits); in float32:
 *     d    = lp - old_logp;   r = exp(d)
 *     Ahat = adv_norm ? (adv - mean) * rscale : adv
 *     pg   = max(-Ahat * r, -Ahat * clamp(r, 1 - clip, 1 + clip))
 *     g_lp = -Ahat * r, but 0 where (r > 1 + clip and Ahat > 0) or (r < 1 - clip and Ahat < 0)
 *     e    = v - ret;  vl = 0.5 e^2;  g_v = e
 *       with value_clip > 0:  vc = old_v + clamp(v - old_v, -value_clip, value_clip);  ec = vc - ret
 *            if ec^2 > e^2:  vl = 0.5 ec^2;  g_v = (|v - old_v| <= value_clip) ? ec : 0
 *     kl   = (r - 1) - d;    cf = (|r - 1| > clip) ? 1 : 0
 * policy_loss = mean pg, value_loss = mean vl, entropy = mean H, approx_kl = mean kl, clip_fraction = mean cf, and
 *     loss = policy_loss + vf_coef * value_loss - ent_coef * entropy.
 * The gradients are those of `loss`: grad_logits is pikazoo_policy.h's backward formula with glogp = g_lp / M and
 * gent = -ent_coef / M; grad_values = vf_coef * g_v / M.
 *
 * A row of pikazoo_policy.h's step 6, or one whose action lies outside [0, num_actions), yields NaN gradients for its
 * logits and makes loss, policy_loss, approx_kl and clip_fraction NaN (a NaN ratio counts as NaN, not as "not clipped");
 * entropy is NaN only for a step-6 row.  Nothing is hidden.
 *
 * The sums: a wave adds its 64 rows as a butterfly in float32, the partials are summed in float64 in index order, the
 * means and the loss are formed in float64 and rounded once.  With old_logp from pz_action_log_probs (or
 * pz_sample_actions) on the same logits and actions, d == +0 and r == 1 in every row, and approx_kl and clip_fraction are
 * +0 bit for bit.
 *
 * Checked before the launches, in this order:
 *   PZ_E_NULL    logits, act, old_logp, adv, ret, values of agent 1, stats or workspace is NULL; old_values NULL with
 *                value_clip > 0; agent 2's pointers are a mix of NULL and non-NULL;
 *   PZ_E_SIZE    n < 0, n > 2^30, num_actions outside [2, 32], logit_pitch < num_actions, grad_pitch < num_actions (with
 *                grad_logits), value_pitch < 1, grad_value_pitch < 1 (with grad_values), n * pitch * 4 bytes beyond int64;
 *   PZ_E_CONFIG  an unknown format; clip not finite or outside (0, 1); value_clip not finite or < 0; vf_coef or ent_coef
 *                not finite or < 0;
 *   PZ_E_ALIGN   a pointer not aligned to its element (logits, values 4 or 2 bytes, actions 4 or 8, floats 4), workspace
 *                not aligned to 16.
 * n == 0 returns PZ_OK without a launch. */
int pz_ppo_loss(const void *logits_p1, const void *logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                int64_t logit_pitch, int32_t action_format, const void *act_p1, const void *act_p2, const float *old_logp_p1,
                const float *old_logp_p2, const float *adv_p1, const float *adv_p2, const float *ret_p1, const float *ret_p2,
                const void *values_p1, const void *values_p2, int32_t value_format, int64_t value_pitch,
                const void *old_values_p1, const void *old_values_p2, int32_t old_value_format, const float *adv_norm,
                float clip, float value_clip, float vf_coef, float ent_coef, void *grad_logits_p1, void *grad_logits_p2,
                int64_t grad_pitch, void *grad_values_p1, void *grad_values_p2, int64_t grad_value_pitch, float *stats,
                void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_PPO_H */
