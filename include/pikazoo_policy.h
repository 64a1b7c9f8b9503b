/* pikazoo_policy.h -- C ABI of libpikazoo_policy.so: the categorical policy head between a policy net's last Linear and
 * env.step().  Sampling, log-probability and entropy from logits in ONE launch, and the update-side pair (log-probability
 * and entropy of GIVEN actions, forward and backward).
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, knows nothing of pz_config or the game state, and nothing in the step path
 * loads it.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a
 * positive value is the hipError_t of the launch).
 *
 * Common to the three launches: pointers are caller-owned device memory; one launch on `stream`, no allocation, no
 * synchronisation: graph-capturable.  Agent 2's pointers are ALL NULL (one side only) or non-NULL exactly where agent
 * 1's are.  Both agents share the formats, num_actions, the pitches and the launch.  Outputs must not alias any input or
 * each other.
 *
 * LOGITS: n rows of num_actions elements, row-major, at logit_pitch ELEMENTS from row to row (what a Linear writes);
 * 2 <= num_actions <= 32, logit_pitch >= num_actions (19 with 18 actions: an actor-critic head that emits logits and
 * value from one Linear).  Columns num_actions .. pitch-1 are never interpreted.  A 16-bit element converts to float32
 * exactly.  ACTIONS: int32[n] or int64[n].
 */
#ifndef PIKAZOO_POLICY_H
#define PIKAZOO_POLICY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_POLICY_ABI_VERSION 1

int pz_policy_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_policy_build_id(void);

/* element type of the logit rows (the values of pz_gae_value_format, in its order) and of the action vectors */
enum pz_policy_logit_format { PZ_POLICY_LOGIT_FLOAT32 = 0, PZ_POLICY_LOGIT_FLOAT16 = 1, PZ_POLICY_LOGIT_BFLOAT16 = 2 };
enum pz_policy_action_format { PZ_POLICY_ACTION_INT32 = 0, PZ_POLICY_ACTION_INT64 = 1 };

/* ---- sample: action, log-probability and entropy of one or both agents in ONE launch ---------------------------------
 * logp_* and ent_* are float32[n]; either pair may be NULL.  An agent's action pointer may not be NULL.
 *
 * Per game g and agent s (0 or 1), with A = num_actions, in float32:
 *   1. l_i = float(logit_i), m = max_i l_i, e_i = exp(l_i - m).
 *   2. c_i = c_{i-1} + e_i in index order, as sequential float32 adds with c_{-1} = 0.  S = c_{A-1}.
 *   3. The uniform draw.  T = step + (step_dev ? *step_dev : 0) (uint64; step_dev is a const uint64_t* on the device: a
 *      by-value step is frozen into a captured graph, the caller increments the device counter inside the capture).
 *      T >= 2^62 is PZ_E_SIZE for the by-value part; the device part is not checked.  G = first_game + g is a GLOBAL
 *      game id: a rank's shard draws what the whole batch would draw.  The block is Philox4x32-10 with
 *      key = ((uint32)seed, (uint32)(seed >> 32)) -- the order of the env's key -- and
 *      counter = (G_lo, G_hi, T_lo, 2 + 4 * T_hi) (mod 2^32).  Word 3 = 2 mod 4 keeps this stream apart from the env
 *      stream (word 3 = 0) and from the on-device random policy (odd word 3): a caller who reuses the env's seed gets no
 *      correlated draws.  Output word s of that block gives u = float(w >> 8) * 2^-24, exact and in [0, 1).
 *   4. thr = u * S.  a = #{ i <= A-2 : c_i <= thr }, clamped to the last index with e_i > 0: a masked action (-inf
 *      logit) is never drawn, not even when thr rounds up to S.
 *   5. logp = (l_a - m) - log(S).  entropy = log(S) - (sum_i e_i * (l_i - m)) / S, the sum accumulated in index order
 *      with one fused multiply-add per term; a term with e_i == 0 contributes 0, not NaN.
 *   6. A row that holds a NaN, a +inf, or no finite logit yields action 0 and NaN for logp and entropy.  An action is
 *      never outside [0, A).
 * Nothing here is pinned bit for bit against a host restatement (contraction stays on); what IS pinned is that
 * pz_action_log_probs on the sampled actions returns pz_sample_actions' logp and entropy bit for bit, and that a shard
 * (rows [g0, n) with first_game + g0) returns the bits of the whole batch's tail.
 *
 * exp and log are OCML's expf and logf as hipcc links them by default (no fast-math, no native_ forms, float32
 * subnormals kept).  Accuracy assumed by the tests' tolerances: <= 3 ulp each, the bound the OpenCL C specification sets
 * for exp and log in full profile, which OCML is written to meet (its own table promises 1 ulp).  The ROCm installation
 * carries neither table as a document; the bound is quoted from the public specification (OpenCL C 3.0, section 7.4,
 * "Relative error as ULPs").
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    a required pointer is NULL, or agent 2's pointers are a mix of NULL and non-NULL;
 *   PZ_E_SIZE    n < 0, n > 2^30, num_actions outside [2, 32], logit_pitch < num_actions, n * logit_pitch * 4 bytes beyond
 *                int64, first_game < 0, step >= 2^62;
 *   PZ_E_CONFIG  an unknown format;
 *   PZ_E_ALIGN   a pointer not aligned to its element (logits 4 or 2 bytes, actions 4 or 8, floats 4, step_dev 8).
 * n == 0 returns PZ_OK without a launch. */
int pz_sample_actions(const void *logits_p1, const void *logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                      int64_t logit_pitch, uint64_t seed, int64_t first_game, uint64_t step, const uint64_t *step_dev,
                      int32_t action_format, void *act_p1, void *act_p2, float *logp_p1, float *logp_p2, float *ent_p1,
                      float *ent_p2, void *stream);

/* ---- log-probability and entropy of GIVEN actions ---------------------------------------------------------------------
 * Steps 1, 2, 5 and 6 above with a read from act_*.  An action outside [0, A) gives logp = NaN and a valid entropy.
 * The same checks as pz_sample_actions (without seed, first_game and the steps). */
int pz_action_log_probs(const void *logits_p1, const void *logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                        int64_t logit_pitch, int32_t action_format, const void *act_p1, const void *act_p2, float *logp_p1,
                        float *logp_p2, float *ent_p1, float *ent_p2, void *stream);

/* ---- its backward -----------------------------------------------------------------------------------------------------
 * glogp_* and gent_* are the float32[n] upstream gradients of logp and entropy; either pair may be NULL, which counts as
 * 0, but not both.  grad_*: n rows in the logits' own format (rounded to nearest even) at grad_pitch >= A elements;
 * columns A .. grad_pitch-1 are not written.  With p_i = e_i / S and H the entropy:
 *     grad_i = glogp * ([i == a] - p_i) + gent * (-p_i * ((l_i - m) - log(S) + H))
 * The second term is 0 where e_i == 0; [i == a] is 0 for an out-of-range action.  A row of step 6 yields NaN gradients.
 * The checks of pz_action_log_probs, with grad_pitch held to logit_pitch's rules and the gradients to the floats'. */
int pz_action_log_probs_backward(const void *logits_p1, const void *logits_p2, int32_t logit_format, int32_t num_actions,
                                 int64_t n, int64_t logit_pitch, int32_t action_format, const void *act_p1,
                                 const void *act_p2, const float *glogp_p1, const float *glogp_p2, const float *gent_p1,
                                 const float *gent_p2, void *grad_p1, void *grad_p2, int64_t grad_pitch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_POLICY_H */
