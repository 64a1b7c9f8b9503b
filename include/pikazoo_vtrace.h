/* pikazoo_vtrace.h -- C ABI of libpikazoo_vtrace.so: V-trace targets (Espeholt et al., IMPALA, 2018) over the trajectory
 * tensors of a k-step launch -- the off-policy generalisation of pz_gae (pikazoo_learn.h) for samples whose behaviour policy is
 * no longer the current one: a second epoch over one rollout, samples kept across a snapshot, an actor / learner split.
 *
 * A library of its own beside the others (built by pika-zoo_amd/build.py, same flags, same build id): it reads and writes
 * caller-owned device tensors only, and nothing in the step path or in any older binding loads it.  Return codes are
 * pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t
 * of the launch).
 */
#ifndef PIKAZOO_VTRACE_H
#define PIKAZOO_VTRACE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_VTRACE_ABI_VERSION 1

int pz_vtrace_abi_version(void);
/* source digest this library was compiled from: equals the build id of the product library built beside it */
const char *pz_vtrace_build_id(void);

/* element type of the reward rows and of the value rows (the values of pikazoo_learn.h's two enums) */
enum pz_vtrace_reward_format { PZ_VTRACE_REWARD_INT32 = 0, PZ_VTRACE_REWARD_FLOAT32 = 1 };
enum pz_vtrace_value_format { PZ_VTRACE_VALUE_FLOAT32 = 0, PZ_VTRACE_VALUE_FLOAT16 = 1, PZ_VTRACE_VALUE_BFLOAT16 = 2 };

/* ---- V-trace: value targets and policy-gradient advantages of one or both agents in ONE launch ------------------------
 * Inputs, rows of n games at a pitch in ELEMENTS (>= n): rewards r [k] rows of `reward_format`; terminated [k] rows of
 * uint8 (shared by both agents); values v [k + 1] rows of `value_format` -- the values of the CURRENT parameters, row t of
 * the observation the action of step t was chosen on, row k the bootstrap; behaviour log-probs lpb [k] float32 rows (what
 * the policy that ACTED assigned to the action: what pz_sample_actions / pz_mlp_act stored); target log-probs lpt [k]
 * float32 rows (what the CURRENT parameters assign to the same action: pz_action_log_probs).  The four log-prob tensors
 * share lp_pitch.  Outputs vs / pg_adv: [k] float32 rows at out_pitch.
 *
 * Per game, for t = k-1 .. 0, in IEEE float32, round to nearest even, NO fused multiply-add, in exactly this order
 * (gl = gamma * lam is rounded once; acc_next starts at +0.0f; v_next starts at float(v[k])):
 *     nt    = (terminated[t] == 0)
 *     d     = lpt[t] - lpb[t]
 *     w     = (d == 0) ? 1.0f : expf(d)            -- the ONE operation not pinned to the bit: the device's expf
 *     rho   = (w > clip_rho)    ? clip_rho    : w  -- a select written this way: a NaN weight stays NaN, +inf becomes the clip
 *     c     = (w > clip_c)      ? clip_c      : w
 *     pg    = (w > clip_pg_rho) ? clip_pg_rho : w
 *     q     = nt ? gamma * v_next : +0.0f          -- a select: nothing crosses an episode end, a NaN neither
 *     delta = (float(r[t]) + q) - float(v[t])
 *     acc   = rho * delta + (nt ? (gl * c) * acc_next : +0.0f)
 *     vs[t]     = float(v[t]) + acc
 *     pg_adv[t] = pg * (delta + (nt ? gl * acc_next : +0.0f))
 *     acc_next = acc;  v_next = float(v[t])
 * (float() of an int32 reward rounds to nearest even beyond 2^24, of a 16-bit value it is exact.)
 *
 * What it is: vs is IMPALA's v-trace target with the lambda-weighted trace c_t = lam * min(clip_c, w_t) and
 * rho_t = min(clip_rho, w_t); pg_adv is min(clip_pg_rho, w_t) * (r_t + gamma * (lam * vs[t+1] + (1 - lam) * v[t+1]) - v[t]),
 * the paper's rho * (r + gamma * vs' - v) at lam = 1 and the usual lambda-mix below it (vs' - v' = acc_next).
 *
 * THE CONSEQUENCE: where lpt and lpb hold the same bits (d == 0, so w = 1 without an expf) and all three clips are >= 1,
 * rho = c = pg = 1, every product with them is exact, and the recurrence IS pz_gae's: vs equals its ret and pg_adv its adv,
 * BIT FOR BIT (tests/test_vtrace_host.py holds the definition to it, tests/test_gpu_vtrace.py the kernel on the device).
 * A weight of 0 (lpt = -inf) and a weight beyond its clip (the clip itself) are exact too; every other weight carries
 * expf's error, which the tests bound.
 *
 * Agent 2's six pointers (rew_p2, val_p2, lpb_p2, lpt_p2, vs_p2, pg_p2) may ALL be NULL: one side only.  Both agents share
 * the formats, the pitches, the flags and the five scalars.  Outputs must not alias any input or each other; columns
 * n .. pitch-1 of an output row are not written.  One launch on `stream`, no allocation, no synchronisation:
 * graph-capturable.
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    a NULL pointer other than all six of agent 2;
 *   PZ_E_SIZE    k < 1, n < 0, a pitch < n, or a tensor beyond the kernel's addressing: n > 2^30, or (k + 1) * pitch * 4
 *                bytes beyond int64 (it never wraps);
 *   PZ_E_CONFIG  an unknown format; gamma or lam not finite or outside [0, 1]; a clip not finite or < 0;
 *   PZ_E_ALIGN   a pointer not aligned to its element (4 bytes; 2 for 16-bit values; flags: any).
 * n == 0 returns PZ_OK without a launch. */
int pz_vtrace(const void *rew_p1, const void *rew_p2, int32_t reward_format, const uint8_t *terminated, const void *val_p1,
              const void *val_p2, int32_t value_format, const float *lpb_p1, const float *lpb_p2, const float *lpt_p1,
              const float *lpt_p2, int32_t k, int64_t n, int64_t rew_pitch, int64_t term_pitch, int64_t val_pitch,
              int64_t lp_pitch, int64_t out_pitch, float gamma, float lam, float clip_rho, float clip_c, float clip_pg_rho,
              float *vs_p1, float *vs_p2, float *pg_p1, float *pg_p2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_VTRACE_H */
