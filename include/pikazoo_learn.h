/* pikazoo_learn.h -- C ABI of libpikazoo_learn.so: what a trainer does FIRST with the trajectory tensors of a k-step launch.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, knows nothing of pz_config or the game state, and nothing in the step path
 * loads it.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a
 * positive value is the hipError_t of the launch).
 */
#ifndef PIKAZOO_LEARN_H
#define PIKAZOO_LEARN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_LEARN_ABI_VERSION 1

int pz_learn_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_learn_build_id(void);

/* element type of the reward rows (what the env produced) and of the value rows */
enum pz_gae_reward_format { PZ_GAE_REWARD_INT32 = 0, PZ_GAE_REWARD_FLOAT32 = 1 };
enum pz_gae_value_format { PZ_GAE_VALUE_FLOAT32 = 0, PZ_GAE_VALUE_FLOAT16 = 1, PZ_GAE_VALUE_BFLOAT16 = 2 };

/* ---- GAE(gamma, lambda): advantages and returns of one or both agents in ONE launch ----------------------------------
 * Inputs, rows of n games at a pitch in ELEMENTS (>= n): rewards [k] rows of `reward_format`, terminated [k] rows of
 * uint8 (shared by both agents), values [k + 1] rows of `value_format` -- row t is the value of the observation the
 * action of step t was chosen on, row k the bootstrap.  Outputs adv / ret: [k] float32 rows at out_pitch.
 *
 * Per game, for t = k-1 .. 0, in IEEE float32, round to nearest even, NO fused multiply-add, in exactly this order
 * (a_next starts at +0.0f, gl = gamma * lam is rounded once):
 *     nt    = (terminated[t] == 0)
 *     q     = nt ? gamma * float(v[t+1]) : +0.0f          -- a select: nothing crosses an episode end, a NaN neither
 *     delta = (float(r[t]) + q) - float(v[t])
 *     a     = delta + (nt ? gl * a_next : +0.0f)
 *     adv[t] = a;  ret[t] = a + float(v[t]);  a_next = a
 * (float() of an int32 reward rounds to nearest even beyond 2^24, of a 16-bit value it is exact.)  lam = 1 gives the
 * bootstrapped Monte-Carlo return, lam = 0 TD(0).  With frame skip the rewards are per policy step, and so is gamma.
 *
 * Agent 2's four pointers (rew_p2, val_p2, adv_p2, ret_p2) may ALL be NULL: one side only.  Both agents share the
 * formats, the pitches and the flags.  Outputs must not alias any input or each other; columns n .. pitch-1 of an
 * output row are not written.  One launch on `stream`, no allocation, no synchronisation: graph-capturable.
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    a NULL pointer other than all four of agent 2;
 *   PZ_E_SIZE    k < 1, n < 0, a pitch < n, or a tensor beyond the kernel's addressing: n > 2^30, or (k + 1) * pitch * 4
 *                bytes beyond int64 (it never wraps);
 *   PZ_E_CONFIG  an unknown format; gamma or lam not finite or outside [0, 1];
 *   PZ_E_ALIGN   a pointer not aligned to its element (4 bytes; 2 for 16-bit values; flags: any).
 * n == 0 returns PZ_OK without a launch. */
int pz_gae(const void *rew_p1, const void *rew_p2, int32_t reward_format, const uint8_t *terminated, const void *val_p1,
           const void *val_p2, int32_t value_format, int32_t k, int64_t n, int64_t rew_pitch, int64_t term_pitch,
           int64_t val_pitch, int64_t out_pitch, float gamma, float lam, float *adv_p1, float *adv_p2, float *ret_p1,
           float *ret_p2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_LEARN_H */
