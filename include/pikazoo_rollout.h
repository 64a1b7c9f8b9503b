/* pikazoo_rollout.h -- C ABI of libpikazoo_rollout.so: k POLICY STEPS in ONE launch -- the policy net's forward, the
 * categorical draw and the game's frame, k times over, with the state in registers and the observation rows handed from the
 * frame to the net through LDS.  What it writes is the rollout buffer a learner reads: observations, actions, log-probs,
 * values (with the bootstrap row), rewards and termination flags.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id); nothing loads
 * it before pikazoo_amd.rollout is used.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2,
 * PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of the launch).
 *
 * THE DEFINITION, by reference to the launches it replaces.  With A = the env's action count (18, or 13 with
 * cfg->simplify_action), O = out_features = A + 1, in_features = 35, both agents driven by the net, for t = 0 .. k-1:
 *   1. obs_*[t]  = the observation rows of the state as pz_step / pz_reset would have written them in cfg->normalize_obs
 *                  (0: int32 rows, 1: float32 normalised rows);
 *   2. (act, logp, ent, val)_*[t] = pz_mlp_act (pikazoo_act.h) on those rows with the same parameters, activation, seed,
 *                  first_game and action_format, at step T = step + (step_dev ? *step_dev : 0) + t, BIT FOR BIT -- and so
 *                  pz_mlp_forward's head followed by pz_sample_actions;
 *   3. one frame exactly as pz_step runs it on the two sampled actions: cfg->auto_reset as configured (a game that ended is
 *                  reset in place by the head of the next step's frame, inside the launch), the fused reward wrappers, the
 *                  episode statistics, *episodes_done;
 *   4. rew_*[t], terminated[t] = that frame's rewards (float32 when cfg->ballpos_reward or cfg->normal_state_mode, else
 *                  int32) and its game_ended byte.
 * Then obs_*[k] = the rows of the final state, and val_*[k] = column A of the head on them (the bootstrap value): no draw
 * is made for it and no step is consumed.  The state is read once and written once.
 * The three layers are csrc/pz_mlp_tile.hpp's tile_layers, the head's row code csrc/pz_policy_rows.hpp's, the frame
 * csrc/pz_physics.hpp's frame_head / frame_tail: one text for this launch and the ones it replaces, and
 * tests/test_gpu_policy_rollout.py holds the two routes to each other.
 *
 * LAYOUT.  Slab t of every per-game output starts t * pitch games behind slab 0 (pitch >= n, in GAMES): act_* int32 or
 * int64 [k][pitch], logp_*, ent_* float32 [k][pitch], val_* float32 [k + 1][pitch], rew_* 4-byte [k][pitch], terminated
 * uint8 [k][pitch], obs_* 4-byte [k + 1][pitch][35].  Elements of games n .. pitch-1 are not written.  ent_* may be NULL
 * (both).  PARAMETERS: as pz_mlp_forward's for in_features 35; agent 2's six are ALL NULL (shared weights: both agents on
 * agent 1's) or ALL given (a set of its own, staged beside agent 1's).
 * GEOMETRY AND LDS.  One workgroup of four waves per 64 games: wave 0 runs the frame, one lane per game; each of the four
 * takes one 32-row tile of the net (agent x half) per step.  The LDS holds the staged parameter set(s), both agents' 64
 * rows, four logit images and the action exchange: 4 * (sets * lds_floats(35, hidden, O) + 4480 + 128 * (O | 1) + 128)
 * bytes.  At O = 19, hidden = 128 with two parameter sets is 235 264 B against 163 840 B and is REFUSED with PZ_E_SIZE;
 * every other combination fits (hidden 128 shared: 131 712 B; hidden 64 separate: 99 072 B; hidden 64 shared: 63 616 B).
 *
 * OUT OF SCOPE, refused with PZ_E_CONFIG: computer players (cfg->p1_computer / p2_computer), the packed state, the 2-byte
 * row formats (cfg->normalize_obs >= 2).
 *
 * Pointers are caller-owned device memory; one launch on `stream`, no allocation, no synchronisation: graph-capturable (a
 * caller with a device step counter adds k to *step_dev between replays).  Checked before the launch, in this order:
 *   PZ_E_NULL    state, cfg, a parameter of agent 1, obs_*, act_*, logp_*, val_*, rew_* or terminated is NULL; agent 2's
 *                six parameters are a mix of NULL and non-NULL; exactly one of ent_p1 / ent_p2 is NULL;
 *   PZ_E_SIZE    n < 0, stride < n, stride beyond one launch's games (2^32 / 176), k outside [1, 2^20], hidden not
 *                32 / 64 / 128, out_features != A + 1, pitch < n or beyond one launch's games, first_game < 0,
 *                step + k > 2^62;
 *   PZ_E_CONFIG  a configuration value outside its enum, anything OUT OF SCOPE above, an unknown activation or action
 *                format;
 *   PZ_E_ALIGN   a pointer not aligned to its element (state, observations, rewards, parameters, floats 4; actions 4 or
 *                8; episode_stats, episodes_done, step_dev 8);
 *   PZ_E_SIZE    the LDS refusal above;
 * and n == 0 then returns PZ_OK without a launch.
 */
#ifndef PIKAZOO_ROLLOUT_H
#define PIKAZOO_ROLLOUT_H
#include <stdint.h>

#include "pikazoo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_ROLLOUT_ABI_VERSION 1
#define PZ_ROLLOUT_MAX_STEPS (1 << 20)

int pz_rollout_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_rollout_build_id(void);

int pz_rollout_policy(int32_t *state, int64_t n, int64_t stride, const pz_config *cfg, int32_t k, int32_t hidden,
                      int32_t out_features, int32_t activation, const float *w1_p1, const float *b1_p1, const float *w2_p1,
                      const float *b2_p1, const float *w3_p1, const float *b3_p1, const float *w1_p2, const float *b1_p2,
                      const float *w2_p2, const float *b2_p2, const float *w3_p2, const float *b3_p2, uint64_t seed,
                      int64_t first_game, uint64_t step, const uint64_t *step_dev, int32_t action_format, int64_t pitch,
                      void *obs_p1, void *obs_p2, void *act_p1, void *act_p2, float *logp_p1, float *logp_p2, float *val_p1,
                      float *val_p2, float *ent_p1, float *ent_p2, void *rew_p1, void *rew_p2, uint8_t *terminated,
                      void *episode_stats, unsigned long long *episodes_done, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_ROLLOUT_H */
