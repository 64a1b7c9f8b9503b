/* pikazoo_act.h -- C ABI of libpikazoo_act.so: a rollout step's policy side in ONE launch, from the observation rows that the
 * step writes to (action, log-probability, entropy, value) -- the forward pass of the three-layer policy net
 * (pikazoo_net.h) and the categorical head over its logits (pikazoo_policy.h) without the [n, out_features] head's round
 * trip through memory and without a second launch.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path, pikazoo_amd.net, pikazoo_amd.policy or any other
 * binding loads it before pikazoo_amd.act is used.  Return codes are pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2,
 * PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of the launch).
 *
 * THE DEFINITION, by reference.  With O = out_features and A = num_actions, per game g of an agent:
 *   - the head row is pz_mlp_forward's float32 row (out_format = PZ_NET_OUT_FLOAT32) of observation row g under the same
 *     parameters, activation and observation format, BIT FOR BIT (pikazoo_net.h: THE DEFINITION, ARITHMETIC);
 *   - the logits are its columns 0 .. A-1, and steps 1-6 of pz_sample_actions (pikazoo_policy.h) run on them as float32
 *     logits: the same key ((uint32)seed, (uint32)(seed >> 32)), the same counter layout, the GLOBAL game id
 *     G = first_game + g, T = step + (step_dev ? *step_dev : 0), output word s of the block for agent s (0: *_p1, 1: *_p2);
 *   - val[g] = column A of the head row.
 * What is pinned: act, logp, ent, val and head of this launch hold exactly the bits that pz_mlp_forward (float32 output at
 * any pitch) followed by pz_sample_actions (float32 logits at that pitch) return on the same inputs.  The staging, the dense
 * layer, the row statistics and the Philox draw are one text for both routes (csrc/pz_mlp_tile.hpp,
 * csrc/pz_policy_rows.hpp); the three layers' driver, the counting of step 4 and the log-prob of step 5 are repeated beside
 * the older kernels' own lines, expression for expression (DESIGN.md 4.23 says why), and tests/test_gpu_act.py holds the two
 * routes to each other.  So a trainer may switch between the two routes in the middle of a run, a shard (rows [g0, n) with
 * first_game + g0) returns the bits of the whole batch's tail, and a row's bits do not depend on the batch around it.
 * What is NOT pinned: nothing is held bit for bit against a host restatement (as in the two older headers).
 *
 * Pointers are caller-owned device memory; one launch on `stream`, no allocation, no synchronisation: graph-capturable.
 * n == 0 returns PZ_OK without a launch.
 *
 * OBSERVATIONS and PARAMETERS: as pz_mlp_forward's.  obs_format is a pz_net_obs_format, activation a pz_net_activation,
 * action_format a pz_policy_action_format, by value.
 * SIZES: the net's box (1 <= in_features <= 72, hidden in {32, 64, 128}, 0 <= n <= 2^30, obs_pitch >= in_features) with
 * 2 <= num_actions <= 32 and num_actions <= out_features <= 40.  (LDS: the staged parameters plus the four waves' logit
 * images of 32 x (out_features | 1) floats each.  At the largest, (72, 128, 40): 136 448 + 20 992 = 157 440 B of the
 * 163 840 B; at (35, 64, 19): 35 456 + 9 728 = 45 184 B, which leaves room for two workgroups per compute unit.)
 * OUTPUTS:
 *   act_*   int32[n] or int64[n]; required.
 *   logp_*, ent_*  float32[n]; either pair may be NULL, as in pz_sample_actions.
 *   val_*   float32[n]; may be NULL.  When given, out_features > num_actions is required (PZ_E_SIZE otherwise).
 *   head_*  float32 rows of out_features elements at head_pitch >= out_features ELEMENTS; may be NULL.  When given, the
 *           launch also stores what pz_mlp_forward would (columns out_features .. head_pitch-1 are not written); every
 *           other output holds the same bits as with head_* = NULL.  head_pitch is checked only when head_p1 is given.
 * AGENT 2 is all-or-none per pointer group: obs_p2 and the six parameters of agent 2 are ALL NULL (one side only) or ALL
 * non-NULL, and each of act_p2, logp_p2, ent_p2, val_p2, head_p2 is non-NULL exactly where agent 1's is, if agent 2 is
 * there at all.  Shared weights: agent 2's parameter pointers equal agent 1's.  Inputs may alias each other; an output must
 * not alias an input or another output.
 *
 * Checked before the launch, in this order (each the union of pz_mlp_forward's and pz_sample_actions' list):
 *   PZ_E_NULL    obs, a parameter or act of agent 1 is NULL; agent 2's obs and parameters are a mix of NULL and non-NULL;
 *                an output of agent 2 is there where agent 1's is not, or missing where agent 1's is;
 *   PZ_E_SIZE    n < 0, n > 2^30, in_features outside [1, 72], hidden not 32 / 64 / 128, num_actions outside [2, 32],
 *                out_features outside [num_actions, 40], val given with out_features == num_actions, obs_pitch <
 *                in_features, head given with head_pitch < out_features, n * pitch * 4 bytes beyond int64, first_game < 0,
 *                step >= 2^62;
 *   PZ_E_CONFIG  an unknown observation format, activation or action format;
 *   PZ_E_ALIGN   a pointer not aligned to its element (observations 4 or 2 bytes, parameters 4, actions 4 or 8 -- int64
 *                actions are held to 8 --, floats 4, head 4, step_dev 8).
 */
#ifndef PIKAZOO_ACT_H
#define PIKAZOO_ACT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_ACT_ABI_VERSION 1
#define PZ_ACT_MAX_ACTIONS 32

int pz_act_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_act_build_id(void);

int pz_mlp_act(const void *obs_p1, const void *obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch,
               int32_t hidden, int32_t out_features, int32_t activation, const float *w1_p1, const float *b1_p1,
               const float *w2_p1, const float *b2_p1, const float *w3_p1, const float *b3_p1, const float *w1_p2,
               const float *b1_p2, const float *w2_p2, const float *b2_p2, const float *w3_p2, const float *b3_p2,
               int32_t num_actions, uint64_t seed, int64_t first_game, uint64_t step, const uint64_t *step_dev,
               int32_t action_format, void *act_p1, void *act_p2, float *logp_p1, float *logp_p2, float *ent_p1,
               float *ent_p2, float *val_p1, float *val_p2, float *head_p1, float *head_p2, int64_t head_pitch,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_ACT_H */
