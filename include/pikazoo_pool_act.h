/* pikazoo_pool_act.h -- C ABI of libpikazoo_pool_act.so: a league rollout step's policy side in ONE launch, from the observation
 * rows that the step writes to (action, log-probability, entropy, value), every row through the parameter set of its own pool
 * member -- pz_mlp_forward_pool (pikazoo_pool.h) and the categorical head over its logits (pikazoo_policy.h) without the
 * [n, out_features] head's round trip through memory and without a second launch.  It is to pz_mlp_forward_pool what pz_mlp_act
 * (pikazoo_act.h) is to pz_mlp_forward.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path, pikazoo_amd.pool, pikazoo_amd.league, pikazoo_amd.act,
 * pikazoo_amd.net or any other binding loads it before pikazoo_amd.pool_act is used.  Return codes are pikazoo_hip.h's (PZ_OK 0,
 * PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of the launch).
 *
 * THE DEFINITION, by reference (as in pikazoo_act.h).  With O = out_features, A = num_actions and P = num_members, take row g
 * of an agent whose member m = members[g] is in [0, P) (an agent without a plan: m = 0 for every row):
 *   - the head row is pz_mlp_forward_pool's float32 row of observation row g, BIT FOR BIT: that is pz_mlp_forward's row under
 *     member m's parameters (pikazoo_pool.h: THE DEFINITION; pikazoo_net.h: ARITHMETIC);
 *   - act, logp and ent are steps 1-6 of pz_sample_actions (pikazoo_policy.h) on columns 0 .. A-1 of that head row as float32
 *     logits: the same key ((uint32)seed, (uint32)(seed >> 32)), the same counter layout, the GLOBAL game id
 *     G = first_game + g -- the ROW's index, whatever slot of the plan holds it --, T = step + (step_dev ? *step_dev : 0),
 *     output word s of the Philox block for agent s (0: *_p1, 1: *_p2), as in pikazoo_act.h;
 *   - val[g] = column A of the head row.
 * A row whose member is outside [0, P) is in no group of the plan: nothing of it is read and NONE of its outputs is written.
 * What is pinned: act, logp, ent, val and head of this launch hold exactly the bits that pz_mlp_forward_pool (float32 output
 * at any pitch) followed by pz_sample_actions (float32 logits at that pitch) return on the same inputs; with P = 1 and no
 * plans they are pz_mlp_act's.  The staging, the three layers, the row statistics, the Philox draw, the counting of step 4 and
 * the log-prob of step 5 are the texts pz_mlp_act runs (csrc/pz_mlp_tile.hpp, csrc/pz_policy_rows.hpp); the group walk is
 * pz_mlp_forward_pool's, repeated beside it, and tests/test_gpu_pool_act.py holds the routes to each other.
 * So a trainer may switch between the routes in the middle of a run, a shard (rows [g0, n) with first_game + g0 and a plan
 * over those rows) returns the bits of the whole batch's tail, and a row's bits depend neither on the batch nor on the plan
 * around it.  What is NOT pinned: nothing is held bit for bit against a host restatement (as in the older headers).
 *
 * Pointers are caller-owned device memory, `members` a HOST array read at call time (pikazoo_pool.h: PARAMETERS); one launch
 * on `stream`, no allocation, no synchronisation: graph-capturable.  n == 0 returns PZ_OK without a launch.
 *
 * OBSERVATIONS, PARAMETERS and PLANS: as pz_mlp_forward_pool's (a plan is read from device memory when the launch runs;
 * whatever it holds, no memory outside the tensors is touched).  obs_format is a pz_net_obs_format, activation a
 * pz_net_activation, action_format a pz_policy_action_format, by value.
 * SIZES: the net's box (1 <= in_features <= 72, hidden in {32, 64, 128}, 0 <= n <= 2^30, obs_pitch >= in_features) with
 * 1 <= num_members <= 16, 2 <= num_actions <= 32 and num_actions <= out_features <= 40.  (LDS: the staged parameters, the 32
 * words that hold `first`, and the four waves' logit images of 32 x (out_features | 1) floats each.  At the largest,
 * (72, 128, 40): 136 448 + 128 + 20 992 = 157 568 B of the 163 840 B; at (35, 64, 19): 35 456 + 128 + 9 728 = 45 312 B, which
 * leaves room for two workgroups per compute unit.)
 * OUTPUTS -- the rules differ from pz_mlp_act's: agent 2's optional outputs do NOT follow agent 1's.
 *   act_*   int32[n] or int64[n]; REQUIRED for every agent that is present (agent 2 is present when obs_p2 is given).
 *   logp_*, ent_*, val_*  float32[n]; each may be NULL, per agent, on its own.  A league passes them for the learner's side
 *           only.  An agent with none of the three skips the log-prob and the stored statistics in the kernel; its action is
 *           the same bit.  val given (for either agent) with out_features == num_actions is PZ_E_SIZE.
 *   head_*  float32 rows of out_features elements at head_pitch >= out_features ELEMENTS; each may be NULL on its own.  Where
 *           given, the launch also stores what pz_mlp_forward_pool would (columns out_features .. head_pitch-1 are not
 *           written); every other output holds the same bits as with head_* = NULL.  head_pitch is checked only when a head
 *           is given.
 * AGENT 2 is there when obs_p2 is: act_p2 is then required, and without obs_p2 every pointer of agent 2 must be NULL.  Inputs
 * may alias each other; an output must not alias an input or another output.
 *
 * Checked before the launch, in this order (the union of pz_mlp_forward_pool's and pz_mlp_act's lists):
 *   PZ_E_NULL    obs or act of agent 1, or members, is NULL; agent 2's obs and act are a mix of NULL and non-NULL; agent 2 is
 *                absent and has an order, a first or an output;
 *   PZ_E_SIZE    num_members outside [1, 16];
 *   PZ_E_NULL    one of the 6 P member pointers is NULL; an agent's first is NULL while its order is not;
 *   PZ_E_SIZE    n < 0, n > 2^30, in_features outside [1, 72], hidden not 32 / 64 / 128, num_actions outside [2, 32],
 *                out_features outside [num_actions, 40], a val given with out_features == num_actions, obs_pitch <
 *                in_features, a head given with head_pitch < out_features, n * pitch * 4 bytes beyond int64, first_game < 0,
 *                step >= 2^62;
 *   PZ_E_CONFIG  an unknown observation format, activation or action format;
 *   PZ_E_ALIGN   a pointer not aligned to its element (observations 4 or 2 bytes, parameters 4, actions 4 or 8 -- int64
 *                actions are held to 8 --, order and first 4, floats 4, head 4, step_dev 8).
 */
#ifndef PIKAZOO_POOL_ACT_H
#define PIKAZOO_POOL_ACT_H
#include <stdint.h>

#include "pikazoo_pool.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_POOL_ACT_ABI_VERSION 1
#define PZ_POOL_ACT_MAX_ACTIONS 32

int pz_pool_act_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_pool_act_build_id(void);

int pz_mlp_act_pool(const void *obs_p1, const void *obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch,
                    int32_t hidden, int32_t out_features, int32_t activation, const pz_pool_member *members, int32_t num_members,
                    const int32_t *order_p1, const int32_t *first_p1, const int32_t *order_p2, const int32_t *first_p2,
                    int32_t num_actions, uint64_t seed, int64_t first_game, uint64_t step, const uint64_t *step_dev,
                    int32_t action_format, void *act_p1, void *act_p2, float *logp_p1, float *logp_p2, float *ent_p1,
                    float *ent_p2, float *val_p1, float *val_p2, float *head_p1, float *head_p2, int64_t head_pitch,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_POOL_ACT_H */
