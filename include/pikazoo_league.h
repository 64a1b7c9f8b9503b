/* pikazoo_league.h -- C ABI of libpikazoo_league.so: what turns a pool of frozen snapshots into a LEAGUE -- the results of the
 * games that ended on a step, accumulated per pair of members in a table on the device (pz_league_tally), and a member per
 * game drawn with integer weights from a counter (pz_league_draw), each in ONE launch.  There is no boolean indexing, no
 * multinomial, no index tensor, no allocation and no synchronisation.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path or in the other libraries loads it.  Return codes are
 * pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of
 * the launch).  Every call is one launch on `stream`, allocates nothing, does not synchronise and is graph-capturable.
 * Outputs must not alias inputs or each other (not checked here).  There is no floating point anywhere: both definitions are
 * in integers, so every result is fixed bit for bit.
 *
 * ---- THE TALLY (pz_league_tally) -------------------------------------------------------------------------------------------------
 *     terminated  [n] uint8: the step's terminations.
 *     score_p1, score_p2   the two scores of game g are score_pX[g * score_stride], ELEMENTS of score_format (int32 or int16,
 *                 read signed).  The int32 state holds them as two rows at stride 1, the packed state as int16 at stride 8.
 *     members_p1, members_p2   [n] of member_format, whose VALUES are pz_pool_member_format's (pikazoo_pool.h: uint8 0, int32 1,
 *                 int64 2).  members_p1 may be NULL: player_1 is member 0 in every game.
 *     P = num_members, 1 <= P <= PZ_LEAGUE_MAX_MEMBERS = 16;  0 <= n <= 2^30.
 *     table       [P][P][PZ_LEAGUE_CELL_WORDS = 4] int64, ACCUMULATED;  errors  [1] int64, ACCUMULATED.
 * For every game g with terminated[g] != 0:  a = members_p1 ? members_p1[g] : 0,  b = members_p2[g],  s1 = score_p1[g *
 * score_stride],  s2 = score_p2[g * score_stride].  If 0 <= a < P and 0 <= b < P:
 *     table[a][b][0] += 1            (games)
 *     table[a][b][1] += (s1 > s2)    (won by player_1)
 *     table[a][b][2] += s1
 *     table[a][b][3] += s2
 * otherwise *errors += 1 and the table is untouched by that game.  A game with terminated[g] == 0 contributes nothing; its
 * members are not read and its scores may hold anything.  The sums are 64-bit integers (two's complement), so the order of
 * accumulation does not show in the result.  n == 0 returns PZ_OK without a launch.
 *
 * ---- THE DRAW (pz_league_draw), in integers -------------------------------------------------------------------------------------
 *     weights     device int64[P]; a weight is VALID iff 0 <= w < 2^32.
 *     W = sum_p weights[p],  cum[p] = weights[0] + .. + weights[p]:  uint64, below 2^36.
 *     C = counter + (counter_dev ? *counter_dev : 0), in uint64.  The by-value part is frozen into a captured graph; the caller
 *         increments the device word inside the capture.  counter < 2^62.
 *     If a weight is invalid or W == 0:  *errors = 1 (an ordinary vector store; the word is never cleared here) and NO member
 *     is written.  Otherwise, for every game g < n with mask == NULL or mask[g] != 0:
 *         G = (uint64) (first_game + g): the game's global id, so that a shard [g0, g0 + n) called with first_game + g0 draws
 *             what the whole batch draws for those games
 *         (word0, word1, ., .) = the Philox4x32-10 block (Salmon et al., SC'11) with
 *             key      ((uint32) seed ^ 0x4C454147, (uint32) (seed >> 32) ^ 0x44524157)
 *             counter  ((uint32) G, (uint32) (G >> 32), (uint32) C, (uint32) (C >> 32))
 *           (the key is XORed because four streams already live under a caller's plain seed -- the env, the policy head and
 *           the random policy, which occupy every residue of counter word 3, and the batch permutation under its own XOR
 *           (pikazoo_batch.h): a caller who reuses one seed for all of them gets no correlated stream)
 *         u = (word1 << 32) | word0,   r = floor(u * W / 2^64)        (the high 64 bits of the 128-bit product; r < W)
 *         members[g] = #{ p < P : cum[p] <= r }                       (the smallest p with cum[p] > r)
 *     A member of weight 0 is never drawn (cum[p] == cum[p - 1] cannot be the first to exceed r), and since r < W = cum[P - 1]
 *     the result is always below P.  Games with mask[g] == 0 are not written.  n == 0 returns PZ_OK without a launch (the
 *     weights are then not looked at).
 *
 * Checked before the launch, in this order (both calls):
 *   PZ_E_NULL    terminated, score_p1, score_p2 or members_p2 NULL with n > 0, table or errors NULL (pz_league_tally);
 *                weights or errors NULL, members NULL with n > 0 (pz_league_draw);
 *   PZ_E_SIZE    n outside [0, 2^30]; num_members outside [1, 16]; score_stride < 1, or n * score_stride elements beyond
 *                int64 bytes (pz_league_tally); counter >= 2^62 (pz_league_draw);
 *   PZ_E_CONFIG  an unknown score_format or member_format;
 *   PZ_E_ALIGN   table, the tally's errors, weights or counter_dev not 8-byte aligned; the draw's errors not 4-byte aligned;
 *                a score or member pointer not aligned to its element.
 */
#ifndef PIKAZOO_LEAGUE_H
#define PIKAZOO_LEAGUE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_LEAGUE_ABI_VERSION 1
#define PZ_LEAGUE_MAX_MEMBERS 16
#define PZ_LEAGUE_CELL_WORDS 4

/* element type of the score vectors */
enum pz_league_score_format { PZ_LEAGUE_SCORE_INT32 = 0, PZ_LEAGUE_SCORE_INT16 = 1 };

int pz_league_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_league_build_id(void);

int pz_league_tally(const uint8_t *terminated, const void *score_p1, const void *score_p2, int32_t score_format, int64_t score_stride, const void *members_p1, const void *members_p2, int32_t member_format, int64_t n, int32_t num_members, int64_t *table, int64_t *errors, void *stream);

int pz_league_draw(const int64_t *weights, int32_t num_members, uint64_t seed, uint64_t counter, const uint64_t *counter_dev, int64_t first_game, const uint8_t *mask, void *members, int32_t member_format, int64_t n, int32_t *errors, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_LEAGUE_H */
