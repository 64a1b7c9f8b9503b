/* pikazoo_pool.h -- C ABI of libpikazoo_pool.so: the forward pass of the policy net for a POOL of parameter sets, every
 * batch row through the set of its own pool member, in ONE launch (pz_mlp_forward_pool), and the plan that groups the rows
 * by member for it (pz_pool_plan).  This is what self-play against a pool of frozen snapshots needs per policy step: each
 * game draws its own opponent, and the net launch serves them all.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path or in the other libraries loads it.  Return codes are
 * pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of
 * the launch).  Every call is one launch on `stream`, allocates nothing, does not synchronise and is graph-capturable.
 *
 * ---- THE PLAN (pz_pool_plan), in integers ------------------------------------------------------------------------------------
 * The forward works on tiles of 32 rows that share one staged parameter set, so rows are grouped by member first.
 *     G = PZ_POOL_GROUP_ROWS = 128: one tile for each of the four waves of a workgroup, which therefore always share a member.
 *     members   [n] of member_format (uint8, int32 or int64), P = num_members, 1 <= P <= PZ_POOL_MAX_MEMBERS = 16,
 *               0 <= n <= 2^30.  Row i is VALID if 0 <= members[i] < P.
 *     count[p]  the number of valid rows of member p;   padded[p] = ceil(count[p] / G) * G
 *     first     [P + 1] int32:  first[0] = 0,  first[p + 1] = first[p] + padded[p]
 *     order     [capacity(n, P)] int32:
 *               order[first[p] + j] = the j-th smallest valid row index with member p, for j < count[p]   (stable)
 *               order[first[p] + j] = -1                                               for count[p] <= j < padded[p]
 *               order[j] = -1                                                          for first[P] <= j < capacity(n, P)
 *     errors    [1] int32: the number of rows that are not valid.  They are in no group: the forward neither reads nor
 *               writes them.  The word is SET by every plan (an ordinary vector store), not accumulated.
 *     capacity(n, P) = (n / G + P) * G   (integer division; pz_pool_capacity returns it, or -1 for n or P out of range).
 * THE BOUND first[P] <= capacity(n, P).  Write count[p] = q_p G + r_p with 0 <= r_p < G.  Then padded[p] = (q_p + [r_p > 0]) G,
 * sum_p q_p <= floor(sum_p count[p] / G) <= n / G, and sum_p [r_p > 0] <= P, so first[P] = sum_p padded[p] <= (n / G + P) G.
 * It is met with equality when every row is valid, every r_p > 0 and sum_p r_p < G: for instance every count = 1 mod G.
 * The plan is ONE launch of one workgroup: a stable counting sort in which each of 16 waves owns a contiguous run of rows,
 * counts them per member with wave ballots, one scan in LDS orders the (member, wave) counts member-major, and a second walk
 * writes each row at its member's next position.  No floating point, no atomics, no workspace.  It is meant to run once per
 * re-assignment of opponents, not per policy step.  n == 0 still launches (order is all -1, first all 0, errors 0).
 *
 * ---- THE FORWARD (pz_mlp_forward_pool) -----------------------------------------------------------------------------------------
 * Sizes, formats, pitches, activations and alignment rules are pz_mlp_forward's (pikazoo_net.h), and so is the arithmetic.
 * What differs:
 *   PARAMETERS come as a HOST array of P pz_pool_member structs of six device pointers each: torch's own nn.Linear tensors of
 *     every member, read in place by every launch.  The array is read at call time and travels in the kernel arguments (16 x 6
 *     pointers = 768 bytes), so a captured graph holds the pointers by value; there is no table in device memory, and nothing
 *     is repacked or cached between launches: a change of a member's parameters between two launches, or between two replays
 *     of a captured graph, is seen by the next one.  Two members may point at the same tensors.  Both agents share the array.
 *   PLANS: each agent passes the `order` and `first` of a pz_pool_plan over ITS rows with the same n and P.  An agent whose
 *     order is NULL runs every row on member 0 (the learner's side needs no plan).  Agent 2's obs and out are both NULL (one
 *     side only; its order and first must then be NULL too) or both non-NULL.
 *   A plan is read from device memory when the launch runs.  Whatever it holds, no memory outside the tensors is touched: a
 *     row index outside [0, n) is treated like -1, a first[p] is clamped to [0, capacity(n, P)].  A plan that is not a
 *     pz_pool_plan of the same n and P gives unspecified rows, not a fault.
 * THE DEFINITION.  For every valid row i of an agent, out[i] holds exactly the bits that pz_mlp_forward of the same build
 * writes for row i with the parameters of member members[i] (an unplanned agent: member 0).  pikazoo_net.h promises that a
 * row's bits do not depend on the batch, the position or the other agent, so this is well defined; both launches run the
 * tile code of csrc/pz_mlp_tile.hpp.  Rows of invalid members, and the columns
 * out_features .. out_pitch-1, are not written.
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    obs, out or members of agent 1 is NULL; agent 2's obs and out are a mix of NULL and non-NULL, or it has an
 *                order or a first without them;
 *   PZ_E_SIZE    num_members outside [1, 16];
 *   PZ_E_NULL    one of the 6 P member pointers is NULL; an agent's first is NULL while its order is not;
 *   PZ_E_SIZE    a size outside pikazoo_net.h's box, a pitch below its width, n * pitch * 4 bytes beyond int64;
 *   PZ_E_CONFIG  an unknown observation format, output format or activation;
 *   PZ_E_ALIGN   a pointer not aligned to its element (observations 4 or 2 bytes, parameters 4, outputs 4 or 2, order and
 *                first 4).
 * n == 0 returns PZ_OK without a launch.
 * pz_pool_plan checks:  PZ_E_NULL  order, first or errors NULL, members NULL with n > 0;  PZ_E_SIZE  n outside [0, 2^30],
 * num_members outside [1, 16];  PZ_E_CONFIG  an unknown member_format;  PZ_E_ALIGN  members not aligned to its element,
 * order, first or errors not 4-byte aligned.
 */
#ifndef PIKAZOO_POOL_H
#define PIKAZOO_POOL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_POOL_ABI_VERSION 1
#define PZ_POOL_MAX_MEMBERS 16
#define PZ_POOL_GROUP_ROWS 128

/* element type of the member vector */
enum pz_pool_member_format { PZ_POOL_MEMBER_UINT8 = 0, PZ_POOL_MEMBER_INT32 = 1, PZ_POOL_MEMBER_INT64 = 2 };

/* one pool member: the six nn.Linear tensors of its net, float32 device memory (shapes: pikazoo_net.h) */
typedef struct pz_pool_member {
    const float *w1;
    const float *b1;
    const float *w2;
    const float *b2;
    const float *w3;
    const float *b3;
} pz_pool_member;

int pz_pool_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_pool_build_id(void);

/* the int32 words of `order` for n rows and num_members members: (n / G + num_members) * G; -1 if either is out of range */
int64_t pz_pool_capacity(int64_t n, int32_t num_members);

int pz_pool_plan(const void *members, int32_t member_format, int64_t n, int32_t num_members, int32_t *order, int32_t *first, int32_t *errors, void *stream);

int pz_mlp_forward_pool(const void *obs_p1, const void *obs_p2, int32_t obs_format, int64_t n, int32_t in_features,
                        int64_t obs_pitch, int32_t hidden, int32_t out_features, int32_t activation,
                        const pz_pool_member *members, int32_t num_members, const int32_t *order_p1, const int32_t *first_p1,
                        const int32_t *order_p2, const int32_t *first_p2, void *out_p1, void *out_p2, int32_t out_format,
                        int64_t out_pitch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_POOL_H */
