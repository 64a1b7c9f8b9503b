/* pikazoo_batch.h -- C ABI of libpikazoo_batch.so: the data movement of a PPO iteration -- filing one policy step's records
 * into the [k, n, ...] rollout buffers (pz_batch_copy) and delivering every tensor of a shuffled minibatch (pz_batch_gather),
 * each in ONE launch.  The permutation of the shuffle is computed inside the kernel from a counter: there is no randperm, no
 * index tensor, no allocation and no synchronisation.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device tensors only, and nothing in the step path or in the other libraries loads it.  Return codes are
 * pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4; a positive value is the hipError_t of
 * the launch).
 *
 * A COLUMN is one tensor of the rollout, described by bytes only: every dtype and every agent is just another column.  The
 * descriptors are HOST structs: they are read at call time and travel as kernel arguments, so a captured graph holds them by
 * value; there is no table in device memory and no allocation.  src and dst are caller-owned device memory.  Outputs must
 * not alias inputs or each other (not checked here).  Bytes between row_bytes and dst_pitch are not written.  Sources are
 * read only.  Every call is one launch on `stream` and is graph-capturable.
 *
 * pz_batch_copy(cols, ncols, n, stream): output row g of every column is source row g, for g < n:
 *     dst + g * dst_pitch  <-  src + g * src_game_pitch          (row_bytes bytes; src_step_pitch is ignored)
 * n == 0 returns PZ_OK without a launch.  ncols == 0 is PZ_E_NULL (there is nothing to write).
 *
 * pz_batch_gather(cols, ncols, k, n, minibatches, seed, counter, counter_dev, index_in, index_out, errors, stream):
 *     M = k * n flat rows, 1 <= M <= 2^31 (n == 0: PZ_OK without a launch);
 *     B = M / minibatches (integer division): the rows of one minibatch.  The M % minibatches positions past
 *         B * minibatches are not visited in an epoch.  B == 0 cannot happen (minibatches <= M).
 *     C = counter + (counter_dev ? *counter_dev : 0), in uint64.  The by-value part is frozen into a captured graph; the
 *         caller increments the device word inside the capture.  counter < 2^62.
 *     E = C / minibatches is the epoch, m = C % minibatches the minibatch.
 *     Output row j < B of every column is source row r = perm_E(m * B + j):
 *         dst + j * dst_pitch  <-  src + (r / n) * src_step_pitch + (r % n) * src_game_pitch        (row_bytes bytes)
 *     index_out  optional, device int64[B]: receives the r of each row.  ncols may be 0 when it is given.
 *     index_in   optional, device const int64[B]: replaces the permutation: r = index_in[j].  THEN `minibatches` IS NOT A
 *                NUMBER OF MINIBATCHES BUT B ITSELF, the number of output rows, 0 <= B <= 2^31 (B == 0: PZ_OK without a
 *                launch), and seed, counter and counter_dev are ignored (counter_dev is not read; counter is not
 *                range-checked).  Duplicates are allowed.
 *     errors     optional, device uint32: an r outside [0, M) (possible with index_in only) never causes an out-of-range
 *                read: that output row is written as zero bytes in every column, index_out receives the r as given, and
 *                *errors is set to 1 by an ordinary vector store.  *errors is never cleared here.
 *
 * THE PERMUTATION perm_E of [0, M), in integers (uint32 unless said otherwise):
 *     b = max(2, bit_length(M - 1)),  hb = (b + 1) / 2,  mask = 2^hb - 1
 *     K[0..5]: the first six of the eight words of two Philox4x32-10 blocks (Salmon et al., SC'11) with
 *         key      ((uint32) seed ^ 0x53485546, (uint32) (seed >> 32) ^ 0x42415443)
 *         counter  ((uint32) E, (uint32) (E >> 32), j, 0)     for j = 0 (K[0..3]) and j = 1 (K[4..5])
 *       (the key is XORed because the env, the policy head and the random policy already occupy every residue of counter
 *       word 3 under the plain seed: a caller who reuses the env's seed gets no correlated stream)
 *     mix(v):  v *= 0x9E3779B1; v ^= v >> 15; v *= 0x85EBCA77; v ^= v >> 13; v *= 0xC2B2AE3D; v ^= v >> 16
 *     perm(p): x = p
 *              repeat
 *                  L = x >> hb, R = x & mask
 *                  six rounds r = 0..5 of  (L, R) = (R, L ^ (mix(R ^ K[r]) >> (32 - hb)))
 *                  x = (L << hb) | R
 *              while x >= M                     (compared unsigned; at M = 2^31 the domain is all of uint32)
 * A Feistel network is a bijection of [0, 2^(2 hb)) whatever mix is, and cycle walking restricts it to [0, M).  The domain
 * is below 4 M, so the mean walk is below 4 passes.
 *
 * Checked before the launch, in this order:
 *   PZ_E_NULL    cols NULL, or a src / dst NULL, with ncols > 0; ncols == 0 without index_out (pz_batch_copy: ncols == 0);
 *   PZ_E_SIZE    ncols outside [0, 16]; k < 1, n < 0, M > 2^31, minibatches outside [1, M] (with index_in: outside
 *                [0, 2^31]); row_bytes outside [1, 512]; src_game_pitch, dst_pitch or (pz_batch_gather) src_step_pitch
 *                below row_bytes; counter >= 2^62 (without index_in); a column's source or destination extent in bytes
 *                that does not fit int64;
 *   PZ_E_CONFIG  elem_bytes not in {1, 2, 4, 8};
 *   PZ_E_ALIGN   src, dst, a pitch (pz_batch_copy: src_step_pitch excepted) or row_bytes that is not a multiple of its
 *                elem_bytes; counter_dev, index_in or index_out not 8-byte aligned; errors not 4-byte aligned.
 */
#ifndef PIKAZOO_BATCH_H
#define PIKAZOO_BATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_BATCH_ABI_VERSION 1
#define PZ_BATCH_MAX_COLUMNS 16
#define PZ_BATCH_MAX_ROW_BYTES 512

typedef struct pz_batch_column {
    const void *src;
    void *dst;
    int64_t src_step_pitch; /* bytes from row (t, g) to (t + 1, g); ignored by pz_batch_copy */
    int64_t src_game_pitch; /* bytes from row (t, g) to (t, g + 1): >= row_bytes, or a stride (the value column of a head) */
    int64_t dst_pitch;      /* bytes between output rows, >= row_bytes */
    int32_t row_bytes;      /* 1 .. 512 */
    int32_t elem_bytes;     /* 1, 2, 4 or 8: src, dst, every pitch and row_bytes are multiples of it */
} pz_batch_column;

int pz_batch_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_batch_build_id(void);

int pz_batch_copy(const pz_batch_column *cols, int32_t ncols, int64_t n, void *stream);
int pz_batch_gather(const pz_batch_column *cols, int32_t ncols, int64_t k, int64_t n, int64_t minibatches, uint64_t seed, uint64_t counter, const uint64_t *counter_dev, const int64_t *index_in, int64_t *index_out, uint32_t *errors, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_BATCH_H */
