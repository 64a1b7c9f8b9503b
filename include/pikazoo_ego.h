/* pikazoo_ego.h -- C ABI of libpikazoo_ego.so: the EGOCENTRIC view of an observation row -- the row that the same player
 * would be handed in the game mirrored about the court's centre line, so that player_2 sees the court as player_1 does
 * (pz_ego_rows), and the matching involution of the 18 absolute actions (pz_ego_actions), each in ONE launch.
 *
 * A library of its own beside libpikazoo_hip.so (built by pika-zoo_amd/build.py, same flags, same build id): it reads and
 * writes caller-owned device memory only, and nothing in the step path or in the other libraries loads it.  Every call is one
 * launch on `stream` (a hipStream_t passed as void*), allocates nothing, does not synchronise and is graph-capturable.
 *
 * ---- THE ROW (pz_ego_rows) ------------------------------------------------------------------------------------------------------
 * A row is PZ_OBS_DIM = 35 elements (pikazoo_hip.h): the own player at 0-12, the other player at 13-25, the ball at 26-34.
 * Eight columns are MIRRORED, the other 27 are copied bit for bit:
 *     column   0  13  26  28  30     both players' x; the ball's x, previous x and previous-previous x       M_j = 432
 *     column   3  16  32             both diving directions; the ball's x velocity                           M_j = 0
 * Raw formats (PZ_OBS_I32, PZ_OBS_I16, PZ_OBS_F16, PZ_OBS_BF16):              out = M_j - v
 * Normalised formats (PZ_OBS_F32_NORM, PZ_OBS_F16_NORM, PZ_OBS_BF16_NORM):    out = c_j - s
 *     with c_j = (M_j - 2 low_j) / (high_j - low_j) over the bounds of the row (pikazoo_env.py:485-562): c_j = 1.0f for seven of
 *     the columns, and c_26 = 0x1.e72548p-1f, the float32 nearest to 392 / 412 -- the ball's x has the bounds [20, 432], which
 *     are not symmetric about 216.
 * Arithmetic.  Integer formats: exact integer subtraction (int16: the low 16 bits of it).  Float formats: the stored element
 * is widened to float32 (exact), ONE float32 subtraction is done, and the difference is rounded to nearest even into the
 * row's format (float32: no rounding).  A NaN stays a NaN (bfloat16: the high half with its quiet bit set).  The definition is
 * of the STORED value, so it is fixed bit for bit in every format.
 *
 * Distance from "normalise the mirrored integer", what a mirror fused into the step would have produced (checked on the host
 * for every value inside the bounds of all eight columns): float32-normalised at most 2^-24 absolute; float16-normalised at
 * most 2^-11 and bfloat16-normalised at most 2^-8 (half an ulp of the input below 1 plus half an ulp of the output); raw
 * int32, int16 and float16: none; raw bfloat16: within 2 of the mirrored integer, because the env's bfloat16 rows are already
 * rounded above 256.
 *
 *     in, out     device rows of `format` (enum pz_obs_format, 0-6): row r begins at element r * in_pitch / r * out_pitch.
 *                 Aligned to the ELEMENT only (2 or 4 bytes): a view that begins at row 1 of a 2-byte tensor is taken.
 *     rows        0 <= rows, and rows * pitch elements within int64 bytes.  rows == 0 returns PZ_OK without a launch.
 *     in_pitch, out_pitch   in elements, >= 35.  The elements of `out` between column 35 and the pitch are NEVER written.
 *     in == out with in_pitch == out_pitch is allowed (every element is read and written by one thread).  Any other overlap
 *                 of the byte ranges [p, p + ((rows - 1) * pitch + 35) * element) is refused: PZ_E_EGO_OVERLAP.
 * Rows with both pitches 35 go as one flat array of rows * 35 elements in 16-byte accesses where `in` and `out` have the same
 * offset within 16 bytes; every other case goes element by element.  The result is the same.
 *
 * ---- THE ACTIONS (pz_ego_actions) -----------------------------------------------------------------------------------------------
 * Mirroring the game swaps the left and the right key.  On the 18 absolute actions (the key table of pikazoo_env.py:121-138
 * with its columns 0 and 1 swapped) that is the involution
 *     pi = (0, 1, 2, 4, 3, 5, 7, 6, 9, 8, 10, 12, 11, 13, 15, 14, 17, 16)
 * which agrees with the two tuples of SimplifyAction (simplify_action.py:17-18): pi[player_1's tuple[i]] = player_2's tuple[i].
 *     out[i] = pi[in[i]] for 0 <= in[i] < 18 on the FULL value of the element; any other value is stored unchanged, so that
 *     the env's range check still sees it.  action_format: enum pz_action_format (int32, int64, uint8, int16).  in == out is
 *     allowed; any other overlap of the two ranges: PZ_E_EGO_OVERLAP.  n == 0 returns PZ_OK without a launch.
 *
 * Return codes: pikazoo_hip.h's (PZ_OK 0, PZ_E_NULL -1, PZ_E_SIZE -2, PZ_E_CONFIG -3, PZ_E_ALIGN -4), PZ_E_EGO_OVERLAP -5, and a
 * positive value is the hipError_t of the launch.  Checked before the launch, in this order (both calls):
 *   PZ_E_NULL         in or out NULL with rows > 0 (n > 0);
 *   PZ_E_SIZE         rows < 0 or n < 0; a pitch below 35; rows * pitch (n) elements of the widest format beyond int64 bytes;
 *   PZ_E_CONFIG       an unknown format / action_format;
 *   PZ_E_ALIGN        in or out not aligned to its element;
 *   then rows == 0 / n == 0 returns PZ_OK;
 *   PZ_E_EGO_OVERLAP  the byte ranges overlap and it is not (in == out with equal pitches).
 */
#ifndef PIKAZOO_EGO_H
#define PIKAZOO_EGO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PZ_EGO_ABI_VERSION 1
#define PZ_EGO_COURT_WIDTH 432      /* M_j of the five x columns */
#define PZ_E_EGO_OVERLAP (-5)

int pz_ego_abi_version(void);
/* source digest this library was compiled from: equals pz_build_id() of the product library built beside it */
const char *pz_ego_build_id(void);
/* the text of a return code of this library (negative codes; NULL for PZ_OK, "HIP error" for a positive one) */
const char *pz_ego_error_string(int code);

int pz_ego_rows(const void *in, void *out, int32_t format, int64_t rows, int64_t in_pitch, int64_t out_pitch, void *stream);

int pz_ego_actions(const void *in, void *out, int32_t action_format, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKAZOO_EGO_H */
