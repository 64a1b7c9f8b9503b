// libpikazoo_league.so: the results of the games that ended on a step, accumulated per pair of pool members
// (pz_league_tally), and a member per game drawn with integer weights from a counter (pz_league_draw), each in ONE launch
// (C ABI and the definitions: include/pikazoo_league.h; the shape and its reasons: DESIGN.md 4.22).
//
// TALLY.  One workgroup of 256 threads looks at a tile of 1024 games.  Each thread reads the termination bytes of its four
// games; a workgroup whose tile holds no finished game -- nearly all of them, a game ends once in thousands of frames -- leaves
// after one barrier, without touching LDS or reading a score.  Otherwise the workgroup zeroes a [P][P][4] table of 64-bit
// words in LDS, every finished game adds its four words there with LDS atomics, and each NON-ZERO cell is added to the
// caller's table with one 64-bit integer atomicAdd.  Integer sums: the order of the adds does not show in the result.
// DRAW.  One thread per game.  Every thread sums the (at most sixteen, wave-uniform) weights into registers, checks them,
// runs one Philox block for its game and counts the prefix sums that do not exceed its scaled word.
// Nothing is written by a scalar unit: `errors` of the draw is set by lane 0 of every workgroup with an ordinary store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_league.h"

namespace pz_league {

constexpr int kThreads = 256;
constexpr int kTallyPerThread = 4;                          // games per thread of the tally
constexpr int kTallyTile = kThreads * kTallyPerThread;      // games per workgroup of the tally
constexpr int kMaxMembers = PZ_LEAGUE_MAX_MEMBERS;
constexpr int kCell = PZ_LEAGUE_CELL_WORDS;
constexpr int64_t kMaxGames = (int64_t)1 << 30;
// the VALUES of pz_pool_member_format (pikazoo_pool.h)
enum MemberFormat { kMemberUint8 = 0, kMemberInt32 = 1, kMemberInt64 = 2 };

using u64 = unsigned long long;

// Philox4x32-10 (Salmon et al., SC'11), the first two words of the block
__device__ __forceinline__ uint64_t philox4x32_10_low64(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        c1 = (uint32_t)p1;
        c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ((uint64_t)c1 << 32) | c0;
}

// element g of a member vector as int64 (the range check is the caller's)
__device__ __forceinline__ int64_t load_member(const void* p, int format, int64_t g)
{
    if (format == kMemberUint8) return ((const uint8_t*)p)[g];
    if (format == kMemberInt32) return ((const int32_t*)p)[g];
    return ((const int64_t*)p)[g];
}

__device__ __forceinline__ void store_member(void* p, int format, int64_t g, uint32_t m)
{
    if (format == kMemberUint8)
        ((uint8_t*)p)[g] = (uint8_t)m;
    else if (format == kMemberInt32)
        ((int32_t*)p)[g] = (int32_t)m;
    else
        ((int64_t*)p)[g] = (int64_t)m;
}

__device__ __forceinline__ int64_t load_score(const void* p, int format, int64_t at)
{
    return format == PZ_LEAGUE_SCORE_INT32 ? (int64_t)((const int32_t*)p)[at] : (int64_t)((const int16_t*)p)[at];
}

__global__ __launch_bounds__(kThreads) void tally_kernel(const uint8_t* __restrict__ terminated, const void* __restrict__ score_p1,
                                                         const void* __restrict__ score_p2, int score_format, int64_t score_stride,
                                                         const void* __restrict__ members_p1, const void* __restrict__ members_p2,
                                                         int member_format, int64_t n, int P, u64* table, u64* errors)
{
    __shared__ u64 s_table[kMaxMembers * kMaxMembers * kCell];  // 8 KiB
    __shared__ uint32_t s_errors;
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * kTallyTile;
    // thread t takes games g0 + t, g0 + t + 256, ...: a wave reads 64 consecutive bytes
    uint32_t ended = 0;
#pragma unroll
    for (int i = 0; i < kTallyPerThread; ++i) {
        const int64_t g = g0 + i * kThreads + tid;
        if (g < n && terminated[g] != 0) ended |= 1u << i;
    }
    if (!__syncthreads_or(ended != 0)) return;  // (uniform: the whole workgroup leaves)

    const int cells = P * P * kCell;
    for (int c = tid; c < cells; c += kThreads) s_table[c] = 0;
    if (tid == 0) s_errors = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTallyPerThread; ++i) {
        if (!(ended & (1u << i))) continue;
        const int64_t g = g0 + i * kThreads + tid;
        const int64_t a = members_p1 != nullptr ? load_member(members_p1, member_format, g) : 0;
        const int64_t b = load_member(members_p2, member_format, g);
        if ((uint64_t)a >= (uint64_t)P || (uint64_t)b >= (uint64_t)P) {
            atomicAdd(&s_errors, 1u);
            continue;
        }
        const int64_t s1 = load_score(score_p1, score_format, g * score_stride);
        const int64_t s2 = load_score(score_p2, score_format, g * score_stride);
        u64* cell = s_table + ((int)a * P + (int)b) * kCell;
        atomicAdd(cell + 0, (u64)1);
        if (s1 > s2) atomicAdd(cell + 1, (u64)1);
        if (s1 != 0) atomicAdd(cell + 2, (u64)s1);
        if (s2 != 0) atomicAdd(cell + 3, (u64)s2);
    }
    __syncthreads();
    for (int c = tid; c < cells; c += kThreads) {
        const u64 v = s_table[c];
        if (v != 0) atomicAdd(table + c, v);
    }
    if (tid == 0 && s_errors != 0) atomicAdd(errors, (u64)s_errors);
}

__global__ __launch_bounds__(kThreads) void draw_kernel(const int64_t* __restrict__ weights, int P, uint32_t key0, uint32_t key1, uint64_t counter,
                                                        const uint64_t* __restrict__ counter_dev, int64_t first_game,
                                                        const uint8_t* __restrict__ mask, void* members, int member_format, int64_t n,
                                                        int32_t* errors)
{
    uint64_t cum[kMaxMembers];
    uint64_t W = 0;
    bool valid = true;
#pragma unroll
    for (int p = 0; p < kMaxMembers; ++p) {
        if (p < P) {
            const int64_t w = weights[p];
            valid = valid && (uint64_t)w < ((uint64_t)1 << 32);
            W += (uint64_t)w & 0xFFFFFFFFu;  // (an invalid weight's sum is never used)
        }
        cum[p] = W;
    }
    if (!valid || W == 0) {
        if (threadIdx.x == 0) *errors = 1;
        return;
    }
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    if (mask != nullptr && mask[g] == 0) return;
    const uint64_t C = counter + (counter_dev != nullptr ? *counter_dev : 0);
    const uint64_t G = (uint64_t)first_game + (uint64_t)g;
    const uint64_t u = philox4x32_10_low64((uint32_t)G, (uint32_t)(G >> 32), (uint32_t)C, (uint32_t)(C >> 32), key0, key1);
    const uint64_t r = __umul64hi(u, W);
    uint32_t m = 0;
#pragma unroll
    for (int p = 0; p < kMaxMembers; ++p) m += (p < P && cum[p] <= r) ? 1u : 0u;
    store_member(members, member_format, g, m);
}

static int member_bytes(int32_t format) { return format == kMemberUint8 ? 1 : format == kMemberInt32 ? 4 : 8; }

}  // namespace pz_league

using namespace pz_league;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kLeagueBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_league_build_id(void) { return kLeagueBuildIdRecord + 12; }

int pz_league_abi_version(void) { return PZ_LEAGUE_ABI_VERSION; }

int pz_league_tally(const uint8_t* terminated, const void* score_p1, const void* score_p2, int32_t score_format, int64_t score_stride,
                    const void* members_p1, const void* members_p2, int32_t member_format, int64_t n, int32_t num_members, int64_t* table,
                    int64_t* errors, void* stream)
{
    if (table == nullptr || errors == nullptr) return PZ_E_NULL;
    if (n > 0 && (terminated == nullptr || score_p1 == nullptr || score_p2 == nullptr || members_p2 == nullptr)) return PZ_E_NULL;
    if (n < 0 || n > kMaxGames || num_members < 1 || num_members > kMaxMembers || score_stride < 1) return PZ_E_SIZE;
    int64_t extent;  // bytes up to the last score read (an element has at most 4)
    if (__builtin_mul_overflow(n, score_stride, &extent) || __builtin_mul_overflow(extent, (int64_t)4, &extent)) return PZ_E_SIZE;
    if (score_format != PZ_LEAGUE_SCORE_INT32 && score_format != PZ_LEAGUE_SCORE_INT16) return PZ_E_CONFIG;
    if (member_format < kMemberUint8 || member_format > kMemberInt64) return PZ_E_CONFIG;
    const uintptr_t sb = score_format == PZ_LEAGUE_SCORE_INT32 ? 4 : 2, mb = (uintptr_t)member_bytes(member_format);
    if ((((uintptr_t)table | (uintptr_t)errors) & 7) || (((uintptr_t)score_p1 | (uintptr_t)score_p2) & (sb - 1)) ||
        (((uintptr_t)members_p1 | (uintptr_t)members_p2) & (mb - 1)))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    hipLaunchKernelGGL(tally_kernel, dim3((unsigned)((n + kTallyTile - 1) / kTallyTile)), dim3(kThreads), 0, (hipStream_t)stream, terminated, score_p1,
                       score_p2, (int)score_format, score_stride, members_p1, members_p2, (int)member_format, n, (int)num_members, (u64*)table,
                       (u64*)errors);
    return (int)hipGetLastError();
}

int pz_league_draw(const int64_t* weights, int32_t num_members, uint64_t seed, uint64_t counter, const uint64_t* counter_dev, int64_t first_game,
                   const uint8_t* mask, void* members, int32_t member_format, int64_t n, int32_t* errors, void* stream)
{
    if (weights == nullptr || errors == nullptr || (n > 0 && members == nullptr)) return PZ_E_NULL;
    if (n < 0 || n > kMaxGames || num_members < 1 || num_members > kMaxMembers || counter >= ((uint64_t)1 << 62)) return PZ_E_SIZE;
    if (member_format < kMemberUint8 || member_format > kMemberInt64) return PZ_E_CONFIG;
    const uintptr_t mb = (uintptr_t)member_bytes(member_format);
    if ((((uintptr_t)weights | (uintptr_t)counter_dev) & 7) || ((uintptr_t)errors & 3) || ((uintptr_t)members & (mb - 1))) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, weights,
                       (int)num_members, (uint32_t)seed ^ 0x4C454147u, (uint32_t)(seed >> 32) ^ 0x44524157u, counter, counter_dev, first_game, mask,
                       members, (int)member_format, n, errors);
    return (int)hipGetLastError();
}

}  // extern "C"
