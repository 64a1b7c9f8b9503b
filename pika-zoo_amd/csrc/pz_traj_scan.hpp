// The backward scan over the [k, N] trajectory tensors of a k-step launch, shared by the translation units that run one
// (pz_learn.hip: GAE, pz_vtrace.hip: V-trace targets; tools/gae_variants.hip for its two-chains-per-lane form): the lane and
// chunk sizes, the reward and value formats, the schedule of loads against the serial chain, the dispatch of a launch to its
// format instantiation, and the argument checks both C entry points make.
//
// The shape, the right one for a serial scan: one lane per game, blockIdx.y = agent, one wave (64 consecutive games) per
// workgroup, so every row access of a wave is one coalesced segment.  The scan over time is serial per game and the loads do
// not depend on it: they are issued a chunk of kChunk rows ahead into a second register buffer, so the wave waits on vmcnt for
// the chunk it scans while the next one is in flight.  The rows above the last multiple of kChunk are scanned first, one by
// one.  What a row's arithmetic is, and which streams a chunk holds, is the including translation unit's: its lane state.
//
// No multiply-add of the arithmetic may be contracted: each translation unit sets `#pragma clang fp contract(off)` AHEAD of
// this include.
#ifndef PZ_TRAJ_SCAN_HPP
#define PZ_TRAJ_SCAN_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

namespace pz_traj {

constexpr int kLanes = 64;  // games per workgroup: one wave
// rows loaded ahead of the scan, per buffer.  8 is V-trace's budget: 5 registers per row and buffer make 80 VGPRs of staging,
// the chunk's 24 weights take the place of its 16 log-probs; with addresses and pitches its six kernels stay within 128 VGPRs,
// no scratch: 4 waves per SIMD, where 65 536 games of both agents fill 2.  A chunk of 16 would not fit 128 registers and would
// halve that.  GAE (3 registers per row and buffer) runs the same chunk: tests/gae_judge.py K_EDGES are the edges of 8.
constexpr int kChunk = 8;

// the formats, in the values of the public headers (each translation unit asserts that its PZ_GAE_* / PZ_VTRACE_* equal them)
constexpr int kRewardInt32 = 0, kRewardFloat32 = 1;
constexpr int kValueFloat32 = 0, kValueFloat16 = 1, kValueBfloat16 = 2;

// a reward row element is 4 bytes in both formats: loaded as its bits, converted where it is used
template <int RF>
__device__ __forceinline__ float reward_of(uint32_t bits)
{
    return RF == kRewardInt32 ? (float)(int32_t)bits : __uint_as_float(bits);
}

template <int VF>
struct ValueRaw {
    using type = uint16_t;
};
template <>
struct ValueRaw<kValueFloat32> {
    using type = uint32_t;
};

template <int VF>
__device__ __forceinline__ float value_of(typename ValueRaw<VF>::type bits)
{
    if constexpr (VF == kValueFloat32)
        return __uint_as_float(bits);
    else if constexpr (VF == kValueFloat16)
        return (float)__builtin_bit_cast(_Float16, bits);  // exact
    else
        return __uint_as_float((uint32_t)bits << 16);  // bfloat16 is the upper half of a float32: exact
}

// The schedule: rows [0, k) of one lane, from the last to the first.  `Lane` is what a lane keeps over the whole scan (its
// column of every tensor, the pitches, the carried values) and supplies
//   Lane::Chunk                       one buffer: kChunk rows of every input stream, as loaded
//   s.scan_row(t)                     load row t and scan it
//   s.load_chunk(t0, c)               load rows [t0, t0 + kChunk) into c
//   s.scan_chunk(t0, c)               scan them, from the last to the first
// The lane comes by value: nothing of it is read after the scan, and taken by reference the V-trace kernels were allocated up
// to 8 VGPRs more and ran 0.35 us longer at 4 096 games x 128 rows (profiles/traj_scan_ab.log).
template <class Lane>
__device__ __forceinline__ void scan_rows(Lane s, int32_t k)
{
    int64_t t = k;  // rows [0, t) are still to scan
    // the rows above the last multiple of kChunk, one by one
    for (int rest = k % kChunk; rest > 0; --rest) s.scan_row(--t);
    if (t == 0) return;
    // t is a multiple of kChunk: chunk by chunk, the next one loading into the other buffer while this one is scanned
    // (two chunks per trip, so that the buffers swap roles without a copy; no load sits behind a condition inside it)
    typename Lane::Chunk c0, c1;
    s.load_chunk(t - kChunk, c0);
    while (t >= 3 * kChunk) {
        s.load_chunk(t - 2 * kChunk, c1);
        s.scan_chunk(t - kChunk, c0);
        s.load_chunk(t - 3 * kChunk, c0);
        s.scan_chunk(t - 2 * kChunk, c1);
        t -= 2 * kChunk;
    }
    if (t == 2 * kChunk) {
        s.load_chunk(0, c1);
        s.scan_chunk(kChunk, c0);
        s.scan_chunk(0, c1);
    } else {
        s.scan_chunk(0, c0);
    }
}

// ---- the host side of a launch ----------------------------------------------------------------------------------------
static inline dim3 grid_of(int64_t n, bool both) { return dim3((unsigned)((n + kLanes - 1) / kLanes), both ? 2 : 1); }

// f(reward format, value format) with the two as std::integral_constant: one of the six instantiations
template <class F>
static void dispatch_formats(int reward_format, int value_format, F&& f)
{
    auto values = [&](auto rf) {
        switch (value_format) {
            case kValueFloat32: f(rf, std::integral_constant<int, kValueFloat32>{}); break;
            case kValueFloat16: f(rf, std::integral_constant<int, kValueFloat16>{}); break;
            default: f(rf, std::integral_constant<int, kValueBfloat16>{}); break;
        }
    };
    if (reward_format == kRewardInt32)
        values(std::integral_constant<int, kRewardInt32>{});
    else
        values(std::integral_constant<int, kRewardFloat32>{});
}

static inline bool known_formats(int reward_format, int value_format)
{
    return (reward_format == kRewardInt32 || reward_format == kRewardFloat32) &&
           (value_format == kValueFloat32 || value_format == kValueFloat16 || value_format == kValueBfloat16);
}
static inline uintptr_t value_bytes(int value_format) { return value_format == kValueFloat32 ? 4 : 2; }

static inline bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static inline bool unit(float x) { return x >= 0.0f && x <= 1.0f; }  // (a NaN fails both)

// k >= 1 rows of 0 <= n <= 2^30 games at pitches >= n -- the kernel's addressing: a game index and a grid in 32 bits, byte
// offsets of up to k + 1 rows of 4-byte elements in int64
static inline bool sizes_fit(int32_t k, int64_t n, std::initializer_list<int64_t> pitches)
{
    if (k < 1 || n < 0 || n > ((int64_t)1 << 30)) return false;
    const int64_t most = (INT64_MAX / 4) / ((int64_t)k + 1);
    for (const int64_t pitch : pitches)
        if (pitch < n || pitch > most) return false;
    return true;
}

}  // namespace pz_traj

#endif
