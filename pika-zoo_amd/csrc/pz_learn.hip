// libpikazoo_learn.so (include/pikazoo_learn.h): GAE(gamma, lambda) over the [k, N] trajectory tensors of a k-step launch.
//
// One lane per game, blockIdx.y = agent, one wave (64 consecutive games) per workgroup: every row access of a wave is one
// coalesced segment.  The scan over time is serial per game -- five float operations per row, in the order the header
// pins -- and the loads do not depend on it: they are issued a chunk of kChunk rows ahead into a second register buffer
// (reward, value, flag per row; the extra value row is carried from chunk to chunk), so the wave waits on vmcnt for the
// chunk it scans while the next one is in flight.  The rows above the last multiple of kChunk are scanned first, one by
// one.  Stores are non-temporal and never waited for.
//
// The formats are compile-time instantiations (2 reward x 3 value formats = 6 kernels); the arithmetic is the same text
// for all of them.  No multiply-add may be contracted: the pragma below holds for the whole translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_learn.h"

#pragma clang fp contract(off)

namespace pz_learn {

constexpr int kLanes = 64;  // games per workgroup: one wave
constexpr int kChunk = 8;   // rows loaded ahead of the scan (per buffer: 8 rewards, 8 values, 8 flags)

struct GaeArgs {
    const void* rew_p1;
    const void* rew_p2;
    const uint8_t* term;
    const void* val_p1;
    const void* val_p2;
    float* adv_p1;
    float* adv_p2;
    float* ret_p1;
    float* ret_p2;
    int64_t n, rew_pitch, term_pitch, val_pitch, out_pitch;
    int32_t k;
    float gamma, gl;
};

// a reward row element is 4 bytes in both formats: loaded as its bits, converted where it is used
template <int RF>
__device__ __forceinline__ float reward_of(uint32_t bits)
{
    return RF == PZ_GAE_REWARD_INT32 ? (float)(int32_t)bits : __uint_as_float(bits);
}

template <int VF>
struct ValueRaw {
    using type = uint16_t;
};
template <>
struct ValueRaw<PZ_GAE_VALUE_FLOAT32> {
    using type = uint32_t;
};

template <int VF>
__device__ __forceinline__ float value_of(typename ValueRaw<VF>::type bits)
{
    if constexpr (VF == PZ_GAE_VALUE_FLOAT32)
        return __uint_as_float(bits);
    else if constexpr (VF == PZ_GAE_VALUE_FLOAT16)
        return (float)__builtin_bit_cast(_Float16, bits);  // exact
    else
        return __uint_as_float((uint32_t)bits << 16);  // bfloat16 is the upper half of a float32: exact
}

template <int VF>
struct Chunk {
    uint32_t r[kChunk];
    typename ValueRaw<VF>::type v[kChunk];
    uint8_t d[kChunk];
};

// what a lane keeps over the whole scan: its column of every tensor, the pitches, the two carried values
template <int VF>
struct Lane {
    const uint32_t* rew;
    const typename ValueRaw<VF>::type* val;
    const uint8_t* term;
    float* adv;
    float* ret;
    int64_t rew_pitch, term_pitch, val_pitch, out_pitch;
    float gamma, gl;
    float v_next, a_next;
};

template <int RF, int VF>
__device__ __forceinline__ void scan_row(Lane<VF>& s, int64_t t, uint32_t r_bits, typename ValueRaw<VF>::type v_bits, uint8_t d)
{
    const bool nt = d == 0;
    const float r = reward_of<RF>(r_bits), v = value_of<VF>(v_bits);
    const float q = nt ? s.gamma * s.v_next : 0.0f;
    const float delta = (r + q) - v;
    const float a = delta + (nt ? s.gl * s.a_next : 0.0f);
    __builtin_nontemporal_store(a, s.adv + t * s.out_pitch);
    __builtin_nontemporal_store(a + v, s.ret + t * s.out_pitch);
    s.a_next = a;
    s.v_next = v;
}

template <int VF>
__device__ __forceinline__ void load_chunk(const Lane<VF>& s, int64_t t0, Chunk<VF>& c)
{
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
        c.r[i] = s.rew[(t0 + i) * s.rew_pitch];
        c.v[i] = s.val[(t0 + i) * s.val_pitch];
        c.d[i] = s.term[(t0 + i) * s.term_pitch];
    }
}

template <int RF, int VF>
__device__ __forceinline__ void scan_chunk(Lane<VF>& s, int64_t t0, const Chunk<VF>& c)
{
#pragma unroll
    for (int i = kChunk - 1; i >= 0; --i) scan_row<RF, VF>(s, t0 + i, c.r[i], c.v[i], c.d[i]);
}

template <int RF, int VF>
__global__ void __launch_bounds__(kLanes) gae_kernel(const GaeArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.n) return;
    const bool second = blockIdx.y != 0;
    using V = typename ValueRaw<VF>::type;
    Lane<VF> s;
    s.rew = (const uint32_t*)(second ? a.rew_p2 : a.rew_p1) + g;
    s.val = (const V*)(second ? a.val_p2 : a.val_p1) + g;
    s.term = a.term + g;
    s.adv = (second ? a.adv_p2 : a.adv_p1) + g;
    s.ret = (second ? a.ret_p2 : a.ret_p1) + g;
    s.rew_pitch = a.rew_pitch, s.term_pitch = a.term_pitch, s.val_pitch = a.val_pitch, s.out_pitch = a.out_pitch;
    s.gamma = a.gamma, s.gl = a.gl;
    int64_t t = a.k;  // rows [0, t) are still to scan
    s.v_next = value_of<VF>(s.val[t * s.val_pitch]);
    s.a_next = 0.0f;
    // the rows above the last multiple of kChunk, one by one
    for (int rest = a.k % kChunk; rest > 0; --rest) {
        --t;
        scan_row<RF, VF>(s, t, s.rew[t * s.rew_pitch], s.val[t * s.val_pitch], s.term[t * s.term_pitch]);
    }
    if (t == 0) return;
    // t is a multiple of kChunk: chunk by chunk, the next one loading into the other buffer while this one is scanned
    // (two chunks per trip, so that the buffers swap roles without a copy; no load sits behind a condition inside it)
    Chunk<VF> c0, c1;
    load_chunk<VF>(s, t - kChunk, c0);
    while (t >= 3 * kChunk) {
        load_chunk<VF>(s, t - 2 * kChunk, c1);
        scan_chunk<RF, VF>(s, t - kChunk, c0);
        load_chunk<VF>(s, t - 3 * kChunk, c0);
        scan_chunk<RF, VF>(s, t - 2 * kChunk, c1);
        t -= 2 * kChunk;
    }
    if (t == 2 * kChunk) {
        load_chunk<VF>(s, 0, c1);
        scan_chunk<RF, VF>(s, kChunk, c0);
        scan_chunk<RF, VF>(s, 0, c1);
    } else {
        scan_chunk<RF, VF>(s, 0, c0);
    }
}

template <int RF, int VF>
static void launch(const GaeArgs& a, bool both, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.n + kLanes - 1) / kLanes), both ? 2 : 1);
    hipLaunchKernelGGL((gae_kernel<RF, VF>), grid, dim3(kLanes), 0, stream, a);
}

template <int RF>
static void launch_values(int value_format, const GaeArgs& a, bool both, hipStream_t stream)
{
    switch (value_format) {
        case PZ_GAE_VALUE_FLOAT32: launch<RF, PZ_GAE_VALUE_FLOAT32>(a, both, stream); break;
        case PZ_GAE_VALUE_FLOAT16: launch<RF, PZ_GAE_VALUE_FLOAT16>(a, both, stream); break;
        default: launch<RF, PZ_GAE_VALUE_BFLOAT16>(a, both, stream); break;
    }
}

static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

}  // namespace pz_learn

using namespace pz_learn;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kLearnBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_learn_build_id(void) { return kLearnBuildIdRecord + 12; }

int pz_learn_abi_version(void) { return PZ_LEARN_ABI_VERSION; }

int pz_gae(const void* rew_p1, const void* rew_p2, int32_t reward_format, const uint8_t* terminated, const void* val_p1,
           const void* val_p2, int32_t value_format, int32_t k, int64_t n, int64_t rew_pitch, int64_t term_pitch,
           int64_t val_pitch, int64_t out_pitch, float gamma, float lam, float* adv_p1, float* adv_p2, float* ret_p1,
           float* ret_p2, void* stream)
{
    if (!rew_p1 || !terminated || !val_p1 || !adv_p1 || !ret_p1) return PZ_E_NULL;
    const int second = (rew_p2 != nullptr) + (val_p2 != nullptr) + (adv_p2 != nullptr) + (ret_p2 != nullptr);
    if (second != 0 && second != 4) return PZ_E_NULL;  // agent 2: all four or none
    if (k < 1 || n < 0) return PZ_E_SIZE;
    if (rew_pitch < n || term_pitch < n || val_pitch < n || out_pitch < n) return PZ_E_SIZE;
    // the kernel's addressing: a game index and a grid in 32 bits, byte offsets of up to k + 1 rows of 4-byte elements in int64
    if (n > ((int64_t)1 << 30)) return PZ_E_SIZE;
    const int64_t most = (INT64_MAX / 4) / ((int64_t)k + 1);
    if (rew_pitch > most || term_pitch > most || val_pitch > most || out_pitch > most) return PZ_E_SIZE;
    if (reward_format != PZ_GAE_REWARD_INT32 && reward_format != PZ_GAE_REWARD_FLOAT32) return PZ_E_CONFIG;
    if (value_format != PZ_GAE_VALUE_FLOAT32 && value_format != PZ_GAE_VALUE_FLOAT16 && value_format != PZ_GAE_VALUE_BFLOAT16)
        return PZ_E_CONFIG;
    if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lam >= 0.0f && lam <= 1.0f)) return PZ_E_CONFIG;  // (a NaN fails both)
    const uintptr_t value_bytes = value_format == PZ_GAE_VALUE_FLOAT32 ? 4 : 2;
    if (misaligned(rew_p1, 4) || misaligned(rew_p2, 4) || misaligned(val_p1, value_bytes) || misaligned(val_p2, value_bytes) ||
        misaligned(adv_p1, 4) || misaligned(adv_p2, 4) || misaligned(ret_p1, 4) || misaligned(ret_p2, 4))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const GaeArgs a{rew_p1, rew_p2,    terminated, val_p1,    val_p2, adv_p1, adv_p2, ret_p1,
                    ret_p2, n,         rew_pitch,  term_pitch, val_pitch, out_pitch, k,      gamma,
                    gamma * lam};
    if (reward_format == PZ_GAE_REWARD_INT32)
        launch_values<PZ_GAE_REWARD_INT32>(value_format, a, second == 4, (hipStream_t)stream);
    else
        launch_values<PZ_GAE_REWARD_FLOAT32>(value_format, a, second == 4, (hipStream_t)stream);
    return (int)hipGetLastError();
}

}  // extern "C"
