// libpikazoo_learn.so (include/pikazoo_learn.h): GAE(gamma, lambda) over the [k, N] trajectory tensors of a k-step launch.
//
// The shape and the schedule are pz_traj_scan.hpp's, shared with pz_vtrace.hip: one lane per game, blockIdx.y = agent, one
// wave per workgroup, the loads a chunk of kChunk rows ahead of the serial scan.  This file holds what is GAE's own: three
// input streams per agent (reward, value, flag per row; the extra value row is carried from chunk to chunk) and five float
// operations per row, in the order the header pins.  Stores are non-temporal and never waited for.
//
// The formats are compile-time instantiations (2 reward x 3 value formats = 6 kernels); the arithmetic is the same text
// for all of them.  No multiply-add may be contracted: the pragma below holds for the whole translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_learn.h"

#pragma clang fp contract(off)

#include "pz_traj_scan.hpp"

namespace pz_learn {

using namespace pz_traj;

static_assert(PZ_GAE_REWARD_INT32 == kRewardInt32 && PZ_GAE_REWARD_FLOAT32 == kRewardFloat32, "pz_traj_scan.hpp: the reward formats");
static_assert(PZ_GAE_VALUE_FLOAT32 == kValueFloat32 && PZ_GAE_VALUE_FLOAT16 == kValueFloat16 && PZ_GAE_VALUE_BFLOAT16 == kValueBfloat16,
              "pz_traj_scan.hpp: the value formats");

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

// what a lane keeps over the whole scan: its column of every tensor, the pitches, the two carried values
template <int RF, int VF>
struct Lane {
    using Raw = typename ValueRaw<VF>::type;
    // per buffer: 8 rewards, 8 values, 8 flags (the extra value row is carried from chunk to chunk)
    struct Chunk {
        uint32_t r[kChunk];
        Raw v[kChunk];
        uint8_t d[kChunk];
    };
    const uint32_t* rew;
    const Raw* val;
    const uint8_t* term;
    float* adv;
    float* ret;
    int64_t rew_pitch, term_pitch, val_pitch, out_pitch;
    float gamma, gl;
    float v_next, a_next;

    // five float operations, in the order the header pins
    __device__ __forceinline__ void scan(int64_t t, uint32_t r_bits, Raw v_bits, uint8_t d)
    {
        const bool nt = d == 0;
        const float r = reward_of<RF>(r_bits), v = value_of<VF>(v_bits);
        const float q = nt ? gamma * v_next : 0.0f;
        const float delta = (r + q) - v;
        const float a = delta + (nt ? gl * a_next : 0.0f);
        __builtin_nontemporal_store(a, adv + t * out_pitch);
        __builtin_nontemporal_store(a + v, ret + t * out_pitch);
        a_next = a;
        v_next = v;
    }

    __device__ __forceinline__ void scan_row(int64_t t) { scan(t, rew[t * rew_pitch], val[t * val_pitch], term[t * term_pitch]); }

    __device__ __forceinline__ void load_chunk(int64_t t0, Chunk& c) const
    {
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            c.r[i] = rew[(t0 + i) * rew_pitch];
            c.v[i] = val[(t0 + i) * val_pitch];
            c.d[i] = term[(t0 + i) * term_pitch];
        }
    }

    __device__ __forceinline__ void scan_chunk(int64_t t0, const Chunk& c)
    {
#pragma unroll
        for (int i = kChunk - 1; i >= 0; --i) scan(t0 + i, c.r[i], c.v[i], c.d[i]);
    }
};

template <int RF, int VF>
__global__ void __launch_bounds__(kLanes) gae_kernel(const GaeArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.n) return;
    const bool second = blockIdx.y != 0;
    Lane<RF, VF> s;
    s.rew = (const uint32_t*)(second ? a.rew_p2 : a.rew_p1) + g;
    s.val = (const typename Lane<RF, VF>::Raw*)(second ? a.val_p2 : a.val_p1) + g;
    s.term = a.term + g;
    s.adv = (second ? a.adv_p2 : a.adv_p1) + g;
    s.ret = (second ? a.ret_p2 : a.ret_p1) + g;
    s.rew_pitch = a.rew_pitch, s.term_pitch = a.term_pitch, s.val_pitch = a.val_pitch, s.out_pitch = a.out_pitch;
    s.gamma = a.gamma, s.gl = a.gl;
    s.v_next = value_of<VF>(s.val[a.k * s.val_pitch]);
    s.a_next = 0.0f;
    scan_rows(s, a.k);
}

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
    if (!sizes_fit(k, n, {rew_pitch, term_pitch, val_pitch, out_pitch})) return PZ_E_SIZE;
    if (!known_formats(reward_format, value_format)) return PZ_E_CONFIG;
    if (!unit(gamma) || !unit(lam)) return PZ_E_CONFIG;
    const uintptr_t vb = value_bytes(value_format);
    if (misaligned(rew_p1, 4) || misaligned(rew_p2, 4) || misaligned(val_p1, vb) || misaligned(val_p2, vb) || misaligned(adv_p1, 4) ||
        misaligned(adv_p2, 4) || misaligned(ret_p1, 4) || misaligned(ret_p2, 4))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const GaeArgs a{rew_p1, rew_p2,    terminated, val_p1,    val_p2, adv_p1, adv_p2, ret_p1,
                    ret_p2, n,         rew_pitch,  term_pitch, val_pitch, out_pitch, k,      gamma,
                    gamma * lam};
    dispatch_formats(reward_format, value_format, [&](auto rf, auto vf) {
        hipLaunchKernelGGL((gae_kernel<decltype(rf)::value, decltype(vf)::value>), grid_of(n, second == 4), dim3(kLanes), 0,
                           (hipStream_t)stream, a);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
