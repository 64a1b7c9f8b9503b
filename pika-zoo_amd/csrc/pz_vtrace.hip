// libpikazoo_vtrace.so (include/pikazoo_vtrace.h): V-trace targets over the [k, N] trajectory tensors of a k-step launch.
//
// The shape and the schedule are pz_traj_scan.hpp's, shared with pz_learn.hip: one lane per game, blockIdx.y = agent, one
// wave per workgroup, the loads a chunk of kChunk rows ahead of the serial scan.  This file holds what is V-trace's own: five
// input streams per agent (reward, value, flag, behaviour and target log-prob), and what does not depend on the scan -- the
// expf of the log-ratio, the three selects against the clips and the product gl * c -- computed for the whole chunk AHEAD of
// the serial chain (scan_chunk's first loop), so the dependent chain per row stays one multiply and one add.  Stores are
// non-temporal and never waited for.  The six kernels come to 109 .. 121 VGPRs, no scratch (pz_traj_scan.hpp: kChunk).
//
// The formats are compile-time instantiations (2 reward x 3 value formats = 6 kernels); the arithmetic is the same text
// for all of them.  No multiply-add may be contracted: the pragma below holds for the whole translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_vtrace.h"

#pragma clang fp contract(off)

#include "pz_traj_scan.hpp"

namespace pz_vt {

using namespace pz_traj;

static_assert(PZ_VTRACE_REWARD_INT32 == kRewardInt32 && PZ_VTRACE_REWARD_FLOAT32 == kRewardFloat32, "pz_traj_scan.hpp: the reward formats");
static_assert(PZ_VTRACE_VALUE_FLOAT32 == kValueFloat32 && PZ_VTRACE_VALUE_FLOAT16 == kValueFloat16 &&
                  PZ_VTRACE_VALUE_BFLOAT16 == kValueBfloat16,
              "pz_traj_scan.hpp: the value formats");

struct VtraceArgs {
    const void* rew_p1;
    const void* rew_p2;
    const uint8_t* term;
    const void* val_p1;
    const void* val_p2;
    const float* lpb_p1;
    const float* lpb_p2;
    const float* lpt_p1;
    const float* lpt_p2;
    float* vs_p1;
    float* vs_p2;
    float* pg_p1;
    float* pg_p2;
    int64_t n, rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch;
    int32_t k;
    float gamma, gl, clip_rho, clip_c, clip_pg;
};

// what a row's log-probs become before the scan reaches it: the clipped weights, the trace's already times gl
struct Weight {
    float rho, glc, pg;
};

// what a lane keeps over the whole scan: its column of every tensor, the pitches, the scalars, the two carried values
template <int RF, int VF>
struct Lane {
    using Raw = typename ValueRaw<VF>::type;
    // per buffer: 8 rewards, values, flags and 2 x 8 log-probs
    struct Chunk {
        uint32_t r[kChunk];
        Raw v[kChunk];
        uint8_t d[kChunk];
        float lpb[kChunk], lpt[kChunk];
    };
    const uint32_t* rew;
    const Raw* val;
    const uint8_t* term;
    const float* lpb;
    const float* lpt;
    float* vs;
    float* pg;
    int64_t rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch;
    float gamma, gl, clip_rho, clip_c, clip_pg;
    float v_next, acc_next;

    __device__ __forceinline__ Weight weigh(float b, float t) const
    {
        const float d = t - b;
        const float w = d == 0.0f ? 1.0f : expf(d);
        // selects, not a minimum: a NaN weight fails the comparison and stays
        const float rho = w > clip_rho ? clip_rho : w;
        const float c = w > clip_c ? clip_c : w;
        const float p = w > clip_pg ? clip_pg : w;
        return Weight{rho, gl * c, p};
    }

    __device__ __forceinline__ void scan(int64_t t, uint32_t r_bits, Raw v_bits, uint8_t d, const Weight w)
    {
        const bool nt = d == 0;
        const float r = reward_of<RF>(r_bits), v = value_of<VF>(v_bits);
        const float q = nt ? gamma * v_next : 0.0f;
        const float delta = (r + q) - v;
        const float acc = w.rho * delta + (nt ? w.glc * acc_next : 0.0f);
        __builtin_nontemporal_store(v + acc, vs + t * out_pitch);
        __builtin_nontemporal_store(w.pg * (delta + (nt ? gl * acc_next : 0.0f)), pg + t * out_pitch);
        acc_next = acc;
        v_next = v;
    }

    __device__ __forceinline__ void scan_row(int64_t t)
    {
        scan(t, rew[t * rew_pitch], val[t * val_pitch], term[t * term_pitch], weigh(lpb[t * lp_pitch], lpt[t * lp_pitch]));
    }

    __device__ __forceinline__ void load_chunk(int64_t t0, Chunk& c) const
    {
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            c.lpb[i] = lpb[(t0 + i) * lp_pitch];
            c.lpt[i] = lpt[(t0 + i) * lp_pitch];
            c.r[i] = rew[(t0 + i) * rew_pitch];
            c.v[i] = val[(t0 + i) * val_pitch];
            c.d[i] = term[(t0 + i) * term_pitch];
        }
    }

    __device__ __forceinline__ void scan_chunk(int64_t t0, const Chunk& c)
    {
        // the chunk's weights first: none of them waits for the scan
        Weight w[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) w[i] = weigh(c.lpb[i], c.lpt[i]);
#pragma unroll
        for (int i = kChunk - 1; i >= 0; --i) scan(t0 + i, c.r[i], c.v[i], c.d[i], w[i]);
    }
};

template <int RF, int VF>
__global__ void __launch_bounds__(kLanes) vtrace_kernel(const VtraceArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.n) return;
    const bool second = blockIdx.y != 0;
    Lane<RF, VF> s;
    s.rew = (const uint32_t*)(second ? a.rew_p2 : a.rew_p1) + g;
    s.val = (const typename Lane<RF, VF>::Raw*)(second ? a.val_p2 : a.val_p1) + g;
    s.term = a.term + g;
    s.lpb = (second ? a.lpb_p2 : a.lpb_p1) + g;
    s.lpt = (second ? a.lpt_p2 : a.lpt_p1) + g;
    s.vs = (second ? a.vs_p2 : a.vs_p1) + g;
    s.pg = (second ? a.pg_p2 : a.pg_p1) + g;
    s.rew_pitch = a.rew_pitch, s.term_pitch = a.term_pitch, s.val_pitch = a.val_pitch, s.lp_pitch = a.lp_pitch, s.out_pitch = a.out_pitch;
    s.gamma = a.gamma, s.gl = a.gl, s.clip_rho = a.clip_rho, s.clip_c = a.clip_c, s.clip_pg = a.clip_pg;
    s.v_next = value_of<VF>(s.val[a.k * s.val_pitch]);
    s.acc_next = 0.0f;
    scan_rows(s, a.k);
}

static bool clip_ok(float x) { return x >= 0.0f && x <= 3.402823466e38f; }  // finite and not negative

}  // namespace pz_vt

using namespace pz_vt;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kVtraceBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_vtrace_build_id(void) { return kVtraceBuildIdRecord + 12; }

int pz_vtrace_abi_version(void) { return PZ_VTRACE_ABI_VERSION; }

int pz_vtrace(const void* rew_p1, const void* rew_p2, int32_t reward_format, const uint8_t* terminated, const void* val_p1,
              const void* val_p2, int32_t value_format, const float* lpb_p1, const float* lpb_p2, const float* lpt_p1,
              const float* lpt_p2, int32_t k, int64_t n, int64_t rew_pitch, int64_t term_pitch, int64_t val_pitch,
              int64_t lp_pitch, int64_t out_pitch, float gamma, float lam, float clip_rho, float clip_c, float clip_pg_rho,
              float* vs_p1, float* vs_p2, float* pg_p1, float* pg_p2, void* stream)
{
    if (!rew_p1 || !terminated || !val_p1 || !lpb_p1 || !lpt_p1 || !vs_p1 || !pg_p1) return PZ_E_NULL;
    const int second = (rew_p2 != nullptr) + (val_p2 != nullptr) + (lpb_p2 != nullptr) + (lpt_p2 != nullptr) + (vs_p2 != nullptr) +
                       (pg_p2 != nullptr);
    if (second != 0 && second != 6) return PZ_E_NULL;  // agent 2: all six or none
    if (!sizes_fit(k, n, {rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch})) return PZ_E_SIZE;
    if (!known_formats(reward_format, value_format)) return PZ_E_CONFIG;
    if (!unit(gamma) || !unit(lam) || !clip_ok(clip_rho) || !clip_ok(clip_c) || !clip_ok(clip_pg_rho)) return PZ_E_CONFIG;
    const uintptr_t vb = value_bytes(value_format);
    if (misaligned(rew_p1, 4) || misaligned(rew_p2, 4) || misaligned(val_p1, vb) || misaligned(val_p2, vb) || misaligned(lpb_p1, 4) ||
        misaligned(lpb_p2, 4) || misaligned(lpt_p1, 4) || misaligned(lpt_p2, 4) || misaligned(vs_p1, 4) || misaligned(vs_p2, 4) ||
        misaligned(pg_p1, 4) || misaligned(pg_p2, 4))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const VtraceArgs a{rew_p1, rew_p2, terminated, val_p1,    val_p2,     lpb_p1,    lpb_p2,   lpt_p1,    lpt_p2, vs_p1,
                       vs_p2,  pg_p1,  pg_p2,      n,         rew_pitch,  term_pitch, val_pitch, lp_pitch,  out_pitch, k,
                       gamma,  gamma * lam, clip_rho, clip_c, clip_pg_rho};
    dispatch_formats(reward_format, value_format, [&](auto rf, auto vf) {
        hipLaunchKernelGGL((vtrace_kernel<decltype(rf)::value, decltype(vf)::value>), grid_of(n, second == 6), dim3(kLanes), 0,
                           (hipStream_t)stream, a);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
