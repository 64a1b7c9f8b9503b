// libpikazoo_vtrace.so (include/pikazoo_vtrace.h): V-trace targets over the [k, N] trajectory tensors of a k-step launch.
//
// The shape is pz_learn.hip's, the right one for a serial scan: one lane per game, blockIdx.y = agent, one wave (64
// consecutive games) per workgroup, so every row access of a wave is one coalesced segment.  Five input streams per agent
// (reward, value, flag, behaviour and target log-prob) are loaded a chunk of kChunk rows ahead into a second register buffer:
// the wave waits on vmcnt for the chunk it scans while the next one is in flight.  What does not depend on the scan -- the
// expf of the log-ratio, the three selects against the clips and the product gl * c -- is computed for the whole chunk AHEAD of
// the serial chain (scan_chunk's first loop), so the dependent chain per row stays one multiply and one add.  The rows above
// the last multiple of kChunk are scanned first, one by one.  Stores are non-temporal and never waited for.
//
// kChunk = 8: 5 registers per row and buffer make 80 VGPRs of staging, the chunk's 24 weights take the place of its 16
// log-probs; with addresses and pitches the six kernels come to 109 .. 121 VGPRs, no scratch: 4 waves per SIMD, where 65 536
// games of both agents fill 2.  A chunk of 16 would not fit 128 registers and would halve that.
//
// The formats are compile-time instantiations (2 reward x 3 value formats = 6 kernels); the arithmetic is the same text
// for all of them.  No multiply-add may be contracted: the pragma below holds for the whole translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_vtrace.h"

#pragma clang fp contract(off)

namespace pz_vt {

constexpr int kLanes = 64;  // games per workgroup: one wave
constexpr int kChunk = 8;   // rows loaded ahead of the scan (per buffer: 8 rewards, values, flags and 2 x 8 log-probs)

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

// a reward row element is 4 bytes in both formats: loaded as its bits, converted where it is used
template <int RF>
__device__ __forceinline__ float reward_of(uint32_t bits)
{
    return RF == PZ_VTRACE_REWARD_INT32 ? (float)(int32_t)bits : __uint_as_float(bits);
}

template <int VF>
struct ValueRaw {
    using type = uint16_t;
};
template <>
struct ValueRaw<PZ_VTRACE_VALUE_FLOAT32> {
    using type = uint32_t;
};

template <int VF>
__device__ __forceinline__ float value_of(typename ValueRaw<VF>::type bits)
{
    if constexpr (VF == PZ_VTRACE_VALUE_FLOAT32)
        return __uint_as_float(bits);
    else if constexpr (VF == PZ_VTRACE_VALUE_FLOAT16)
        return (float)__builtin_bit_cast(_Float16, bits);  // exact
    else
        return __uint_as_float((uint32_t)bits << 16);  // bfloat16 is the upper half of a float32: exact
}

template <int VF>
struct Chunk {
    uint32_t r[kChunk];
    typename ValueRaw<VF>::type v[kChunk];
    uint8_t d[kChunk];
    float lpb[kChunk], lpt[kChunk];
};

// what a row's log-probs become before the scan reaches it: the clipped weights, the trace's already times gl
struct Weight {
    float rho, glc, pg;
};

// what a lane keeps over the whole scan: its column of every tensor, the pitches, the scalars, the two carried values
template <int VF>
struct Lane {
    const uint32_t* rew;
    const typename ValueRaw<VF>::type* val;
    const uint8_t* term;
    const float* lpb;
    const float* lpt;
    float* vs;
    float* pg;
    int64_t rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch;
    float gamma, gl, clip_rho, clip_c, clip_pg;
    float v_next, acc_next;
};

template <int VF>
__device__ __forceinline__ Weight weigh(const Lane<VF>& s, float lpb, float lpt)
{
    const float d = lpt - lpb;
    const float w = d == 0.0f ? 1.0f : expf(d);
    // selects, not a minimum: a NaN weight fails the comparison and stays
    const float rho = w > s.clip_rho ? s.clip_rho : w;
    const float c = w > s.clip_c ? s.clip_c : w;
    const float pg = w > s.clip_pg ? s.clip_pg : w;
    return Weight{rho, s.gl * c, pg};
}

template <int RF, int VF>
__device__ __forceinline__ void scan_row(Lane<VF>& s, int64_t t, uint32_t r_bits, typename ValueRaw<VF>::type v_bits, uint8_t d,
                                         const Weight w)
{
    const bool nt = d == 0;
    const float r = reward_of<RF>(r_bits), v = value_of<VF>(v_bits);
    const float q = nt ? s.gamma * s.v_next : 0.0f;
    const float delta = (r + q) - v;
    const float acc = w.rho * delta + (nt ? w.glc * s.acc_next : 0.0f);
    __builtin_nontemporal_store(v + acc, s.vs + t * s.out_pitch);
    __builtin_nontemporal_store(w.pg * (delta + (nt ? s.gl * s.acc_next : 0.0f)), s.pg + t * s.out_pitch);
    s.acc_next = acc;
    s.v_next = v;
}

template <int VF>
__device__ __forceinline__ void load_chunk(const Lane<VF>& s, int64_t t0, Chunk<VF>& c)
{
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
        c.lpb[i] = s.lpb[(t0 + i) * s.lp_pitch];
        c.lpt[i] = s.lpt[(t0 + i) * s.lp_pitch];
        c.r[i] = s.rew[(t0 + i) * s.rew_pitch];
        c.v[i] = s.val[(t0 + i) * s.val_pitch];
        c.d[i] = s.term[(t0 + i) * s.term_pitch];
    }
}

template <int RF, int VF>
__device__ __forceinline__ void scan_chunk(Lane<VF>& s, int64_t t0, const Chunk<VF>& c)
{
    // the chunk's weights first: none of them waits for the scan
    Weight w[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) w[i] = weigh<VF>(s, c.lpb[i], c.lpt[i]);
#pragma unroll
    for (int i = kChunk - 1; i >= 0; --i) scan_row<RF, VF>(s, t0 + i, c.r[i], c.v[i], c.d[i], w[i]);
}

template <int RF, int VF>
__global__ void __launch_bounds__(kLanes) vtrace_kernel(const VtraceArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.n) return;
    const bool second = blockIdx.y != 0;
    using V = typename ValueRaw<VF>::type;
    Lane<VF> s;
    s.rew = (const uint32_t*)(second ? a.rew_p2 : a.rew_p1) + g;
    s.val = (const V*)(second ? a.val_p2 : a.val_p1) + g;
    s.term = a.term + g;
    s.lpb = (second ? a.lpb_p2 : a.lpb_p1) + g;
    s.lpt = (second ? a.lpt_p2 : a.lpt_p1) + g;
    s.vs = (second ? a.vs_p2 : a.vs_p1) + g;
    s.pg = (second ? a.pg_p2 : a.pg_p1) + g;
    s.rew_pitch = a.rew_pitch, s.term_pitch = a.term_pitch, s.val_pitch = a.val_pitch, s.lp_pitch = a.lp_pitch, s.out_pitch = a.out_pitch;
    s.gamma = a.gamma, s.gl = a.gl, s.clip_rho = a.clip_rho, s.clip_c = a.clip_c, s.clip_pg = a.clip_pg;
    int64_t t = a.k;  // rows [0, t) are still to scan
    s.v_next = value_of<VF>(s.val[t * s.val_pitch]);
    s.acc_next = 0.0f;
    // the rows above the last multiple of kChunk, one by one
    for (int rest = a.k % kChunk; rest > 0; --rest) {
        --t;
        scan_row<RF, VF>(s, t, s.rew[t * s.rew_pitch], s.val[t * s.val_pitch], s.term[t * s.term_pitch],
                         weigh<VF>(s, s.lpb[t * s.lp_pitch], s.lpt[t * s.lp_pitch]));
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
static void launch(const VtraceArgs& a, bool both, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.n + kLanes - 1) / kLanes), both ? 2 : 1);
    hipLaunchKernelGGL((vtrace_kernel<RF, VF>), grid, dim3(kLanes), 0, stream, a);
}

template <int RF>
static void launch_values(int value_format, const VtraceArgs& a, bool both, hipStream_t stream)
{
    switch (value_format) {
        case PZ_VTRACE_VALUE_FLOAT32: launch<RF, PZ_VTRACE_VALUE_FLOAT32>(a, both, stream); break;
        case PZ_VTRACE_VALUE_FLOAT16: launch<RF, PZ_VTRACE_VALUE_FLOAT16>(a, both, stream); break;
        default: launch<RF, PZ_VTRACE_VALUE_BFLOAT16>(a, both, stream); break;
    }
}

static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static bool unit(float x) { return x >= 0.0f && x <= 1.0f; }          // (a NaN fails both)
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
    if (k < 1 || n < 0) return PZ_E_SIZE;
    if (rew_pitch < n || term_pitch < n || val_pitch < n || lp_pitch < n || out_pitch < n) return PZ_E_SIZE;
    // the kernel's addressing: a game index and a grid in 32 bits, byte offsets of up to k + 1 rows of 4-byte elements in int64
    if (n > ((int64_t)1 << 30)) return PZ_E_SIZE;
    const int64_t most = (INT64_MAX / 4) / ((int64_t)k + 1);
    if (rew_pitch > most || term_pitch > most || val_pitch > most || lp_pitch > most || out_pitch > most) return PZ_E_SIZE;
    if (reward_format != PZ_VTRACE_REWARD_INT32 && reward_format != PZ_VTRACE_REWARD_FLOAT32) return PZ_E_CONFIG;
    if (value_format != PZ_VTRACE_VALUE_FLOAT32 && value_format != PZ_VTRACE_VALUE_FLOAT16 && value_format != PZ_VTRACE_VALUE_BFLOAT16)
        return PZ_E_CONFIG;
    if (!unit(gamma) || !unit(lam) || !clip_ok(clip_rho) || !clip_ok(clip_c) || !clip_ok(clip_pg_rho)) return PZ_E_CONFIG;
    const uintptr_t value_bytes = value_format == PZ_VTRACE_VALUE_FLOAT32 ? 4 : 2;
    if (misaligned(rew_p1, 4) || misaligned(rew_p2, 4) || misaligned(val_p1, value_bytes) || misaligned(val_p2, value_bytes) ||
        misaligned(lpb_p1, 4) || misaligned(lpb_p2, 4) || misaligned(lpt_p1, 4) || misaligned(lpt_p2, 4) || misaligned(vs_p1, 4) ||
        misaligned(vs_p2, 4) || misaligned(pg_p1, 4) || misaligned(pg_p2, 4))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const VtraceArgs a{rew_p1, rew_p2, terminated, val_p1,    val_p2,     lpb_p1,    lpb_p2,   lpt_p1,    lpt_p2, vs_p1,
                       vs_p2,  pg_p1,  pg_p2,      n,         rew_pitch,  term_pitch, val_pitch, lp_pitch,  out_pitch, k,
                       gamma,  gamma * lam, clip_rho, clip_c, clip_pg_rho};
    if (reward_format == PZ_VTRACE_REWARD_INT32)
        launch_values<PZ_VTRACE_REWARD_INT32>(value_format, a, second == 6, (hipStream_t)stream);
    else
        launch_values<PZ_VTRACE_REWARD_FLOAT32>(value_format, a, second == 6, (hipStream_t)stream);
    return (int)hipGetLastError();
}

}  // extern "C"
