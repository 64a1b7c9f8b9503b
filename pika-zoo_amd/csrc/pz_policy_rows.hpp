// The logit rows of the categorical head, shared by the translation units that read them (pz_policy.hip, pz_ppo.hip,
// pz_act.hip): the element formats, a wave's span staged into its transposed LDS image, the row statistics every kernel of
// these libraries runs as this one text (the log-prob and entropy bits two launches must share come from here), the Philox
// block and the uniform draw (pz_sample_actions' and pz_mlp_act's alike), steps 4 and 5 as pz_act.hip runs them, the action
// read, and the dense store of a gradient image.  pz_policy.hip describes the layout and why it is what it is.
#ifndef PZ_POLICY_ROWS_HPP
#define PZ_POLICY_ROWS_HPP
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_policy.h"

namespace pz_policy {

constexpr int kLanes = 64;            // games per workgroup: one wave
constexpr int kMaxActions = 32;
constexpr int kMaxStride = kMaxActions | 1;  // dwords per row of the LDS image, at most
constexpr int kMaxStagedPitch = 64;   // above it the live columns are gathered instead of the span staged
constexpr int kDivShift = 20;         // idx / d == (idx * ceil(2^20 / d)) >> 20 for idx < 64 * 64 + 8, 2 <= d <= 64

struct Common {
    const void* logits[2];
    const void* act[2];  // (written by the sample launch)
    float* logp[2];
    float* ent[2];
    int64_t n, pitch;
    int32_t A, action_format;
    uint32_t pitch_magic, a_magic;  // ceil(2^20 / pitch) (0 when the pitch is gathered), ceil(2^20 / A)
};

template <int LF>
struct Raw {
    using type = uint16_t;
};
template <>
struct Raw<PZ_POLICY_LOGIT_FLOAT32> {
    using type = uint32_t;
};

template <int LF>
__device__ __forceinline__ float to_float(typename Raw<LF>::type bits)
{
    if constexpr (LF == PZ_POLICY_LOGIT_FLOAT32)
        return __uint_as_float(bits);
    else if constexpr (LF == PZ_POLICY_LOGIT_FLOAT16)
        return (float)__builtin_bit_cast(_Float16, bits);  // exact
    else
        return __uint_as_float((uint32_t)bits << 16);  // bfloat16 is the upper half of a float32: exact
}

// round to nearest even into the logits' own format
template <int LF>
__device__ __forceinline__ typename Raw<LF>::type from_float(float x)
{
    if constexpr (LF == PZ_POLICY_LOGIT_FLOAT32) {
        return __float_as_uint(x);
    } else if constexpr (LF == PZ_POLICY_LOGIT_FLOAT16) {
        return __builtin_bit_cast(uint16_t, (_Float16)x);
    } else {
        const uint32_t b = __float_as_uint(x);
        if (x != x) return (uint16_t)((b >> 16) | 0x40u);  // a NaN stays one
        return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
    }
}

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

// element j of a 16-byte piece
template <int LF>
__device__ __forceinline__ typename Raw<LF>::type piece_element(const u32x4& v, int j)
{
    if constexpr (LF == PZ_POLICY_LOGIT_FLOAT32)
        return v[j];
    else
        return (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
}

// ---- global -> LDS: the wave's span, transposed -------------------------------------------------------------------------
// `span`: the first element of the wave's first row; `len` = (rows - 1) * pitch + A elements.  image[row * stride + col]
// receives every element with col < A as a float32.
template <int LF>
__device__ __forceinline__ void stage_span(const typename Raw<LF>::type* span, int len, int pitch, uint32_t magic, int A, int stride,
                                           float* image, int lane)
{
    using R = typename Raw<LF>::type;
    constexpr int E = 16 / (int)sizeof(R);       // elements per piece
    constexpr int kGroup = sizeof(R) == 4 ? 5 : 3;  // pieces per lane in flight: one group covers 64 rows at pitch 19 (20)
    const int mis = (int)(((uintptr_t)span & 15) / sizeof(R));   // elements between the 16-byte boundary below and `span`
    const int head = mis ? min(E - mis, len) : 0;               // elements in front of the first whole piece
    const int pieces = (len - head) / E;                         // whole pieces
    const int tail = len - head - pieces * E;                    // elements behind the last whole piece
    auto put = [&](int idx, R bits) {
        const int row = (int)(((uint32_t)idx * magic) >> kDivShift), col = idx - row * pitch;
        if (col < A) image[row * stride + col] = to_float<LF>(bits);
    };
    // the peeled ends: lanes 0 .. head-1 and 32 .. 32+tail-1, one element each (head, tail < E <= 8)
    if (lane < head) put(lane, span[lane]);
    if (lane >= 32 && lane - 32 < tail) put(head + pieces * E + lane - 32, span[head + pieces * E + lane - 32]);
    const u32x4* body = (const u32x4*)(span + head);  // 16-byte aligned
    for (int p0 = 0; p0 < pieces; p0 += kGroup * kLanes) {
        u32x4 v[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) v[k] = body[min(p0 + k * kLanes + lane, pieces - 1)];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const int p = p0 + k * kLanes + lane;
            if (p < pieces) {
#pragma unroll
                for (int j = 0; j < E; ++j) put(head + p * E + j, piece_element<LF>(v[k], j));
            }
        }
    }
}

// the same image from a wide pitch: 64 consecutive (row, column < A) pairs per load instruction
template <int LF>
__device__ __forceinline__ void gather_rows(const typename Raw<LF>::type* span, int rows, int64_t pitch, uint32_t a_magic, int A,
                                            int stride, float* image, int lane)
{
    const int count = rows * A;
#pragma unroll 4
    for (int e = lane; e < count; e += kLanes) {
        const int row = (int)(((uint32_t)e * a_magic) >> kDivShift), col = e - row * A;
        image[row * stride + col] = to_float<LF>(span[row * pitch + col]);
    }
}

template <int LF>
__device__ __forceinline__ void load_image(const Common& c, int side, int64_t g0, int rows, int stride, float* image, int lane)
{
    using R = typename Raw<LF>::type;
    const R* span = (const R*)c.logits[side] + g0 * c.pitch;
    if (c.pitch <= kMaxStagedPitch)
        stage_span<LF>(span, (rows - 1) * (int)c.pitch + c.A, (int)c.pitch, c.pitch_magic, c.A, stride, image, lane);
    else
        gather_rows<LF>(span, rows, c.pitch, c.a_magic, c.A, stride, image, lane);
    __syncthreads();  // (one wave: no s_barrier, the LDS writes are waited for)
}

// ---- the row ------------------------------------------------------------------------------------------------------------
struct RowStats {
    float m, S, logS, H;
    int last;  // the last index with e_i > 0
    bool bad;  // step 6 of the header: a NaN, a +inf, or no finite logit
};

// steps 1, 2 and the entropy of step 5; every kernel runs exactly this text
__device__ __forceinline__ RowStats row_stats(const float* row, int A)
{
    RowStats s;
    float m = -INFINITY;
    bool bad = false;
    for (int i = 0; i < A; ++i) {
        const float l = row[i];
        bad |= !(l < INFINITY);  // NaN or +inf
        m = fmaxf(m, l);
    }
    bad |= m == -INFINITY;
    float c = 0.0f, t = 0.0f;
    int last = 0;
    for (int i = 0; i < A; ++i) {
        const float d = row[i] - m;
        const float e = expf(d);
        c += e;
        if (e > 0.0f) {
            t = fmaf(e, d, t);
            last = i;
        }
    }
    s.m = m, s.S = c, s.logS = logf(c), s.last = last, s.bad = bad;
    s.H = s.logS - t / c;
    return s;
}

// Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t& o0,
                                              uint32_t& o1)
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
    o0 = c0;
    o1 = c1;
}

// step 3: the uniform draw of global game G at step T for agent `side`
__device__ __forceinline__ float draw_uniform(uint64_t G, uint64_t T, uint32_t key0, uint32_t key1, int side)
{
    uint32_t w0, w1;
    philox4x32_10((uint32_t)G, (uint32_t)(G >> 32), (uint32_t)T, 2u + 4u * (uint32_t)(T >> 32), key0, key1, w0, w1);
    return (float)((side ? w1 : w0) >> 8) * 0x1p-24f;
}

// Steps 4 and 5 as pz_act.hip runs them: sample_kernel's and finish's own lines of pz_policy.hip once more.  Those two keep
// their text where it is, because calling these functions from them moved their kernels' instruction streams (DESIGN.md
// 4.23); the expressions must stay alike, and tests/test_gpu_act.py holds the two launches to each other bit for bit.
// step 4: the same sums again (the same expf of the same arguments: the same c_i), counted against the threshold
__device__ __forceinline__ int draw_action(const float* row, int A, const RowStats& s, float u)
{
    const float thr = u * s.S;
    float cum = 0.0f;
    int act = 0;
    for (int i = 0; i < A - 1; ++i) {
        cum += expf(row[i] - s.m);
        act += cum <= thr;
    }
    return s.bad ? 0 : min(act, s.last);
}

// step 5's log-prob of action a (NaN for a row of step 6 or an action outside [0, A))
__device__ __forceinline__ float action_log_prob(const float* row, int A, const RowStats& s, int a)
{
    const bool in_range = (unsigned)a < (unsigned)A;
    const float la = row[in_range ? a : 0];
    const float nan = __uint_as_float(0x7FC00000u);
    const float logp = (la - s.m) - s.logS;
    return (s.bad || !in_range) ? nan : logp;
}

__device__ __forceinline__ int load_action(const void* act, int format, int64_t g)
{
    if (format == PZ_POLICY_ACTION_INT32) return ((const int32_t*)act)[g];
    const int64_t a = ((const int64_t*)act)[g];
    return a == (int32_t)a ? (int32_t)a : -1;  // (beyond int32: out of range either way)
}

// ---- LDS -> global: the gradient rows, transposed back --------------------------------------------------------------------
// dense rows (grad_pitch == A): the span of rows * A elements in 16-byte pieces, the ends peeled as in stage_span
template <int LF>
__device__ __forceinline__ void store_dense(typename Raw<LF>::type* span, int len, int A, uint32_t magic, int stride, const float* image,
                                            int lane)
{
    using R = typename Raw<LF>::type;
    constexpr int E = 16 / (int)sizeof(R);
    const int mis = (int)(((uintptr_t)span & 15) / sizeof(R));
    const int head = mis ? min(E - mis, len) : 0;
    const int pieces = (len - head) / E;
    const int tail = len - head - pieces * E;
    auto get = [&](int idx) {
        const int row = (int)(((uint32_t)idx * magic) >> kDivShift), col = idx - row * A;
        return from_float<LF>(image[row * stride + col]);
    };
    if (lane < head) span[lane] = get(lane);
    if (lane >= 32 && lane - 32 < tail) span[head + pieces * E + lane - 32] = get(head + pieces * E + lane - 32);
    u32x4* body = (u32x4*)(span + head);
    for (int p = lane; p < pieces; p += kLanes) {
        u32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (sizeof(R) == 4)
                v[j] = get(head + p * E + j);
            else
                v[j] = (uint32_t)get(head + p * E + 2 * j) | ((uint32_t)get(head + p * E + 2 * j + 1) << 16);
        }
        body[p] = v;
    }
}

// ---- host side: what every entry point checks ----------------------------------------------------------------------------
static uint32_t magic_of(int64_t d) { return (uint32_t)((((int64_t)1 << kDivShift) + d - 1) / d); }

static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static bool known_logit_format(int f)
{
    return f == PZ_POLICY_LOGIT_FLOAT32 || f == PZ_POLICY_LOGIT_FLOAT16 || f == PZ_POLICY_LOGIT_BFLOAT16;
}

static bool known_action_format(int f) { return f == PZ_POLICY_ACTION_INT32 || f == PZ_POLICY_ACTION_INT64; }

// agent 2's pointer is there exactly where agent 1's is, if agent 2 is there at all
static bool paired(const void* p1, const void* p2, bool both) { return (p2 != nullptr) == (both && p1 != nullptr); }

static bool bad_sizes(int32_t A, int64_t n, int64_t pitch)
{
    if (n < 0 || n > ((int64_t)1 << 30)) return true;
    if (A < 2 || A > kMaxActions || pitch < A) return true;
    return n > 0 && pitch > (INT64_MAX / 4) / n;  // n * pitch * 4 bytes: refused, never wrapped
}

}  // namespace pz_policy

#endif  // PZ_POLICY_ROWS_HPP
