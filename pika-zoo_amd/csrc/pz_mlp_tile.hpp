// The policy net's forward tile, shared by libpikazoo_net.so (pz_net.hip) and libpikazoo_pool.so (pz_pool.hip): the staging of
// one parameter set into LDS in operand order, the three layers of one tile of 32 batch rows, and what the two entry points
// check and size alike.  include/pikazoo_pool.h promises pz_mlp_forward's bits for every row: both kernels call tile_forward,
// so the k order, the operand permutation and the roundings are written down here and nowhere else.
// libpikazoo_act.so (pz_act.hip) shares the staging, the dense layer and the checks, and takes the layers without the store
// from tile_layers, below tile_forward.
//
// Every layer is computed as W . X^T on v_mfma_f32_32x32x2_f32 (exact float32: a k-ordered chain of fused multiply-adds):
// the weights are the A operand, a tile of 32 batch rows the B operand, so an accumulator tile has its hidden index in the
// 16 registers and its batch row on the lane:
//     D[i][j]: j = lane & 31 (the batch row), i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// The next layer sums over exactly that register index: register r of input tile `tin` IS the B operand of one k-step,
//     B[k = lane >> 5][j = lane & 31]  with  k -> hidden index 32 * tin + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5),
// with no lane movement and no LDS round trip.  The weight operand of that step has to come in the same permuted k order;
// the permutation is paid when the parameters are staged from torch's own [out, in] tensors into LDS in operand order: the A
// operand of (layer, k-step u, output tile t) is 64 consecutive floats, lane l reads float l.
// Pads (in_features up to a multiple of 8, out_features up to a multiple of 32) are zeros the staging writes itself; a lane
// whose row is not live, or whose column is >= in_features, loads nothing and feeds +0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_net.h"

namespace pz_mlp {

constexpr int kThreads = 256;  // four waves, one per SIMD, share one staged parameter set
constexpr int kWaves = kThreads / 64;
constexpr int kTileRows = 32;  // batch rows per wave and pass: the columns of one 32x32 tile
constexpr int kChunk = 4;      // k-steps of the first layer per group of observation loads (8 columns)
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kLdsBytes = 160 * 1024;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// floats of LDS: [layer 1: K8 * H][layer 2: H * H][layer 3: H * 32 * TO][b1: H][b2: H][b3: 32 * TO]
__host__ __device__ constexpr int k8_of(int K) { return (K + 7) & ~7; }
__host__ __device__ constexpr int out_tiles_of(int O) { return (O + 31) >> 5; }
__host__ __device__ constexpr int lds_floats(int K, int H, int O)
{
    return k8_of(K) * H + H * H + H * 32 * out_tiles_of(O) + 2 * H + 32 * out_tiles_of(O);
}

// the hidden (or output) index that register r of a tile holds in lane half h
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float load_obs(const void* p, int format, int64_t idx)
{
    switch (format) {
        case PZ_NET_OBS_INT32:
            return (float)((const int32_t*)p)[idx];  // (beyond 2^24: to nearest even)
        case PZ_NET_OBS_INT16:
            return (float)((const int16_t*)p)[idx];
        case PZ_NET_OBS_FLOAT32:
            return ((const float*)p)[idx];
        case PZ_NET_OBS_FLOAT16:
            return (float)((const _Float16*)p)[idx];
        default:
            return __uint_as_float((uint32_t)((const uint16_t*)p)[idx] << 16);  // bfloat16: the upper half of a float32
    }
}

// one rounding, to nearest even
__device__ __forceinline__ void store_out(void* p, int format, int64_t idx, float x)
{
    if (format == PZ_NET_OUT_FLOAT32) {
        ((float*)p)[idx] = x;
    } else if (format == PZ_NET_OUT_FLOAT16) {
        ((_Float16*)p)[idx] = (_Float16)x;
    } else {
        const uint32_t b = __float_as_uint(x);
        ((uint16_t*)p)[idx] = x != x ? (uint16_t)((b >> 16) | 0x40u) : (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
    }
}

template <int ACT>
__device__ __forceinline__ float activate(float z)
{
    if constexpr (ACT == PZ_NET_ACT_TANH)
        return tanhf(z);
    else
        return z < 0.0f ? 0.0f : z;  // (a NaN is not < 0: it stays)
}

// One weight matrix, global [rows, cols] row-major -> LDS in operand order, zero-padded to [32 * tiles_out, cols_pad], by the
// whole workgroup.  The matrix is walked in blocks of 8 rows x 8 columns, a wave taking one block per load: 8 segments of 32
// contiguous bytes (every workgroup of the launch reads the same 30 KB: a walk in LDS order, one row per lane, asks the L2
// for a line per lane and made the staging the longest part of the launch), 16 LDS banks per store (a 4-way conflict).
// kStageBatch loads of a thread are in flight before their stores.  PERMUTED: k is the register index of the previous
// layer's accumulator (layers 2 and 3); otherwise k-step s holds columns 2 s and 2 s + 1 (layer 1).
constexpr int kStageBatch = 8;

template <bool PERMUTED>
__device__ __forceinline__ void stage_matrix(float* dst, const float* w, int rows, int cols, int cols_pad, int tiles_out, int tid)
{
    const int col_blocks = cols_pad >> 3, total = 32 * tiles_out * cols_pad;
    for (int base = tid; base < total; base += kThreads * kStageBatch) {
        float v[kStageBatch];
        int at[kStageBatch];
#pragma unroll
        for (int j = 0; j < kStageBatch; ++j) {
            const int e = base + j * kThreads;
            const int blk = e >> 6, ib = blk / col_blocks, kb = blk - ib * col_blocks;
            const int i = 8 * ib + ((e >> 3) & 7), k = 8 * kb + (e & 7);
            const int t = i >> 5;
            int step, half;
            if constexpr (PERMUTED) {  // k = 32 tin + (r & 3) + 8 (r >> 2) + 4 half, step = 16 tin + r
                half = (k >> 2) & 1;
                step = 16 * (k >> 5) + (k & 3) + 4 * ((k & 31) >> 3);
            } else {
                half = k & 1;
                step = k >> 1;
            }
            at[j] = e < total ? (step * tiles_out + t) * 64 + 32 * half + (i & 31) : -1;
            v[j] = e < total && i < rows && k < cols ? w[i * cols + k] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kStageBatch; ++j)
            if (at[j] >= 0) dst[at[j]] = v[j];
    }
}

// where one staged parameter set lies in LDS
struct Staged {
    float *w1, *w2, *w3, *b1, *b2, *b3;
};

template <int H>
__device__ __forceinline__ Staged staged_at(float* lds, int K, int O)
{
    const int K8 = k8_of(K), TO = out_tiles_of(O);
    Staged s;
    s.w1 = lds;
    s.w2 = s.w1 + K8 * H;
    s.w3 = s.w2 + H * H;
    s.b1 = s.w3 + H * 32 * TO;
    s.b2 = s.b1 + H;
    s.b3 = s.b2 + H;
    return s;
}

// one parameter set, global -> LDS in operand order, by the whole workgroup (the caller puts the barriers around it)
template <int H>
__device__ __forceinline__ void stage_parameters(const Staged& s, const float* w1, const float* b1, const float* w2, const float* b2,
                                                 const float* w3, const float* b3, int K, int O, int tid)
{
    constexpr int TH = H / 32;
    const int K8 = k8_of(K), TO = out_tiles_of(O);
    stage_matrix<false>(s.w1, w1, H, K, K8, TH, tid);
    stage_matrix<true>(s.w2, w2, H, H, H, TH, tid);
    stage_matrix<true>(s.w3, w3, O, H, H, TO, tid);
    for (int d = tid; d < H; d += kThreads) {
        s.b1[d] = b1[d];
        s.b2[d] = b2[d];
    }
    for (int d = tid; d < 32 * TO; d += kThreads) s.b3[d] = d < O ? b3[d] : 0.0f;
}

// A layer whose input is the previous layer's accumulator tiles: register r of input tile tin is the B operand of k-step
// u = tin * 16 + r.  The A operands of kGroup steps are read one group ahead of the products that use them, and a scheduling
// barrier closes each group, so that the compiler keeps two groups of operands in registers and no more.
constexpr int kGroup = 4;

template <int TIN, int TOUT, int TACC>
__device__ __forceinline__ void dense(const f32x16 (&in)[TIN], const float* w, const float* bias, f32x16 (&acc)[TACC], int lane)
{
    constexpr int kGroups = TIN * 16 / kGroup;
    const int half = lane >> 5;
#pragma unroll
    for (int t = 0; t < TOUT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = bias[32 * t + acc_row(r, half)];
    float a[2][kGroup * TOUT];
#pragma unroll
    for (int e = 0; e < kGroup * TOUT; ++e) a[0][e] = w[e * 64 + lane];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        if (g + 1 < kGroups) {
#pragma unroll
            for (int e = 0; e < kGroup * TOUT; ++e) a[(g + 1) & 1][e] = w[((g + 1) * kGroup * TOUT + e) * 64 + lane];
        }
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            const int u = g * kGroup + j;
            const float b = in[u >> 4][u & 15];
#pragma unroll
            for (int t = 0; t < TOUT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g & 1][j * TOUT + t], b, acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The three layers of one tile: the wave's 32 batch rows, lane (row j = lane & 31, half h = lane >> 5) holding batch row `row`
// (both halves of a row agree on it).  A lane that is not `live` loads nothing, feeds +0 and stores nothing.
template <int H, int ACT>
__device__ __forceinline__ void tile_forward(const Staged& s, const void* obs, void* out, int64_t row, bool live, int K, int O, int64_t obs_pitch,
                                             int64_t out_pitch, int obs_format, int out_format, int lane)
{
    constexpr int TH = H / 32;
    const int half = lane >> 5, K8 = k8_of(K), TO = out_tiles_of(O);
    const float* lds1 = s.w1;
    const int chunks = K8 / (2 * kChunk);
    const int64_t obs_at = row * obs_pitch;
    // lane (row j, half h) feeds column 2 s + h of its row at k-step s
    auto load_chunk = [&](int c, float (&x)[kChunk]) {
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const int k = 2 * (kChunk * c + j) + half;
            x[j] = live && k < K ? load_obs(obs, obs_format, obs_at + k) : 0.0f;
        }
    };
    auto load_weights = [&](int c, float (&w)[kChunk * TH]) {
#pragma unroll
        for (int e = 0; e < kChunk * TH; ++e) w[e] = lds1[(c * kChunk * TH + e) * 64 + lane];
    };
    float x[kChunk], xn[kChunk] = {}, w[kChunk * TH], wn[kChunk * TH] = {};
    load_chunk(0, x);
    load_weights(0, w);

    // ---- layer 1 -------------------------------------------------------------------------------------------------------------
    f32x16 h1[TH];
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[t][r] = s.b1[32 * t + acc_row(r, half)];
    for (int c = 0; c < chunks; ++c) {
        if (c + 1 < chunks) {  // (in flight under this chunk's products)
            load_chunk(c + 1, xn);
            load_weights(c + 1, wn);
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
#pragma unroll
            for (int t = 0; t < TH; ++t) h1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j * TH + t], x[j], h1[t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) x[j] = xn[j];
#pragma unroll
        for (int e = 0; e < kChunk * TH; ++e) w[e] = wn[e];
    }
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[t][r] = activate<ACT>(h1[t][r]);

    // ---- layer 2 -------------------------------------------------------------------------------------------------------------
    f32x16 h2[TH];
    dense<TH, TH, TH>(h1, s.w2, s.b2, h2, lane);
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[t][r] = activate<ACT>(h2[t][r]);

    // ---- layer 3 and the store -----------------------------------------------------------------------------------------------
    f32x16 y[2];
    if (TO == 1)
        dense<TH, 1, 2>(h2, s.w3, s.b3, y, lane);
    else
        dense<TH, 2, 2>(h2, s.w3, s.b3, y, lane);
    if (live) {
        const int64_t out_at = row * out_pitch;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * t + acc_row(r, half);
                if (o < O) store_out(out, out_format, out_at + o, y[t][r]);
            }
    }
}

// tile_forward's three layers ONCE MORE, without the store, for libpikazoo_act.so (pz_act.hip), which goes on from the head in
// registers: output o = 32 t + acc_row(r, half) of the lane's row comes back as y[t][r].  It stands beside tile_forward rather
// than under it because a tile_forward that called it compiled pz_net.hip's and pz_pool.hip's kernels to other instruction
// streams (the same arithmetic, scheduled differently), and those kernels keep theirs.  The two texts must stay
// line for line alike from load_chunk to the layer-3 dense: include/pikazoo_act.h promises pz_mlp_forward's bits, and
// tests/test_gpu_act.py holds the two to each other.
template <int H, int ACT>
__device__ __forceinline__ void tile_layers(const Staged& s, const void* obs, int64_t row, bool live, int K, int O, int64_t obs_pitch,
                                            int obs_format, int lane, f32x16 (&y)[2])
{
    constexpr int TH = H / 32;
    const int half = lane >> 5, K8 = k8_of(K), TO = out_tiles_of(O);
    const float* lds1 = s.w1;
    const int chunks = K8 / (2 * kChunk);
    const int64_t obs_at = row * obs_pitch;
    auto load_chunk = [&](int c, float (&x)[kChunk]) {
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const int k = 2 * (kChunk * c + j) + half;
            x[j] = live && k < K ? load_obs(obs, obs_format, obs_at + k) : 0.0f;
        }
    };
    auto load_weights = [&](int c, float (&w)[kChunk * TH]) {
#pragma unroll
        for (int e = 0; e < kChunk * TH; ++e) w[e] = lds1[(c * kChunk * TH + e) * 64 + lane];
    };
    float x[kChunk], xn[kChunk] = {}, w[kChunk * TH], wn[kChunk * TH] = {};
    load_chunk(0, x);
    load_weights(0, w);

    f32x16 h1[TH];
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[t][r] = s.b1[32 * t + acc_row(r, half)];
    for (int c = 0; c < chunks; ++c) {
        if (c + 1 < chunks) {
            load_chunk(c + 1, xn);
            load_weights(c + 1, wn);
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
#pragma unroll
            for (int t = 0; t < TH; ++t) h1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j * TH + t], x[j], h1[t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) x[j] = xn[j];
#pragma unroll
        for (int e = 0; e < kChunk * TH; ++e) w[e] = wn[e];
    }
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[t][r] = activate<ACT>(h1[t][r]);

    f32x16 h2[TH];
    dense<TH, TH, TH>(h1, s.w2, s.b2, h2, lane);
#pragma unroll
    for (int t = 0; t < TH; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[t][r] = activate<ACT>(h2[t][r]);

    if (TO == 1)
        dense<TH, 1, 2>(h2, s.w3, s.b3, y, lane);
    else
        dense<TH, 2, 2>(h2, s.w3, s.b3, y, lane);
}

// a live lane's share of its float32 row, from tile_layers' accumulators: what tile_forward stores at PZ_NET_OUT_FLOAT32
__device__ __forceinline__ void store_tile_float32(const f32x16 (&y)[2], float* out, int64_t row, bool live, int O, int64_t out_pitch, int lane)
{
    const int half = lane >> 5;
    if (live) {
        const int64_t out_at = row * out_pitch;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * t + acc_row(r, half);
                if (o < O) out[out_at + o] = y[t][r];
            }
    }
}

static inline bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static inline bool bad_pitch(int64_t n, int64_t width, int64_t pitch)
{
    if (pitch < width) return true;
    return n > 0 && pitch > (INT64_MAX / 4) / n;  // n * pitch * 4 bytes: refused, never wrapped
}

// The most workgroups a launch of `sides` agents asks for: two resident workgroups per CU where the LDS holds two parameter
// sets (the loads of one hide under the other's products), else one, divided over the sides.
static inline int64_t grid_cap(size_t lds_bytes, unsigned sides)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    const int64_t resident = (int64_t)cus * (2 * lds_bytes <= (size_t)kLdsBytes ? 2 : 1);
    return (resident + sides - 1) / sides;
}

}  // namespace pz_mlp
