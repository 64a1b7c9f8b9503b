// libpikazoo_net.so: the forward pass of the three-layer policy net in ONE launch (C ABI and the definition:
// include/pikazoo_net.h; the shape and its reasons: DESIGN.md 4.17).
//
// Every layer is computed as W . X^T on v_mfma_f32_32x32x2_f32 (exact float32: a k-ordered chain of fused multiply-adds):
// the weights are the A operand, a tile of 32 batch rows the B operand, so an accumulator tile has its hidden index in the
// 16 registers and its batch row on the lane:
//     D[i][j]: j = lane & 31 (the batch row), i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// The next layer sums over exactly that register index: register r of input tile `tin` IS the B operand of one k-step,
//     B[k = lane >> 5][j = lane & 31]  with  k -> hidden index 32 * tin + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5),
// with no lane movement and no LDS round trip.  The weight operand of that step has to come in the same permuted k order;
// the permutation is paid once per workgroup, when the parameters are staged from torch's own [out, in] tensors into LDS
// in operand order: the A operand of (layer, k-step u, output tile t) is 64 consecutive floats, lane l reads float l.
// Pads (in_features up to a multiple of 8, out_features up to a multiple of 32) are zeros the staging writes itself; a lane
// whose row is >= n, or whose column is >= in_features, loads nothing and feeds +0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_net.h"

namespace pz_net {

constexpr int kThreads = 256;  // four waves, one per SIMD, share one staged parameter set
constexpr int kWaves = kThreads / 64;
constexpr int kTileRows = 32;  // batch rows per wave and pass: the columns of one 32x32 tile
constexpr int kChunk = 4;      // k-steps of the first layer per group of observation loads (8 columns)
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kLdsBytes = 160 * 1024;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Args {
    const void* obs[2];
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
    const float* w3[2];
    const float* b3[2];
    void* out[2];
    int64_t n, obs_pitch, out_pitch, tiles;
    int32_t K, O, obs_format, out_format;
};

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

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_forward_kernel(const Args a)
{
    constexpr int TH = H / 32;
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int K = a.K, O = a.O, K8 = k8_of(K), TO = out_tiles_of(O);
    float* lds1 = lds;
    float* lds2 = lds1 + K8 * H;
    float* lds3 = lds2 + H * H;
    float* bias1 = lds3 + H * 32 * TO;
    float* bias2 = bias1 + H;
    float* bias3 = bias2 + H;

    // ---- the parameters, global -> LDS in operand order, once per workgroup --------------------------------------------
    {
        stage_matrix<false>(lds1, a.w1[side], H, K, K8, TH, tid);
        stage_matrix<true>(lds2, a.w2[side], H, H, H, TH, tid);
        stage_matrix<true>(lds3, a.w3[side], O, H, H, TO, tid);
        for (int d = tid; d < H; d += kThreads) {
            bias1[d] = a.b1[side][d];
            bias2[d] = a.b2[side][d];
        }
        for (int d = tid; d < 32 * TO; d += kThreads) bias3[d] = d < O ? a.b3[side][d] : 0.0f;
    }
    __syncthreads();

    const void* obs = a.obs[side];
    void* out = a.out[side];
    const int chunks = K8 / (2 * kChunk);
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < a.tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t row = tile * kTileRows + (lane & 31);
        const bool live = row < a.n;
        const int64_t obs_at = row * a.obs_pitch;
        // lane (row j, half h) feeds column 2 s + h of its row at k-step s
        auto load_chunk = [&](int c, float (&x)[kChunk]) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int k = 2 * (kChunk * c + j) + half;
                x[j] = live && k < K ? load_obs(obs, a.obs_format, obs_at + k) : 0.0f;
            }
        };
        auto load_weights = [&](int c, float (&w)[kChunk * TH]) {
#pragma unroll
            for (int e = 0; e < kChunk * TH; ++e) w[e] = lds1[(c * kChunk * TH + e) * 64 + lane];
        };
        float x[kChunk], xn[kChunk] = {}, w[kChunk * TH], wn[kChunk * TH] = {};
        load_chunk(0, x);
        load_weights(0, w);

        // ---- layer 1 ---------------------------------------------------------------------------------------------------------
        f32x16 h1[TH];
#pragma unroll
        for (int t = 0; t < TH; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[t][r] = bias1[32 * t + acc_row(r, half)];
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

        // ---- layer 2 ---------------------------------------------------------------------------------------------------------
        f32x16 h2[TH];
        dense<TH, TH, TH>(h1, lds2, bias2, h2, lane);
#pragma unroll
        for (int t = 0; t < TH; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[t][r] = activate<ACT>(h2[t][r]);

        // ---- layer 3 and the store -------------------------------------------------------------------------------------------
        f32x16 y[2];
        if (TO == 1)
            dense<TH, 1, 2>(h2, lds3, bias3, y, lane);
        else
            dense<TH, 2, 2>(h2, lds3, bias3, y, lane);
        if (live) {
            const int64_t out_at = row * a.out_pitch;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = 32 * t + acc_row(r, half);
                    if (o < O) store_out(out, a.out_format, out_at + o, y[t][r]);
                }
        }
    }
}

static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static bool bad_pitch(int64_t n, int64_t width, int64_t pitch)
{
    if (pitch < width) return true;
    return n > 0 && pitch > (INT64_MAX / 4) / n;  // n * pitch * 4 bytes: refused, never wrapped
}

template <int H, int ACT>
static int launch(const Args& a, unsigned sides, void* stream)
{
    const size_t bytes = (size_t)lds_floats(a.K, H, a.O) * sizeof(float);
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_forward_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    // two resident workgroups per CU where the LDS holds two parameter sets: the loads of one hide under the other's products
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    const int64_t resident = (int64_t)cus * (2 * bytes <= (size_t)kLdsBytes ? 2 : 1);
    int64_t blocks = (a.tiles + kWaves - 1) / kWaves;
    const int64_t cap = (resident + sides - 1) / sides;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((mlp_forward_kernel<H, ACT>), dim3((unsigned)blocks, sides), dim3(kThreads), bytes, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

template <int ACT>
static int launch_hidden(const Args& a, int hidden, unsigned sides, void* stream)
{
    switch (hidden) {
        case 32:
            return launch<32, ACT>(a, sides, stream);
        case 64:
            return launch<64, ACT>(a, sides, stream);
        default:
            return launch<128, ACT>(a, sides, stream);
    }
}

}  // namespace pz_net

using namespace pz_net;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kNetBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_net_build_id(void) { return kNetBuildIdRecord + 12; }

int pz_net_abi_version(void) { return PZ_NET_ABI_VERSION; }

int pz_mlp_forward(const void* obs_p1, const void* obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch,
                   int32_t hidden, int32_t out_features, int32_t activation, const float* w1_p1, const float* b1_p1,
                   const float* w2_p1, const float* b2_p1, const float* w3_p1, const float* b3_p1, const float* w1_p2,
                   const float* b1_p2, const float* w2_p2, const float* b2_p2, const float* w3_p2, const float* b3_p2, void* out_p1,
                   void* out_p2, int32_t out_format, int64_t out_pitch, void* stream)
{
    if (!obs_p1 || !w1_p1 || !b1_p1 || !w2_p1 || !b2_p1 || !w3_p1 || !b3_p1 || !out_p1) return PZ_E_NULL;
    const void* second[] = {obs_p2, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2, out_p2};
    int present = 0;
    for (const void* p : second) present += p != nullptr;
    if (present != 0 && present != 8) return PZ_E_NULL;
    if (n < 0 || n > kMaxRows || in_features < 1 || in_features > PZ_NET_MAX_IN || (hidden != 32 && hidden != 64 && hidden != 128) ||
        out_features < 1 || out_features > PZ_NET_MAX_OUT || bad_pitch(n, in_features, obs_pitch) || bad_pitch(n, out_features, out_pitch))
        return PZ_E_SIZE;
    if (obs_format < PZ_NET_OBS_INT32 || obs_format > PZ_NET_OBS_BFLOAT16 || out_format < PZ_NET_OUT_FLOAT32 ||
        out_format > PZ_NET_OUT_BFLOAT16 || (activation != PZ_NET_ACT_TANH && activation != PZ_NET_ACT_RELU))
        return PZ_E_CONFIG;
    const uintptr_t xb = obs_format == PZ_NET_OBS_INT32 || obs_format == PZ_NET_OBS_FLOAT32 ? 4 : 2;
    const uintptr_t yb = out_format == PZ_NET_OUT_FLOAT32 ? 4 : 2;
    if (misaligned(obs_p1, xb) || misaligned(obs_p2, xb) || misaligned(out_p1, yb) || misaligned(out_p2, yb)) return PZ_E_ALIGN;
    const float* params[] = {w1_p1, b1_p1, w2_p1, b2_p1, w3_p1, b3_p1, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2};
    for (const float* p : params)
        if (misaligned(p, 4)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const Args a{{obs_p1, obs_p2}, {w1_p1, w1_p2}, {b1_p1, b1_p2}, {w2_p1, w2_p2}, {b2_p1, b2_p2}, {w3_p1, w3_p2}, {b3_p1, b3_p2},
                 {out_p1, out_p2}, n, obs_pitch, out_pitch, (n + kTileRows - 1) / kTileRows, in_features, out_features, obs_format,
                 out_format};
    const unsigned sides = present ? 2 : 1;
    return activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, sides, stream)
                                         : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, sides, stream);
}

}  // extern "C"
