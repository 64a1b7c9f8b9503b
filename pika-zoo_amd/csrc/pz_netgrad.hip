// libpikazoo_netgrad.so: the backward pass of the three-layer policy net -- the six parameter gradients from grad_head, the
// forward recomputed inside the call (C ABI and the definition: include/pikazoo_netgrad.h; the shape and its reasons:
// DESIGN.md 4.18).
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact float32), D[i][j] += A[i][k] B[k][j] with
//     A: lane l holds A[i = l & 31][k = l >> 5],   B: lane l holds B[k = l >> 5][j = l & 31],
//     D: lane l, register r holds D[i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][j = l & 31].
// A workgroup of four waves takes a PASS of R = 32 * (128 / H) consecutive rows, so that every layer of the chain
// (h1, h2, d2, d1: H x R values each) is four 32 x 32 tiles, one per wave.  The chain has the feature on i and the batch row
// on j; a weight gradient sums over the batch, which therefore sits on k, with one activation as A and another as B.  Both
// orientations read the same LDS buffer buf[feature][row] (row pitch R + 1: neither walk conflicts): the chain reads
// buf[k][j], a gradient tile reads buf[i or j][k].  Only W2 and W3 are staged in LDS, row-major with a pitch of H + 1, and
// serve W . h (lane on the row) as well as W^T . d (lane on the column); W1, the observations and grad_head come from
// global memory in the orientation each use needs.  The gradient tiles (up to 36 at H = 128) are dealt round-robin to the four
// waves and live in their accumulation registers across all passes of the workgroup; the bias gradients are the running sums
// of the A operands of the tiles in tile column 0.  A workgroup's sums go to the workspace with plain stores, a second launch
// adds the workgroups' partials in index order: no atomics, the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "pikazoo_hip.h"
#include "pikazoo_net.h"
#include "pikazoo_netgrad.h"

namespace pz_netgrad {

constexpr int kThreads = 256;  // four waves, one per SIMD
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kReduceThreads = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Args {
    const void* obs[2];
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
    const float* w3[2];
    const void* grad[2];
    float* ws;
    int64_t n, obs_pitch, grad_pitch, passes;
    int32_t K, O, obs_format, grad_format;
};

// floats of one workgroup's partial sums: [dW1: H K][db1: H][dW2: H H][db2: H][dW3: O H][db3: O]
__host__ __device__ constexpr int64_t partial_floats(int K, int H, int O) { return (int64_t)H * K + H + H * H + H + O * H + O; }
// floats of LDS: [W2: H (H + 1)][W3: O (H + 1)][three buffers: H (R + 1)][b1: H][b2: H]
__host__ __device__ constexpr int rows_per_pass(int H) { return 32 * (128 / H); }
__host__ __device__ constexpr int lds_floats(int H, int O) { return (H + O) * (H + 1) + 3 * H * (rows_per_pass(H) + 1) + 2 * H; }

__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// N elements of a tensor of pz_net_obs_format `format`, as float32; an element that is not `ok` is +0 and its address is not
// formed (element 0 is read in its place).  The switch on the format stands outside the loads: one wave-uniform branch per group.
template <int N>
__device__ __forceinline__ void load_values(const void* p, int format, const int64_t (&idx)[N], const bool (&ok)[N], float (&v)[N])
{
    auto each = [&](auto element) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float x = element(ok[u] ? idx[u] : (int64_t)0);
            v[u] = ok[u] ? x : 0.0f;
        }
    };
    switch (format) {
        case PZ_NET_OBS_INT32:
            each([&](int64_t i) { return (float)((const int32_t*)p)[i]; });  // (beyond 2^24: to nearest even)
            break;
        case PZ_NET_OBS_INT16:
            each([&](int64_t i) { return (float)((const int16_t*)p)[i]; });
            break;
        case PZ_NET_OBS_FLOAT32:
            each([&](int64_t i) { return ((const float*)p)[i]; });
            break;
        case PZ_NET_OBS_FLOAT16:
            each([&](int64_t i) { return (float)((const _Float16*)p)[i]; });
            break;
        default:  // bfloat16: the upper half of a float32
            each([&](int64_t i) { return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16); });
            break;
    }
}

// pz_net_out_format -> the observation format of the same element type
__device__ __forceinline__ int grad_as_obs_format(int format) { return format + PZ_NET_OBS_FLOAT32; }
static_assert(PZ_NET_OUT_FLOAT32 + PZ_NET_OBS_FLOAT32 == PZ_NET_OBS_FLOAT32 && PZ_NET_OUT_FLOAT16 + PZ_NET_OBS_FLOAT32 == PZ_NET_OBS_FLOAT16 &&
                  PZ_NET_OUT_BFLOAT16 + PZ_NET_OBS_FLOAT32 == PZ_NET_OBS_BFLOAT16,
              "the two enums keep their order");

template <int ACT>
__device__ __forceinline__ float activate(float z)
{
    if constexpr (ACT == PZ_NET_ACT_TANH)
        return tanhf(z);
    else
        return z < 0.0f ? 0.0f : z;  // (a NaN is not < 0: it stays)
}

// act'(z) from h = act(z).  relu: h == 0 exactly where z <= 0 (z = -0 gives h = -0), and a NaN h is not 0: the factor is 1.
template <int ACT>
__device__ __forceinline__ float derivative(float h)
{
    if constexpr (ACT == PZ_NET_ACT_TANH)
        return 1.0f - h * h;
    else
        return h == 0.0f ? 0.0f : 1.0f;
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// A gradient tile over the R rows of a pass: acc[i][j] += sum_row A(i, row) B(row, j), bsum += the A operands (the bias
// gradient of the tile's 32 rows, one half of the batch rows per lane half).  `fill_a` and `fill_b` give this lane's operands
// of kTileUnroll k-steps from step s0 on: step s holds the pass's row 2 s + (lane >> 5).
constexpr int kTileUnroll = 8;

template <int R, class FA, class FB>
__device__ __forceinline__ void grad_tile(f32x16& acc, float& bsum, FA fill_a, FB fill_b)
{
#pragma unroll 1
    for (int s0 = 0; s0 < R / 2; s0 += kTileUnroll) {
        float av[kTileUnroll], bv[kTileUnroll];
        fill_a(s0, av);
        fill_b(s0, bv);
#pragma unroll
        for (int u = 0; u < kTileUnroll; ++u) {
            acc = mfma(av[u], bv[u], acc);
            bsum += av[u];
        }
    }
}

// a finished tile -> the workgroup's partial sums: dW[32 ti + i][32 tj + j], and the bias gradient where tj == 0
__device__ __forceinline__ void store_tile(const f32x16& acc, float bsum, float* dw, float* db, int ti, int tj, int rows, int cols,
                                           int lane)
{
    const int half = lane >> 5, j = 32 * tj + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = 32 * ti + acc_row(r, half);
        if (i < rows && j < cols) dw[i * cols + j] = acc[r];
    }
    const float other = __shfl_xor(bsum, 32);  // the other half of the batch rows: a + b in both lanes
    const int f = 32 * ti + (lane & 31);
    if (tj == 0 && half == 0 && f < rows) db[f] = bsum + other;
}

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_backward_kernel(const Args a)
{
    constexpr int TH = H / 32, R = rows_per_pass(H), RP = R + 1, HP = H + 1;
    constexpr int M3 = (2 * TH + kWaves - 1) / kWaves, M2 = (TH * TH + kWaves - 1) / kWaves, M1 = (3 * TH + kWaves - 1) / kWaves;
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int K = a.K, O = a.O, TO = (O + 31) >> 5, TK = (K + 31) >> 5;
    float* w2s = lds;
    float* w3s = w2s + H * HP;
    float* buf1 = w3s + O * HP;  // h1
    float* buf2 = buf1 + H * RP;  // h2, then d1
    float* buf3 = buf2 + H * RP;  // d2
    float* bias1 = buf3 + H * RP;
    float* bias2 = bias1 + H;

    for (int e = tid; e < H * H; e += kThreads) w2s[(e / H) * HP + (e % H)] = a.w2[side][e];
    for (int e = tid; e < O * H; e += kThreads) w3s[(e / H) * HP + (e % H)] = a.w3[side][e];
    for (int e = tid; e < H; e += kThreads) {
        bias1[e] = a.b1[side][e];
        bias2[e] = a.b2[side][e];
    }
    __syncthreads();

    const void* obs = a.obs[side];
    const void* grad = a.grad[side];
    const float* w1 = a.w1[side];
    const int obs_format = a.obs_format, grad_format = grad_as_obs_format(a.grad_format);
    // this wave's tile of the chain: features 32 th .., rows 32 rt .. of the pass
    const int th = wave % TH, rt = wave / TH;
    const int f_lane = 32 * th + l31;  // (the feature of this lane as an A operand)
    const int col = 32 * rt + l31;     // (the row of the pass of this lane as a B operand and in the result)
    // the LDS operands of kTileUnroll steps: row 2 s + half of a feature's line
    auto from_lds = [&](const float* line) {
        return [=](int s0, float (&v)[kTileUnroll]) {
#pragma unroll
            for (int u = 0; u < kTileUnroll; ++u) v[u] = line[2 * (s0 + u) + half];
        };
    };

    f32x16 g3[M3] = {}, g2[M2] = {}, g1[M1] = {};
    float s3[M3] = {}, s2[M2] = {}, s1[M1] = {};

    for (int64_t pass = blockIdx.x; pass < a.passes; pass += gridDim.x) {
        const int64_t row0 = pass * R, row = row0 + col;
        const bool live = row < a.n;
        const int64_t obs_at = row * a.obs_pitch, grad_at = row * a.grad_pitch;
        // the global operands of kTileUnroll steps: column c of the rows 2 s + half of the pass
        auto from_rows = [&](const void* p, int format, int64_t pitch, int c, bool c_ok) {
            return [=](int s0, float (&v)[kTileUnroll]) {
                int64_t idx[kTileUnroll];
                bool ok[kTileUnroll];
#pragma unroll
                for (int u = 0; u < kTileUnroll; ++u) {
                    const int64_t r = row0 + 2 * (s0 + u) + half;
                    ok[u] = c_ok && r < a.n;
                    idx[u] = r * pitch + c;
                }
                load_values(p, format, idx, ok, v);
            };
        };

        // ---- h1 = act(W1 x + b1) -------------------------------------------------------------------------------------------
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias1[32 * th + acc_row(r, half)];
#pragma unroll 1
        for (int s0 = 0; s0 < (K + 1) / 2; s0 += 4) {
            float av[4], bv[4];
            int64_t idx[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 2 * (s0 + u) + half;
                av[u] = w1[k < K ? f_lane * K + k : 0];
                av[u] = k < K ? av[u] : 0.0f;
                ok[u] = live && k < K;
                idx[u] = obs_at + k;
            }
            load_values(obs, obs_format, idx, ok, bv);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma(av[u], bv[u], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) buf1[(32 * th + acc_row(r, half)) * RP + col] = live ? activate<ACT>(acc[r]) : 0.0f;
        __syncthreads();

        // ---- h2 = act(W2 h1 + b2) ------------------------------------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias2[32 * th + acc_row(r, half)];
#pragma unroll 8
        for (int s = 0; s < H / 2; ++s) {
            const int k = 2 * s + half;
            acc = mfma(w2s[f_lane * HP + k], buf1[k * RP + col], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) buf2[(32 * th + acc_row(r, half)) * RP + col] = live ? activate<ACT>(acc[r]) : 0.0f;
        __syncthreads();

        // ---- d2 = (W3^T d3) act'(z2), and dW3 += d3 h2^T ------------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 1
        for (int s0 = 0; s0 < (O + 1) / 2; s0 += 4) {
            float av[4], bv[4];
            int64_t idx[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = 2 * (s0 + u) + half;
                av[u] = w3s[o < O ? o * HP + f_lane : 0];
                av[u] = o < O ? av[u] : 0.0f;
                ok[u] = live && o < O;
                idx[u] = grad_at + o;
            }
            load_values(grad, grad_format, idx, ok, bv);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma(av[u], bv[u], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = (32 * th + acc_row(r, half)) * RP + col;
            buf3[at] = live ? acc[r] * derivative<ACT>(buf2[at]) : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < M3; ++m) {
            const int q = wave + kWaves * m;
            if (q < TO * TH) {
                const int o = 32 * (q / TH) + l31;
                grad_tile<R>(g3[m], s3[m], from_rows(grad, grad_format, a.grad_pitch, o, o < O), from_lds(buf2 + (32 * (q % TH) + l31) * RP));
            }
        }
        __syncthreads();

        // ---- d1 = (W2^T d2) act'(z1) -> buf2 (h2 is done with), and dW2 += d2 h1^T ----------------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 8
        for (int s = 0; s < H / 2; ++s) {
            const int k = 2 * s + half;
            acc = mfma(w2s[k * HP + f_lane], buf3[k * RP + col], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = (32 * th + acc_row(r, half)) * RP + col;
            buf2[at] = live ? acc[r] * derivative<ACT>(buf1[at]) : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < M2; ++m) {
            const int q = wave + kWaves * m;
            if (q < TH * TH)
                grad_tile<R>(g2[m], s2[m], from_lds(buf3 + (32 * (q / TH) + l31) * RP), from_lds(buf1 + (32 * (q % TH) + l31) * RP));
        }
        __syncthreads();

        // ---- dW1 += d1 x^T --------------------------------------------------------------------------------------------------
#pragma unroll
        for (int m = 0; m < M1; ++m) {
            const int q = wave + kWaves * m;
            if (q < TH * TK) {
                const int k = 32 * (q % TK) + l31;
                grad_tile<R>(g1[m], s1[m], from_lds(buf2 + (32 * (q / TK) + l31) * RP), from_rows(obs, obs_format, a.obs_pitch, k, k < K));
            }
        }
        // (the next pass writes buf1, last read before the barrier above, and writes buf2 behind its own first barrier)
    }

    // ---- this workgroup's partial sums ----------------------------------------------------------------------------------------
    float* p = a.ws + ((int64_t)side * gridDim.x + blockIdx.x) * partial_floats(K, H, O);
    float* dw1 = p;
    float* db1 = dw1 + H * K;
    float* dw2 = db1 + H;
    float* db2 = dw2 + H * H;
    float* dw3 = db2 + H;
    float* db3 = dw3 + O * H;
#pragma unroll
    for (int m = 0; m < M3; ++m) {
        const int q = wave + kWaves * m;
        if (q < TO * TH) store_tile(g3[m], s3[m], dw3, db3, q / TH, q % TH, O, H, lane);
    }
#pragma unroll
    for (int m = 0; m < M2; ++m) {
        const int q = wave + kWaves * m;
        if (q < TH * TH) store_tile(g2[m], s2[m], dw2, db2, q / TH, q % TH, H, H, lane);
    }
#pragma unroll
    for (int m = 0; m < M1; ++m) {
        const int q = wave + kWaves * m;
        if (q < TH * TK) store_tile(g1[m], s1[m], dw1, db1, q / TK, q % TK, H, K, lane);
    }
}

struct ReduceArgs {
    const float* ws;
    float* out[2][6];
    int64_t blocks, floats;  // workgroups per agent, floats per partial
    int32_t ends[6];         // the end of each of the six tensors within a partial
    int32_t sides_in, sides_out;
};

// out[e] = the partials of element e in index order; a shared net adds agent 2's total to agent 1's
__global__ __launch_bounds__(kReduceThreads) void mlp_backward_reduce_kernel(const ReduceArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kReduceThreads + threadIdx.x;
    if (e >= a.floats) return;
    const int side = blockIdx.y;
    auto total = [&](int s) {
        const float* p = a.ws + (int64_t)s * a.blocks * a.floats + e;
        float sum = p[0];
        for (int64_t b = 1; b < a.blocks; ++b) sum += p[b * a.floats];
        return sum;
    };
    float sum = total(side);
    if (a.sides_in == 2 && a.sides_out == 1) sum += total(1);
    int t = 0, begin = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (e >= a.ends[i]) {
            t = i + 1;
            begin = a.ends[i];
        }
    a.out[side][t][e - begin] = sum;
}

static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

static bool bad_pitch(int64_t n, int64_t width, int64_t pitch)
{
    if (pitch < width) return true;
    return n > 0 && pitch > (INT64_MAX / 4) / n;  // n * pitch * 4 bytes: refused, never wrapped
}

static bool in_box(int64_t n, int32_t in_features, int32_t hidden, int32_t out_features)
{
    return n >= 0 && n <= kMaxRows && in_features >= 1 && in_features <= PZ_NET_MAX_IN && (hidden == 32 || hidden == 64 || hidden == 128) &&
           out_features >= 1 && out_features <= PZ_NET_MAX_OUT;
}

// workgroups per agent: one per pass up to one per compute unit (a fixed 256 where the device cannot be asked)
static int64_t blocks_of(int64_t n, int hidden)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    const int64_t R = rows_per_pass(hidden), passes = (n + R - 1) / R;
    return passes < cus ? passes : cus;
}

template <int H, int ACT>
static int launch(const Args& a, int64_t blocks, unsigned sides, void* stream)
{
    const size_t bytes = (size_t)lds_floats(H, a.O) * sizeof(float);
    constexpr size_t most = (size_t)lds_floats(H, PZ_NET_MAX_OUT) * sizeof(float);
    if constexpr (most > 64 * 1024) {
        // above the default limit of a launch's dynamic LDS: raised to the instance's largest size, once per device (a bit per
        // device; a device beyond the mask, or one that cannot be asked, is set on every call)
        static std::atomic<uint64_t> raised{0};
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
        const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t)1 << dev : 0;
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            const hipError_t e = hipFuncSetAttribute((const void*)mlp_backward_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
            if (e != hipSuccess) return (int)e;
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((mlp_backward_kernel<H, ACT>), dim3((unsigned)blocks, sides), dim3(kThreads), bytes, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

template <int ACT>
static int launch_hidden(const Args& a, int hidden, int64_t blocks, unsigned sides, void* stream)
{
    switch (hidden) {
        case 32:
            return launch<32, ACT>(a, blocks, sides, stream);
        case 64:
            return launch<64, ACT>(a, blocks, sides, stream);
        default:
            return launch<128, ACT>(a, blocks, sides, stream);
    }
}

}  // namespace pz_netgrad

using namespace pz_netgrad;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kNetgradBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_netgrad_build_id(void) { return kNetgradBuildIdRecord + 12; }

int pz_netgrad_abi_version(void) { return PZ_NETGRAD_ABI_VERSION; }

int64_t pz_mlp_backward_workspace_bytes(int64_t n, int32_t in_features, int32_t hidden, int32_t out_features)
{
    if (n <= 0 || !in_box(n, in_features, hidden, out_features)) return 0;
    return 2 * blocks_of(n, hidden) * partial_floats(in_features, hidden, out_features) * (int64_t)sizeof(float);
}

int pz_mlp_backward(const void* obs_p1, const void* obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch,
                    int32_t hidden, int32_t out_features, int32_t activation, const float* w1_p1, const float* b1_p1,
                    const float* w2_p1, const float* b2_p1, const float* w3_p1, const float* b3_p1, const float* w1_p2,
                    const float* b1_p2, const float* w2_p2, const float* b2_p2, const float* w3_p2, const float* b3_p2,
                    const void* grad_head_p1, const void* grad_head_p2, int32_t grad_format, int64_t grad_pitch, float* dw1_p1,
                    float* db1_p1, float* dw2_p1, float* db2_p1, float* dw3_p1, float* db3_p1, float* dw1_p2, float* db1_p2,
                    float* dw2_p2, float* db2_p2, float* dw3_p2, float* db3_p2, void* workspace, void* stream)
{
    const float* params1[] = {w1_p1, b1_p1, w2_p1, b2_p1, w3_p1, b3_p1};
    const float* params2[] = {w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2};
    float* grads1[] = {dw1_p1, db1_p1, dw2_p1, db2_p1, dw3_p1, db3_p1};
    float* grads2[] = {dw1_p2, db1_p2, dw2_p2, db2_p2, dw3_p2, db3_p2};
    if (!obs_p1 || !grad_head_p1 || !workspace) return PZ_E_NULL;
    int present = (obs_p2 != nullptr) + (grad_head_p2 != nullptr), outputs = 0;
    for (int i = 0; i < 6; ++i) {
        if (!params1[i] || !grads1[i]) return PZ_E_NULL;
        present += params2[i] != nullptr;
        outputs += grads2[i] != nullptr;
    }
    if ((present != 0 && present != 8) || (outputs != 0 && outputs != 6) || (present == 0 && outputs != 0)) return PZ_E_NULL;
    if (!in_box(n, in_features, hidden, out_features) || bad_pitch(n, in_features, obs_pitch) || bad_pitch(n, out_features, grad_pitch))
        return PZ_E_SIZE;
    if (obs_format < PZ_NET_OBS_INT32 || obs_format > PZ_NET_OBS_BFLOAT16 || grad_format < PZ_NET_OUT_FLOAT32 ||
        grad_format > PZ_NET_OUT_BFLOAT16 || (activation != PZ_NET_ACT_TANH && activation != PZ_NET_ACT_RELU))
        return PZ_E_CONFIG;
    const bool shared = present != 0 && outputs == 0;
    if (shared)
        for (int i = 0; i < 6; ++i)
            if (params2[i] != params1[i]) return PZ_E_CONFIG;
    const uintptr_t xb = obs_format == PZ_NET_OBS_INT32 || obs_format == PZ_NET_OBS_FLOAT32 ? 4 : 2;
    const uintptr_t gb = grad_format == PZ_NET_OUT_FLOAT32 ? 4 : 2;
    if (misaligned(obs_p1, xb) || misaligned(obs_p2, xb) || misaligned(grad_head_p1, gb) || misaligned(grad_head_p2, gb) ||
        misaligned(workspace, 16))
        return PZ_E_ALIGN;
    for (int i = 0; i < 6; ++i)
        if (misaligned(params1[i], 4) || misaligned(params2[i], 4) || misaligned(grads1[i], 4) || misaligned(grads2[i], 4)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;

    const int R = rows_per_pass(hidden);
    const int64_t blocks = blocks_of(n, hidden);
    const unsigned sides = present ? 2 : 1;
    const Args a{{obs_p1, obs_p2}, {w1_p1, w1_p2}, {b1_p1, b1_p2}, {w2_p1, w2_p2}, {b2_p1, b2_p2}, {w3_p1, w3_p2},
                 {grad_head_p1, grad_head_p2}, (float*)workspace, n, obs_pitch, grad_pitch, (n + R - 1) / R, in_features, out_features,
                 obs_format, grad_format};
    const int code = activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, blocks, sides, stream)
                                                   : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, blocks, sides, stream);
    if (code != 0) return code;
    ReduceArgs r{};
    r.ws = (const float*)workspace;
    for (int i = 0; i < 6; ++i) {
        r.out[0][i] = grads1[i];
        r.out[1][i] = grads2[i];
    }
    r.blocks = blocks;
    r.floats = partial_floats(in_features, hidden, out_features);
    const int32_t sizes[6] = {hidden * in_features, hidden, hidden * hidden, hidden, out_features * hidden, out_features};
    int32_t end = 0;
    for (int i = 0; i < 6; ++i) r.ends[i] = end += sizes[i];
    r.sides_in = (int32_t)sides;
    r.sides_out = shared ? 1 : (int32_t)sides;
    hipLaunchKernelGGL(mlp_backward_reduce_kernel, dim3((unsigned)((r.floats + kReduceThreads - 1) / kReduceThreads), (unsigned)r.sides_out),
                       dim3(kReduceThreads), 0, (hipStream_t)stream, r);
    return (int)hipGetLastError();
}

}  // extern "C"
