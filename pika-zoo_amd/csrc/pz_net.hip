// libpikazoo_net.so: the forward pass of the three-layer policy net in ONE launch (C ABI and the definition:
// include/pikazoo_net.h; the shape and its reasons: DESIGN.md 4.17).
//
// The tile -- the layout of the operands, the staging of the parameters into LDS and the three layers of 32 batch rows -- is
// csrc/pz_mlp_tile.hpp's, shared with libpikazoo_pool.so.  Here: which rows a wave takes, and the entry point's checks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_net.h"
#include "pz_mlp_tile.hpp"

namespace pz_net {

using namespace pz_mlp;

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

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_forward_kernel(const Args a)
{
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Staged s = staged_at<H>(lds, a.K, a.O);
    // the parameters, global -> LDS in operand order, once per workgroup
    stage_parameters<H>(s, a.w1[side], a.b1[side], a.w2[side], a.b2[side], a.w3[side], a.b3[side], a.K, a.O, tid);
    __syncthreads();
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < a.tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t row = tile * kTileRows + (lane & 31);
        tile_forward<H, ACT>(s, a.obs[side], a.out[side], row, row < a.n, a.K, a.O, a.obs_pitch, a.out_pitch, a.obs_format, a.out_format, lane);
    }
}

template <int H, int ACT>
static int launch(const Args& a, unsigned sides, void* stream)
{
    const size_t bytes = (size_t)lds_floats(a.K, H, a.O) * sizeof(float);
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_forward_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    const int64_t blocks = min((a.tiles + kWaves - 1) / kWaves, grid_cap(bytes, sides));
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
