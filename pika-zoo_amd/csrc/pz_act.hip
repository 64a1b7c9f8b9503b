// libpikazoo_act.so: the policy net's forward and the categorical head over its logits in ONE launch, from observation rows
// to (action, log-prob, entropy, value) (C ABI and the definition, by reference to the two launches it replaces:
// include/pikazoo_act.h; the shape and its reasons: DESIGN.md 4.23).
//
// The workgroup, the staging and the grid-stride loop over 32-row tiles are pz_net.hip's, and the three layers are
// tile_forward's text beside it (csrc/pz_mlp_tile.hpp, tile_layers: the same chains of the same products).  A tile ends with
// the head in the accumulators: output o of batch row j in lane (j, half h), register r with o = 32 t + acc_row(r, h).  The
// head's row code (csrc/pz_policy_rows.hpp) wants one lane to walk one row, so the wave writes its accumulators into an LDS
// image of its own, 32 rows x (O | 1) floats (the odd stride for the reason given at the top of pz_policy.hip: 32 lanes
// reading column i of 32 rows hit 32 banks), and the 32 lanes of half 0 each take their row from it: row_stats, the Philox
// block, the draw, the log-prob -- pz_sample_actions' functions, or its own lines repeated in pz_policy_rows.hpp, on the
// float32 values pz_mlp_forward would have stored, hence the bits of the two launches.
//   * The waves of a workgroup have different trip counts: there is NO workgroup barrier inside the tile loop.  The image is
//     written and read by one wave only; its writes are ordered before its reads (and a tile's reads before the next tile's
//     writes) by a wavefront-scope fence around a wave barrier: the LDS executes one wave's instructions in order, the fence
//     keeps the compiler from reordering them.
//   * A is a runtime value: the passes re-read the image, as sample_kernel does.
//   * Half the lanes idle during the row work (two tiles per sampling pass is the open lever).
//   * The optional head store goes from the registers, as tile_forward's does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_act.h"
#include "pikazoo_hip.h"
#include "pikazoo_net.h"
#include "pikazoo_policy.h"
#include "pz_mlp_tile.hpp"
#include "pz_policy_rows.hpp"

namespace pz_act {

using namespace pz_mlp;

struct Args {
    const void* obs[2];
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
    const float* w3[2];
    const float* b3[2];
    void* act[2];
    float* logp[2];
    float* ent[2];
    float* val[2];
    float* head[2];
    const uint64_t* step_dev;
    uint64_t step;
    int64_t first_game, n, obs_pitch, head_pitch, tiles;
    int32_t K, O, A, obs_format, action_format;
    uint32_t key0, key1;
};

// floats of one wave's image, and the dynamic LDS of a launch: the staged parameter set and the four images behind it
__host__ __device__ constexpr int image_stride(int O) { return O | 1; }
__host__ __device__ constexpr int act_lds_floats(int K, int H, int O) { return lds_floats(K, H, O) + kWaves * kTileRows * image_stride(O); }

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_act_kernel(const Args a)
{
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const Staged s = staged_at<H>(lds, a.K, a.O);
    const int stride = image_stride(a.O);
    float* image = lds + lds_floats(a.K, H, a.O) + wave * kTileRows * stride;  // this wave's alone
    float* mine = image + j * stride;
    // the parameters, global -> LDS in operand order, once per workgroup
    stage_parameters<H>(s, a.w1[side], a.b1[side], a.w2[side], a.b2[side], a.w3[side], a.b3[side], a.K, a.O, tid);
    __syncthreads();
    const uint64_t T = a.step + (a.step_dev ? *a.step_dev : 0);
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < a.tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t g = tile * kTileRows + j;
        const bool live = g < a.n;
        f32x16 y[2];
        tile_layers<H, ACT>(s, a.obs[side], g, live, a.K, a.O, a.obs_pitch, a.obs_format, lane, y);
        if (a.head[side]) store_tile_float32(y, a.head[side], g, live, a.O, a.head_pitch, lane);
        // registers -> the wave's image: both halves write their columns of row j
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * t + acc_row(r, half);
                if (o < a.O) mine[o] = y[t][r];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (half == 0 && live) {
            const pz_policy::RowStats st = pz_policy::row_stats(mine, a.A);
            const float u = pz_policy::draw_uniform((uint64_t)(a.first_game + g), T, a.key0, a.key1, side);
            const int act = pz_policy::draw_action(mine, a.A, st, u);
            if (a.action_format == PZ_POLICY_ACTION_INT32)
                ((int32_t*)a.act[side])[g] = act;
            else
                ((int64_t*)a.act[side])[g] = act;
            const float logp = pz_policy::action_log_prob(mine, a.A, st, act);
            const float nan = __uint_as_float(0x7FC00000u);
            if (a.logp[side]) a.logp[side][g] = logp;
            if (a.ent[side]) a.ent[side][g] = st.bad ? nan : st.H;
            if (a.val[side]) a.val[side][g] = mine[a.A];  // (O > A: checked by the entry point)
        }
        // this tile's reads before the next tile's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int H, int ACT>
static int launch(const Args& a, unsigned sides, void* stream)
{
    const size_t bytes = (size_t)act_lds_floats(a.K, H, a.O) * sizeof(float);
    static_assert((size_t)act_lds_floats(PZ_NET_MAX_IN, 128, PZ_NET_MAX_OUT) * sizeof(float) <= (size_t)kLdsBytes, "the worst case fits the LDS");
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_act_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    const int64_t blocks = min((a.tiles + kWaves - 1) / kWaves, grid_cap(bytes, sides));  // (the full figure: images included)
    hipLaunchKernelGGL((mlp_act_kernel<H, ACT>), dim3((unsigned)blocks, sides), dim3(kThreads), bytes, (hipStream_t)stream, a);
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

}  // namespace pz_act

using namespace pz_act;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kActBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_act_build_id(void) { return kActBuildIdRecord + 12; }

int pz_act_abi_version(void) { return PZ_ACT_ABI_VERSION; }

int pz_mlp_act(const void* obs_p1, const void* obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch, int32_t hidden,
               int32_t out_features, int32_t activation, const float* w1_p1, const float* b1_p1, const float* w2_p1, const float* b2_p1,
               const float* w3_p1, const float* b3_p1, const float* w1_p2, const float* b1_p2, const float* w2_p2, const float* b2_p2,
               const float* w3_p2, const float* b3_p2, int32_t num_actions, uint64_t seed, int64_t first_game, uint64_t step,
               const uint64_t* step_dev, int32_t action_format, void* act_p1, void* act_p2, float* logp_p1, float* logp_p2, float* ent_p1,
               float* ent_p2, float* val_p1, float* val_p2, float* head_p1, float* head_p2, int64_t head_pitch, void* stream)
{
    using pz_policy::paired;
    if (!obs_p1 || !w1_p1 || !b1_p1 || !w2_p1 || !b2_p1 || !w3_p1 || !b3_p1 || !act_p1) return PZ_E_NULL;
    const void* second[] = {obs_p2, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2};
    int present = 0;
    for (const void* p : second) present += p != nullptr;
    if (present != 0 && present != 7) return PZ_E_NULL;
    const bool both = present != 0;
    if (!paired(act_p1, act_p2, both) || !paired(logp_p1, logp_p2, both) || !paired(ent_p1, ent_p2, both) || !paired(val_p1, val_p2, both) ||
        !paired(head_p1, head_p2, both))
        return PZ_E_NULL;
    if (n < 0 || n > kMaxRows || in_features < 1 || in_features > PZ_NET_MAX_IN || (hidden != 32 && hidden != 64 && hidden != 128) ||
        num_actions < 2 || num_actions > PZ_ACT_MAX_ACTIONS || out_features < num_actions || out_features > PZ_NET_MAX_OUT ||
        (val_p1 && out_features == num_actions) || bad_pitch(n, in_features, obs_pitch) || (head_p1 && bad_pitch(n, out_features, head_pitch)))
        return PZ_E_SIZE;
    if (first_game < 0 || step >= ((uint64_t)1 << 62)) return PZ_E_SIZE;
    if (obs_format < PZ_NET_OBS_INT32 || obs_format > PZ_NET_OBS_BFLOAT16 || (activation != PZ_NET_ACT_TANH && activation != PZ_NET_ACT_RELU) ||
        !pz_policy::known_action_format(action_format))
        return PZ_E_CONFIG;
    const uintptr_t xb = obs_format == PZ_NET_OBS_INT32 || obs_format == PZ_NET_OBS_FLOAT32 ? 4 : 2;
    const uintptr_t ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    using pz_mlp::misaligned;
    if (misaligned(obs_p1, xb) || misaligned(obs_p2, xb) || misaligned(act_p1, ab) || misaligned(act_p2, ab) || misaligned(step_dev, 8))
        return PZ_E_ALIGN;
    const void* floats[] = {w1_p1, b1_p1, w2_p1, b2_p1, w3_p1, b3_p1, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2, logp_p1, logp_p2,
                            ent_p1, ent_p2, val_p1, val_p2, head_p1, head_p2};
    for (const void* p : floats)
        if (misaligned(p, 4)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const Args a{{obs_p1, obs_p2}, {w1_p1, w1_p2}, {b1_p1, b1_p2}, {w2_p1, w2_p2}, {b2_p1, b2_p2}, {w3_p1, w3_p2}, {b3_p1, b3_p2},
                 {act_p1, act_p2}, {logp_p1, logp_p2}, {ent_p1, ent_p2}, {val_p1, val_p2}, {head_p1, head_p2}, step_dev, step, first_game, n,
                 obs_pitch, head_p1 ? head_pitch : 0, (n + kTileRows - 1) / kTileRows, in_features, out_features, num_actions, obs_format,
                 action_format, (uint32_t)seed, (uint32_t)(seed >> 32)};
    const unsigned sides = both ? 2 : 1;
    return activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, sides, stream)
                                         : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, sides, stream);
}

}  // extern "C"
