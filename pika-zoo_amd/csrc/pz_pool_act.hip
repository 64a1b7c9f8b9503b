// libpikazoo_pool_act.so: the policy net's forward for a POOL of parameter sets and the categorical head over its logits in ONE
// launch, every row through the set of its own pool member, from observation rows to (action, log-prob, entropy, value) (C ABI
// and the definition, by reference to the two launches it replaces: include/pikazoo_pool_act.h; the shape and its reasons:
// DESIGN.md 4.24).
//
// The walk is pz_pool.hip's: the plan's `first` words in LDS, a contiguous range of groups of G = 128 slots per workgroup, a
// group's member found from `first`, the parameters re-staged only where the member changes.  The group loop is uniform over
// the workgroup (every wave takes its 32 slots of every group), so the workgroup barriers around a re-staging are legal here;
// pz_act.hip's tile loop, whose waves have different trip counts, could not hold them.  Inside a group a wave does what
// pz_act.hip's does inside a tile: tile_layers on its 32 slots of `order`, the optional head store from the registers, the
// accumulators into an LDS image of its own -- 32 rows x (O | 1) floats behind the staged set and the `first` words -- and the 32
// lanes of half 0 run the row code of csrc/pz_policy_rows.hpp for row = order[slot].
//   * The image is written and read by one wave only, ordered by a wavefront-scope fence around a wave barrier (pz_act.hip says
//     why that is enough).  NO workgroup barrier stands between a wave's image write and its read: the only ones are those
//     around a re-staging, at the top of a group, and the images do not overlap the staged set.
//   * The global game id is first_game + row, the ROW, not the slot: a row's bits do not depend on the plan around it.
//   * An agent with none of logp, ent and val skips the log-prob and every store but the action's; the action comes from the
//     same row_stats and the same draw, hence the same bit.
//   * Nothing of csrc/pz_mlp_tile.hpp, csrc/pz_policy_rows.hpp, pz_pool.hip or pz_act.hip is changed: the group walk and the
//     image hand-off are repeated here beside their first texts (as DESIGN.md 4.23 did), so no older kernel moves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_net.h"
#include "pikazoo_policy.h"
#include "pikazoo_pool.h"
#include "pikazoo_pool_act.h"
#include "pz_mlp_tile.hpp"
#include "pz_policy_rows.hpp"

namespace pz_pool_act {

using namespace pz_mlp;

constexpr int G = PZ_POOL_GROUP_ROWS;
constexpr int kMaxMembers = PZ_POOL_MAX_MEMBERS;
constexpr int kFirstWords = 32;  // the P + 1 words of `first` behind the staged parameter set, padded (pz_pool.hip)
static_assert(G == kWaves * kTileRows, "a group is one tile per wave of the workgroup");
static_assert(kMaxMembers + 1 <= kFirstWords, "the words of `first` fit their place");

struct Args {
    const void* obs[2];
    const int32_t* order[2];
    const int32_t* first[2];
    void* act[2];
    float* logp[2];
    float* ent[2];
    float* val[2];
    float* head[2];
    const uint64_t* step_dev;
    uint64_t step;
    int64_t first_game, n, obs_pitch, head_pitch;
    int32_t K, O, A, obs_format, action_format, P, plan_groups, plain_groups;
    uint32_t key0, key1;
    pz_pool_member members[kMaxMembers];
};

// floats of one wave's image, and the dynamic LDS of a launch: the staged set, the `first` words, the four images
__host__ __device__ constexpr int image_stride(int O) { return O | 1; }
__host__ __device__ constexpr int pool_act_lds_floats(int K, int H, int O)
{
    return lds_floats(K, H, O) + kFirstWords + kWaves * kTileRows * image_stride(O);
}

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_act_pool_kernel(const Args a)
{
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int K = a.K, O = a.O, P = a.P;
    const Staged s = staged_at<H>(lds, K, O);
    int32_t* s_first = (int32_t*)(lds + lds_floats(K, H, O));
    const int stride = image_stride(O);
    float* image = lds + lds_floats(K, H, O) + kFirstWords + wave * kTileRows * stride;  // this wave's alone
    float* mine = image + j * stride;
    const int32_t* order = a.order[side];
    const void* obs = a.obs[side];
    const bool stats = a.logp[side] || a.ent[side] || a.val[side];
    const uint64_t T = a.step + (a.step_dev ? *a.step_dev : 0);

    // the groups of this agent: those of its plan (whatever the words hold, they are used inside the capacity), or all rows
    int groups = a.plain_groups;
    if (order) {
        if (tid <= P) s_first[tid] = min(max(a.first[side][tid], 0), a.plan_groups * G);
        __syncthreads();
        groups = s_first[P] / G;
    }
    // a contiguous range of groups per workgroup: a member's groups are neighbours, so the parameters are re-staged rarely
    const int g0 = (int)((int64_t)blockIdx.x * groups / gridDim.x), g1 = (int)((int64_t)(blockIdx.x + 1) * groups / gridDim.x);
    int staged = -1;
    for (int g = g0; g < g1; ++g) {
        const int slot0 = g * G;
        int m = 0;
        if (order)
            for (int p = 1; p < P; ++p) m += s_first[p] <= slot0;  // (empty members share their successor's first slot)
        m = __builtin_amdgcn_readfirstlane(m);
        if (m != staged) {  // (uniform: a group has one member)
            if (staged >= 0) __syncthreads();
            const pz_pool_member& pm = a.members[m];
            stage_parameters<H>(s, pm.w1, pm.b1, pm.w2, pm.b2, pm.w3, pm.b3, K, O, tid);
            __syncthreads();
            staged = m;
        }
        const int slot = slot0 + wave * kTileRows + j;
        const int64_t row = order ? (int64_t)order[slot] : (int64_t)slot;
        const bool live = row >= 0 && row < a.n;  // (a pad of the plan is -1: handled like a row behind the last one)
        f32x16 y[2];
        tile_layers<H, ACT>(s, obs, row, live, K, O, a.obs_pitch, a.obs_format, lane, y);
        if (a.head[side]) store_tile_float32(y, a.head[side], row, live, O, a.head_pitch, lane);
        // registers -> the wave's image: both halves write their columns of slot j
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * t + acc_row(r, half);
                if (o < O) mine[o] = y[t][r];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (half == 0 && live) {
            const pz_policy::RowStats st = pz_policy::row_stats(mine, a.A);
            const float u = pz_policy::draw_uniform((uint64_t)(a.first_game + row), T, a.key0, a.key1, side);
            const int act = pz_policy::draw_action(mine, a.A, st, u);
            if (a.action_format == PZ_POLICY_ACTION_INT32)
                ((int32_t*)a.act[side])[row] = act;
            else
                ((int64_t*)a.act[side])[row] = act;
            if (stats) {  // (uniform over the launch's side: the frozen opponents' side skips all of it)
                const float logp = pz_policy::action_log_prob(mine, a.A, st, act);
                const float nan = __uint_as_float(0x7FC00000u);
                if (a.logp[side]) a.logp[side][row] = logp;
                if (a.ent[side]) a.ent[side][row] = st.bad ? nan : st.H;
                if (a.val[side]) a.val[side][row] = mine[a.A];  // (O > A: checked by the entry point)
            }
        }
        // this group's reads before the next group's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int H, int ACT>
static int launch(const Args& a, unsigned sides, void* stream)
{
    const size_t bytes = (size_t)pool_act_lds_floats(a.K, H, a.O) * sizeof(float);
    static_assert((size_t)pool_act_lds_floats(PZ_NET_MAX_IN, 128, PZ_NET_MAX_OUT) * sizeof(float) == 157568, "136 448 + 128 + 20 992 B at the largest");
    static_assert((size_t)pool_act_lds_floats(PZ_NET_MAX_IN, 128, PZ_NET_MAX_OUT) * sizeof(float) <= (size_t)kLdsBytes, "the worst case fits the LDS");
    static_assert(2 * (size_t)pool_act_lds_floats(35, 64, 19) * sizeof(float) <= (size_t)kLdsBytes, "two workgroups per compute unit at 35-64-19");
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_act_pool_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    int64_t blocks = 1;
    for (unsigned side = 0; side < sides; ++side) blocks = max(blocks, (int64_t)(a.order[side] ? a.plan_groups : a.plain_groups));
    blocks = min(blocks, grid_cap(bytes, sides));  // (the full figure: `first` and the images included)
    hipLaunchKernelGGL((mlp_act_pool_kernel<H, ACT>), dim3((unsigned)blocks, sides), dim3(kThreads), bytes, (hipStream_t)stream, a);
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

}  // namespace pz_pool_act

using namespace pz_pool_act;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kPoolActBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_pool_act_build_id(void) { return kPoolActBuildIdRecord + 12; }

int pz_pool_act_abi_version(void) { return PZ_POOL_ACT_ABI_VERSION; }

int pz_mlp_act_pool(const void* obs_p1, const void* obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch, int32_t hidden,
                    int32_t out_features, int32_t activation, const pz_pool_member* members, int32_t num_members, const int32_t* order_p1,
                    const int32_t* first_p1, const int32_t* order_p2, const int32_t* first_p2, int32_t num_actions, uint64_t seed,
                    int64_t first_game, uint64_t step, const uint64_t* step_dev, int32_t action_format, void* act_p1, void* act_p2, float* logp_p1,
                    float* logp_p2, float* ent_p1, float* ent_p2, float* val_p1, float* val_p2, float* head_p1, float* head_p2, int64_t head_pitch,
                    void* stream)
{
    if (!obs_p1 || !act_p1 || !members) return PZ_E_NULL;
    const bool second = obs_p2 != nullptr;
    if (second != (act_p2 != nullptr)) return PZ_E_NULL;
    if (!second && (order_p2 || first_p2 || logp_p2 || ent_p2 || val_p2 || head_p2)) return PZ_E_NULL;
    if (num_members < 1 || num_members > kMaxMembers) return PZ_E_SIZE;
    for (int p = 0; p < num_members; ++p)
        if (!members[p].w1 || !members[p].b1 || !members[p].w2 || !members[p].b2 || !members[p].w3 || !members[p].b3) return PZ_E_NULL;
    if ((order_p1 && !first_p1) || (order_p2 && !first_p2)) return PZ_E_NULL;
    const bool any_head = head_p1 || head_p2, any_val = val_p1 || val_p2;
    if (n < 0 || n > kMaxRows || in_features < 1 || in_features > PZ_NET_MAX_IN || (hidden != 32 && hidden != 64 && hidden != 128) ||
        num_actions < 2 || num_actions > PZ_POOL_ACT_MAX_ACTIONS || out_features < num_actions || out_features > PZ_NET_MAX_OUT ||
        (any_val && out_features == num_actions) || bad_pitch(n, in_features, obs_pitch) || (any_head && bad_pitch(n, out_features, head_pitch)))
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
    for (int p = 0; p < num_members; ++p)
        for (const float* q : {members[p].w1, members[p].b1, members[p].w2, members[p].b2, members[p].w3, members[p].b3})
            if (misaligned(q, 4)) return PZ_E_ALIGN;
    const void* words[] = {order_p1, first_p1, order_p2, first_p2, logp_p1, logp_p2, ent_p1, ent_p2, val_p1, val_p2, head_p1, head_p2};
    for (const void* p : words)
        if (misaligned(p, 4)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    Args a{{obs_p1, obs_p2}, {order_p1, order_p2}, {first_p1, first_p2}, {act_p1, act_p2}, {logp_p1, logp_p2}, {ent_p1, ent_p2}, {val_p1, val_p2},
           {head_p1, head_p2}, step_dev, step, first_game, n, obs_pitch, any_head ? head_pitch : 0, in_features, out_features, num_actions,
           obs_format, action_format, num_members, (int32_t)(n / G + num_members), (int32_t)((n + G - 1) / G), (uint32_t)seed,
           (uint32_t)(seed >> 32), {}};
    for (int p = 0; p < kMaxMembers; ++p) a.members[p] = members[p < num_members ? p : 0];  // (the entries behind P are never used)
    const unsigned sides = second ? 2 : 1;
    return activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, sides, stream)
                                         : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, sides, stream);
}

}  // extern "C"
