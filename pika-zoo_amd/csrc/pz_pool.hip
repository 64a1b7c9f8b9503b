// libpikazoo_pool.so: the policy net's forward pass for a pool of parameter sets, every row through the set of its own pool
// member, in ONE launch -- and the plan that groups the rows by member (C ABI and the definition: include/pikazoo_pool.h; the
// shape and its reasons: DESIGN.md 4.21).
//
// The tile body is pz_mlp_tile.hpp's, the code pz_mlp_forward runs: same k order, same operand permutation, same bits.  What
// is new here is which rows a tile holds and which parameter set is staged under it.  The plan's `order` lists the rows member
// by member in groups of G = 128 slots (pads are -1), so the four waves of a workgroup always share a member: a workgroup
// takes a contiguous range of groups, finds a group's member by comparing its first slot with the P + 1 words of `first`
// (held in LDS), and re-stages the parameters only when the member changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_pool.h"
#include "pz_mlp_tile.hpp"

namespace pz_pool {

using namespace pz_mlp;

constexpr int G = PZ_POOL_GROUP_ROWS;
constexpr int kMaxMembers = PZ_POOL_MAX_MEMBERS;
constexpr int kFirstWords = 32;  // the P + 1 words of `first` behind the staged parameter set, padded
static_assert(G == kWaves * kTileRows, "a group is one tile per wave of the workgroup");

// ---- the plan ----------------------------------------------------------------------------------------------------------------
constexpr int kPlanWaves = 16;
constexpr int kPlanThreads = 64 * kPlanWaves;

// the member of row i, -1 if it is not in [0, P)
__device__ __forceinline__ int load_member(const void* p, int format, int i, int P)
{
    if (format == PZ_POOL_MEMBER_UINT8) {
        const int v = ((const uint8_t*)p)[i];
        return v < P ? v : -1;
    }
    if (format == PZ_POOL_MEMBER_INT32) {
        const uint32_t v = ((const uint32_t*)p)[i];
        return v < (uint32_t)P ? (int)v : -1;
    }
    const uint64_t v = ((const uint64_t*)p)[i];
    return v < (uint64_t)P ? (int)v : -1;
}

__device__ __forceinline__ int ballot_count(bool pred) { return __popcll(__builtin_amdgcn_ballot_w64(pred)); }

// A stable counting sort by one workgroup.  Wave w owns the rows [w * run, (w + 1) * run) and walks them 64 at a time, so
// the loads are contiguous; a row's rank among the rows of its member inside the wave's 64 is a ballot and a population
// count.  Pass 1 counts per (member, wave); the scan orders those counts member-major; pass 2 writes.
__global__ __launch_bounds__(kPlanThreads) void pool_plan_kernel(const void* members, int format, int n, int P, int capacity, int32_t* order,
                                                               int32_t* first, int32_t* errors)
{
    __shared__ int32_t s_count[kMaxMembers][kPlanWaves];  // pass 1: the counts; behind the scan: the rows of the member in earlier waves
    __shared__ int32_t s_total[kMaxMembers];
    __shared__ int32_t s_first[kMaxMembers + 1];
    __shared__ int32_t s_bad[kPlanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int run = ((n + kPlanWaves - 1) / kPlanWaves + 63) & ~63;
    const int lo = min(n, wave * run), hi = min(n, lo + run);

    int cnt[kMaxMembers] = {};
    int bad = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const int m = i < hi ? load_member(members, format, i, P) : -2;
#pragma unroll
        for (int p = 0; p < kMaxMembers; ++p) cnt[p] += ballot_count(m == p);
        bad += ballot_count(m == -1);
    }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < kMaxMembers; ++p) s_count[p][wave] = cnt[p];
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (tid < kMaxMembers) {
        int sum = 0;
        for (int w = 0; w < kPlanWaves; ++w) {
            const int c = s_count[tid][w];
            s_count[tid][w] = sum;
            sum += c;
        }
        s_total[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        int at = 0, invalid = 0;
        for (int p = 0; p < P; ++p) {
            s_first[p] = at;
            first[p] = at;
            at += (s_total[p] + G - 1) / G * G;
        }
        s_first[P] = at;
        first[P] = at;
        for (int w = 0; w < kPlanWaves; ++w) invalid += s_bad[w];
        errors[0] = invalid;
    }
    __syncthreads();

    int pos[kMaxMembers];
#pragma unroll
    for (int p = 0; p < kMaxMembers; ++p) pos[p] = p < P ? s_first[p] + s_count[p][wave] : 0;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const int m = i < hi ? load_member(members, format, i, P) : -2;
        int at = -1;
#pragma unroll
        for (int p = 0; p < kMaxMembers; ++p) {
            const uint64_t mask = __builtin_amdgcn_ballot_w64(m == p);
            if (m == p) at = pos[p] + __popcll(mask & below);
            pos[p] += __popcll(mask);
        }
        if (at >= 0 && at < capacity) order[at] = i;  // (inside `order` even if `members` changed between the two walks)
    }
    for (int p = 0; p < P; ++p) {
        const int end = s_first[p + 1] - s_first[p];
        for (int j = s_total[p] + tid; j < end; j += kPlanThreads) order[s_first[p] + j] = -1;
    }
    for (int j = s_first[P] + tid; j < capacity; j += kPlanThreads) order[j] = -1;
}

// ---- the forward -------------------------------------------------------------------------------------------------------------
struct Args {
    const void* obs[2];
    void* out[2];
    const int32_t* order[2];
    const int32_t* first[2];
    int64_t n, obs_pitch, out_pitch;
    int32_t K, O, obs_format, out_format, P, plan_groups, plain_groups;
    pz_pool_member members[kMaxMembers];
};

template <int H, int ACT>
__global__ __launch_bounds__(kThreads, H <= 64 ? 2 : 1) void mlp_forward_pool_kernel(const Args a)
{
    extern __shared__ float lds[];
    const int side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, O = a.O, P = a.P;
    const Staged s = staged_at<H>(lds, K, O);
    int32_t* s_first = (int32_t*)(lds + lds_floats(K, H, O));
    const int32_t* order = a.order[side];
    const void* obs = a.obs[side];
    void* out = a.out[side];

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
        const int slot = slot0 + wave * kTileRows + (lane & 31);
        const int64_t row = order ? (int64_t)order[slot] : (int64_t)slot;
        const bool live = row >= 0 && row < a.n;  // (a pad of the plan is -1: handled like a row behind the last one)
        tile_forward<H, ACT>(s, obs, out, row, live, K, O, a.obs_pitch, a.out_pitch, a.obs_format, a.out_format, lane);
    }
}

template <int H, int ACT>
static int launch(const Args& a, unsigned sides, void* stream)
{
    const size_t bytes = ((size_t)lds_floats(a.K, H, a.O) + kFirstWords) * sizeof(float);
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_forward_pool_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    int64_t blocks = 1;
    for (unsigned side = 0; side < sides; ++side) blocks = max(blocks, (int64_t)(a.order[side] ? a.plan_groups : a.plain_groups));
    blocks = min(blocks, grid_cap(bytes, sides));
    hipLaunchKernelGGL((mlp_forward_pool_kernel<H, ACT>), dim3((unsigned)blocks, sides), dim3(kThreads), bytes, (hipStream_t)stream, a);
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

}  // namespace pz_pool

using namespace pz_pool;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kPoolBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_pool_build_id(void) { return kPoolBuildIdRecord + 12; }

int pz_pool_abi_version(void) { return PZ_POOL_ABI_VERSION; }

int64_t pz_pool_capacity(int64_t n, int32_t num_members)
{
    if (n < 0 || n > kMaxRows || num_members < 1 || num_members > kMaxMembers) return -1;
    return (n / G + num_members) * G;
}

int pz_pool_plan(const void* members, int32_t member_format, int64_t n, int32_t num_members, int32_t* order, int32_t* first, int32_t* errors,
                 void* stream)
{
    if (!order || !first || !errors || (!members && n > 0)) return PZ_E_NULL;
    if (n < 0 || n > kMaxRows || num_members < 1 || num_members > kMaxMembers) return PZ_E_SIZE;
    if (member_format < PZ_POOL_MEMBER_UINT8 || member_format > PZ_POOL_MEMBER_INT64) return PZ_E_CONFIG;
    const uintptr_t mb = member_format == PZ_POOL_MEMBER_UINT8 ? 1 : member_format == PZ_POOL_MEMBER_INT32 ? 4 : 8;
    if (misaligned(members, mb) || misaligned(order, 4) || misaligned(first, 4) || misaligned(errors, 4)) return PZ_E_ALIGN;
    hipLaunchKernelGGL(pool_plan_kernel, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, members, (int)member_format, (int)n, (int)num_members,
                       (int)pz_pool_capacity(n, num_members), order, first, errors);
    return (int)hipGetLastError();
}

int pz_mlp_forward_pool(const void* obs_p1, const void* obs_p2, int32_t obs_format, int64_t n, int32_t in_features, int64_t obs_pitch,
                        int32_t hidden, int32_t out_features, int32_t activation, const pz_pool_member* members, int32_t num_members,
                        const int32_t* order_p1, const int32_t* first_p1, const int32_t* order_p2, const int32_t* first_p2, void* out_p1,
                        void* out_p2, int32_t out_format, int64_t out_pitch, void* stream)
{
    if (!obs_p1 || !out_p1 || !members) return PZ_E_NULL;
    const bool second = obs_p2 != nullptr;
    if (second != (out_p2 != nullptr) || (!second && (order_p2 || first_p2))) return PZ_E_NULL;
    if (num_members < 1 || num_members > kMaxMembers) return PZ_E_SIZE;
    for (int p = 0; p < num_members; ++p)
        if (!members[p].w1 || !members[p].b1 || !members[p].w2 || !members[p].b2 || !members[p].w3 || !members[p].b3) return PZ_E_NULL;
    if ((order_p1 && !first_p1) || (order_p2 && !first_p2)) return PZ_E_NULL;
    if (n < 0 || n > kMaxRows || in_features < 1 || in_features > PZ_NET_MAX_IN || (hidden != 32 && hidden != 64 && hidden != 128) ||
        out_features < 1 || out_features > PZ_NET_MAX_OUT || bad_pitch(n, in_features, obs_pitch) || bad_pitch(n, out_features, out_pitch))
        return PZ_E_SIZE;
    if (obs_format < PZ_NET_OBS_INT32 || obs_format > PZ_NET_OBS_BFLOAT16 || out_format < PZ_NET_OUT_FLOAT32 ||
        out_format > PZ_NET_OUT_BFLOAT16 || (activation != PZ_NET_ACT_TANH && activation != PZ_NET_ACT_RELU))
        return PZ_E_CONFIG;
    const uintptr_t xb = obs_format == PZ_NET_OBS_INT32 || obs_format == PZ_NET_OBS_FLOAT32 ? 4 : 2;
    const uintptr_t yb = out_format == PZ_NET_OUT_FLOAT32 ? 4 : 2;
    if (misaligned(obs_p1, xb) || misaligned(obs_p2, xb) || misaligned(out_p1, yb) || misaligned(out_p2, yb)) return PZ_E_ALIGN;
    for (int p = 0; p < num_members; ++p)
        for (const float* q : {members[p].w1, members[p].b1, members[p].w2, members[p].b2, members[p].w3, members[p].b3})
            if (misaligned(q, 4)) return PZ_E_ALIGN;
    if (misaligned(order_p1, 4) || misaligned(first_p1, 4) || misaligned(order_p2, 4) || misaligned(first_p2, 4)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    Args a{{obs_p1, obs_p2}, {out_p1, out_p2}, {order_p1, order_p2}, {first_p1, first_p2}, n, obs_pitch, out_pitch, in_features, out_features,
           obs_format, out_format, num_members, (int32_t)(n / G + num_members), (int32_t)((n + G - 1) / G), {}};
    for (int p = 0; p < kMaxMembers; ++p) a.members[p] = members[p < num_members ? p : 0];  // (the entries behind P are never used)
    const unsigned sides = second ? 2 : 1;
    return activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, sides, stream)
                                         : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, sides, stream);
}

}  // extern "C"
