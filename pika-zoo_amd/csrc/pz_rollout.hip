// libpikazoo_rollout.so: k policy steps in ONE launch -- the policy net's forward, the categorical draw and the game's frame
// k times over, the state in registers, the observation rows handed from the frame to the net through LDS (C ABI and the
// definition, by reference to the launches it replaces: include/pikazoo_rollout.h; the shape and its reasons: DESIGN.md 4.27).
//
// One workgroup of four waves per 64 games.  Wave 0 owns the games, one lane each: it loads the state once, stages both
// agents' observation rows into LDS in front of every step, runs the frame (frame_head / frame_tail of pz_physics.hpp, human
// vs human: no barrier inside) on the two sampled actions and stores the state once.  All four waves flush the staged rows to
// slab t and then take one 32-row tile of the net each -- wave w: agent w >> 1, rows 32 (w & 1) .. + 31 -- through
// tile_layers (csrc/pz_mlp_tile.hpp) with the LDS rows as its observations (the same float32 conversions of the same
// words: pz_mlp_forward's bits), the head through the wave's own LDS image into the row code of csrc/pz_policy_rows.hpp as
// pz_act.hip runs it (pz_sample_actions' bits), and hand the actions to wave 0 through LDS.
//   * Two workgroup barriers per step: rows staged -> [flush, net, draw] -> actions posted -> [frame].  Every wave of every
//     workgroup runs the step loop k times (a wave without a live row computes on +0 and stores nothing), so the barriers
//     sit in a loop whose trip count is the same for all waves.
//   * The rows are read from the LDS staging, never back from global memory: their stores carry the non-temporal hint.
//   * The image is written and read by one wave: wavefront-scope fences around a wave barrier, as in pz_act.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_net.h"
#include "pikazoo_policy.h"
#include "pikazoo_rollout.h"
#include "pz_mlp_tile.hpp"
#include "pz_policy_rows.hpp"
#include "pz_step_io.hpp"

namespace pz_rollout {

using namespace pz_mlp;

constexpr int kGames = pz::kLanes;                 // games per workgroup: the lanes of wave 0
constexpr int kRowWords = kGames * PZ_OBS_DIM;     // one agent's staged rows
constexpr int kRowVecs = kRowWords / 4;            // ... in 16-byte pieces
constexpr int64_t kMaxGames = (int64_t)0xFFFFFFFFu / (PZ_STATE_WORDS * 4);  // one launch's descriptors are 32-bit

struct Args {
    int32_t* state;
    int64_t n, stride, pitch;
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
    const float* w3[2];
    const float* b3[2];
    char* obs[2];
    void* act[2];
    float* logp[2];
    float* val[2];
    float* ent[2];
    char* rew[2];
    uint8_t* term;
    void* episode_stats;
    unsigned long long* episodes_done;
    const uint64_t* step_dev;
    uint64_t step;
    int64_t first_game;
    int32_t k, O, A, action_format, separate;
    uint32_t key0, key1;
    pz_config cfg;
};

__host__ __device__ constexpr int image_stride(int O) { return O | 1; }
// floats of LDS: [parameter set(s)][rows of agent 1][rows of agent 2][four images][actions of agent 1, agent 2]
__host__ __device__ constexpr int64_t rollout_lds_floats(int H, int O, int sets)
{
    return (int64_t)sets * lds_floats(PZ_OBS_DIM, H, O) + 2 * kRowWords + kWaves * kTileRows * image_stride(O) + 2 * kGames;
}

// the workgroup's 64 staged rows of one agent to its span of slab t (`span`: the span's first byte, `bytes`: from there to
// the end of the slab's n rows -- the rows of games past n are dropped by the range check)
__device__ __forceinline__ void flush_group(const int32_t* __restrict__ rows, const char* span, uint32_t bytes, bool by16, int tid)
{
    const pz::Rsrc dst = pz::make_rsrc(span, bytes);
    if (by16) {  // (slabs 16-byte aligned: pitch % 4 == 0)
        const pz::u32x4* src4 = reinterpret_cast<const pz::u32x4*>(rows);
#pragma unroll
        for (int v = tid; v < kRowVecs; v += kThreads) __builtin_amdgcn_raw_buffer_store_b128(src4[v], dst, (uint32_t)v * 16u, 0, pz::kObsAux);
    } else {
        for (int v = tid; v < kRowWords; v += kThreads)
            __builtin_amdgcn_raw_buffer_store_b32((unsigned int)rows[v], dst, (uint32_t)v * 4u, 0, pz::kObsAux);
    }
}

template <int H, int ACT>
__global__ __launch_bounds__(kThreads) void rollout_policy_kernel(const Args a)
{
    extern __shared__ float lds[];
    constexpr int K = PZ_OBS_DIM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int set_floats = lds_floats(K, H, a.O), stride = image_stride(a.O);
    const Staged s0 = staged_at<H>(lds, K, a.O);
    const Staged s1 = a.separate ? staged_at<H>(lds + set_floats, K, a.O) : s0;
    float* behind = lds + (a.separate ? 2 : 1) * set_floats;
    int32_t* rows0 = reinterpret_cast<int32_t*>(behind);  // (16-byte aligned: every term of lds_floats is a multiple of 4)
    int32_t* rows1 = rows0 + kRowWords;
    float* image = behind + 2 * kRowWords + wave * kTileRows * stride;  // this wave's alone
    float* mine = image + j * stride;
    int32_t* posted = reinterpret_cast<int32_t*>(behind + 2 * kRowWords + kWaves * kTileRows * stride);  // [2][kGames]

    // the parameters, global -> LDS in operand order, once per workgroup (the first barrier of the step loop orders them)
    stage_parameters<H>(s0, a.w1[0], a.b1[0], a.w2[0], a.b2[0], a.w3[0], a.b3[0], K, a.O, tid);
    if (a.separate) stage_parameters<H>(s1, a.w1[1], a.b1[1], a.w2[1], a.b2[1], a.w3[1], a.b3[1], K, a.O, tid);

    // ---- wave 0: the games ---------------------------------------------------------------------------------------------
    const int64_t g0 = (int64_t)blockIdx.x * kGames, i = g0 + lane;
    const bool live = i < a.n, frames = wave == 0;
    const uint32_t n32 = (uint32_t)a.n;
    const pz::StateIO io{pz::make_rsrc(a.state, (uint32_t)(a.stride * (PZ_STATE_WORDS * 4))), (uint32_t)a.stride * 4u, (uint32_t)i * 4u};
    const bool as_float = a.cfg.ballpos_reward != 0 || a.cfg.normal_state_mode != 0;
    const bool with_stats = a.episode_stats != nullptr && a.cfg.episode_stats_mode != 0;  // uniform
    const pz::StatsIO sio = pz::make_stats_io(a.episode_stats, with_stats, a.stride, i);
    pz::Game g{};
    const pz::RngId id = pz::make_rng_id(a.cfg, live ? i : 0);
    pz::FlightLut lut{};  // human vs human: nothing is looked up
    lut.has_landing = lut.has_power_hit = false;
    lut.landing = lut.power_hit = pz::make_rsrc(nullptr, 0u);
    const pz::ScoutLink link{nullptr, nullptr, nullptr};
    pz::EpisodeStats st{0.0, 0.0, 0};
    if (frames && live) {
        pz::load_game(g, io);
        if (with_stats) sio.load(st);
    }
    const pz::ZoneTable zones = pz::park_zone_table(a.cfg);
    unsigned int finished = 0;  // a game can end once per step

    // ---- every wave: its tile of the net ---------------------------------------------------------------------------------
    const int side = wave >> 1, row = kTileRows * (wave & 1) + j;
    const int64_t gi = g0 + row;
    const bool row_live = gi < a.n;
    const Staged& s = side ? s1 : s0;
    const int32_t* rows = side ? rows1 : rows0;
    const int obs_format = a.cfg.normalize_obs == PZ_OBS_F32_NORM ? PZ_NET_OBS_FLOAT32 : PZ_NET_OBS_INT32;
    const uint64_t T0 = a.step + (a.step_dev ? *a.step_dev : 0);
    const bool by16 = (a.pitch & 3) == 0;
    const uint32_t span_bytes = (uint32_t)(a.n - g0) * pz::kRowBytes;  // (n - g0 >= 1: the grid covers n)

    // rows staged by wave 0 -> slab t, and this wave's tile: the head into the image, then the row code on the lanes of half 0
    auto rows_and_net = [&](int64_t t, bool draw) {
        if (frames && live) pz::stage_obs<pz::kRows4>(g, rows0, rows1, lane, a.cfg.normalize_obs);
        __syncthreads();  // the rows (and, the first time, the parameters) are in place
        const int64_t slab = (t * a.pitch + g0) * pz::kRowBytes;
        flush_group(rows0, a.obs[0] + slab, span_bytes, by16, tid);
        flush_group(rows1, a.obs[1] + slab, span_bytes, by16, tid);
        f32x16 y[2];
        tile_layers<H, ACT>(s, rows, row, row_live, K, a.O, K, obs_format, lane, y);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * u + acc_row(r, half);
                if (o < a.O) mine[o] = y[u][r];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (half == 0 && row_live) {
            const int64_t at = t * a.pitch + gi;
            if (draw) {
                const pz_policy::RowStats rs = pz_policy::row_stats(mine, a.A);
                const float u = pz_policy::draw_uniform((uint64_t)(a.first_game + gi), T0 + (uint64_t)t, a.key0, a.key1, side);
                const int act = pz_policy::draw_action(mine, a.A, rs, u);
                if (a.action_format == PZ_POLICY_ACTION_INT32)
                    ((int32_t*)a.act[side])[at] = act;
                else
                    ((int64_t*)a.act[side])[at] = act;
                a.logp[side][at] = pz_policy::action_log_prob(mine, a.A, rs, act);
                if (a.ent[side]) a.ent[side][at] = rs.bad ? __uint_as_float(0x7FC00000u) : rs.H;
                posted[side * kGames + row] = act;
            }
            a.val[side][at] = mine[a.A];
        }
        // this step's reads of the image before the next step's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    for (int32_t t = 0; t < a.k; ++t) {
        rows_and_net(t, true);
        __syncthreads();  // both actions of every game are posted; every wave is done with the rows
        if (frames) {
            const int a1 = posted[lane], a2 = posted[kGames + lane];
            const bool resets = live && g.e.game_ended != 0 && a.cfg.auto_reset != 0;  // this frame resets the game in place
            bool frozen = false;
            const int reward = pz::step_games<false, false>(g, a.cfg, id, a1, a2, live, frozen, rows0, lane, lut, link);
            finished += (unsigned int)(live && g.e.game_ended && !frozen);
            const pz::Rewards rw = pz::shape_rewards(a.cfg, g, reward, frozen, &zones);
            if (with_stats) pz::stats_update(st, a.cfg, rw, resets, live && !frozen, as_float);
            if (live) {
                const int64_t at = (int64_t)t * a.pitch;
                const pz::Rsrc rew1 = pz::make_rsrc(a.rew[0] + at * 4, n32 * 4u), rew2 = pz::make_rsrc(a.rew[1] + at * 4, n32 * 4u);
                const pz::Rsrc term = pz::make_rsrc(a.term + at, n32);
                __builtin_amdgcn_raw_buffer_store_b32(as_float ? __float_as_uint(rw.f1) : (unsigned int)rw.i1, rew1, io.voff, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(as_float ? __float_as_uint(rw.f2) : (unsigned int)rw.i2, rew2, io.voff, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b8((unsigned char)g.e.game_ended, term, (uint32_t)i, 0, 0);
            }
        }
    }
    rows_and_net(a.k, false);  // slab k of the observations and the bootstrap values: no draw, no step consumed

    if (frames) {
        if (live) {
            pz::store_game(g, io);
            if (with_stats) sio.store(st);
        }
        if (a.episodes_done != nullptr) {  // one atomic per workgroup
            unsigned int total = finished;
            for (int off = kGames / 2; off > 0; off >>= 1) total += __shfl_down(total, off, kGames);
            if (lane == 0 && total != 0) atomicAdd(a.episodes_done, (unsigned long long)total);
        }
    }
}

template <int H, int ACT>
static int launch(const Args& a, void* stream)
{
    const size_t bytes = (size_t)rollout_lds_floats(H, a.O, a.separate ? 2 : 1) * sizeof(float);
    if (bytes > 64 * 1024) {  // above the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void*)rollout_policy_kernel<H, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
    }
    const unsigned blocks = (unsigned)((a.n + kGames - 1) / kGames);
    hipLaunchKernelGGL((rollout_policy_kernel<H, ACT>), dim3(blocks), dim3(kThreads), bytes, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

template <int ACT>
static int launch_hidden(const Args& a, int hidden, void* stream)
{
    switch (hidden) {
        case 32:
            return launch<32, ACT>(a, stream);
        case 64:
            return launch<64, ACT>(a, stream);
        default:
            return launch<128, ACT>(a, stream);
    }
}

}  // namespace pz_rollout

using namespace pz_rollout;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kRolloutBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_rollout_build_id(void) { return kRolloutBuildIdRecord + 12; }

int pz_rollout_abi_version(void) { return PZ_ROLLOUT_ABI_VERSION; }

int pz_rollout_policy(int32_t* state, int64_t n, int64_t stride, const pz_config* cfg, int32_t k, int32_t hidden, int32_t out_features,
                      int32_t activation, const float* w1_p1, const float* b1_p1, const float* w2_p1, const float* b2_p1, const float* w3_p1,
                      const float* b3_p1, const float* w1_p2, const float* b1_p2, const float* w2_p2, const float* b2_p2, const float* w3_p2,
                      const float* b3_p2, uint64_t seed, int64_t first_game, uint64_t step, const uint64_t* step_dev, int32_t action_format,
                      int64_t pitch, void* obs_p1, void* obs_p2, void* act_p1, void* act_p2, float* logp_p1, float* logp_p2, float* val_p1,
                      float* val_p2, float* ent_p1, float* ent_p2, void* rew_p1, void* rew_p2, uint8_t* terminated, void* episode_stats,
                      unsigned long long* episodes_done, void* stream)
{
    if (!state || !cfg || !w1_p1 || !b1_p1 || !w2_p1 || !b2_p1 || !w3_p1 || !b3_p1 || !obs_p1 || !obs_p2 || !act_p1 || !act_p2 || !logp_p1 ||
        !logp_p2 || !val_p1 || !val_p2 || !rew_p1 || !rew_p2 || !terminated)
        return PZ_E_NULL;
    const void* second[] = {w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2};
    int present = 0;
    for (const void* p : second) present += p != nullptr;
    if (present != 0 && present != 6) return PZ_E_NULL;
    if ((ent_p1 != nullptr) != (ent_p2 != nullptr)) return PZ_E_NULL;
    const int32_t A = cfg->simplify_action ? 13 : 18;
    if (n < 0 || stride < n || stride > kMaxGames || k < 1 || k > PZ_ROLLOUT_MAX_STEPS || (hidden != 32 && hidden != 64 && hidden != 128) ||
        out_features != A + 1 || pitch < n || pitch > kMaxGames)
        return PZ_E_SIZE;
    if (first_game < 0 || step > ((uint64_t)1 << 62) - (uint64_t)k) return PZ_E_SIZE;
    if (cfg->winning_score < 1 || cfg->serve_mode < 0 || cfg->serve_mode > 2 || cfg->normal_state_mode < 0 || cfg->normal_state_mode > 2 ||
        cfg->episode_stats_mode < 0 || cfg->episode_stats_mode > 2 || cfg->normalize_obs < PZ_OBS_I32 || cfg->normalize_obs > PZ_OBS_BF16_NORM ||
        (cfg->packed_state != 0 && cfg->packed_state != 1))
        return PZ_E_CONFIG;
    // out of scope: computer players, the packed state, 2-byte rows
    if (cfg->p1_computer || cfg->p2_computer || cfg->packed_state || cfg->normalize_obs > PZ_OBS_F32_NORM) return PZ_E_CONFIG;
    if ((activation != PZ_NET_ACT_TANH && activation != PZ_NET_ACT_RELU) || !pz_policy::known_action_format(action_format)) return PZ_E_CONFIG;
    const uintptr_t ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    using pz_mlp::misaligned;
    if (misaligned(act_p1, ab) || misaligned(act_p2, ab) || misaligned(episode_stats, 8) || misaligned(episodes_done, 8) || misaligned(step_dev, 8))
        return PZ_E_ALIGN;
    const void* words[] = {state, w1_p1, b1_p1, w2_p1, b2_p1, w3_p1, b3_p1, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2, obs_p1, obs_p2,
                           logp_p1, logp_p2, val_p1, val_p2, ent_p1, ent_p2, rew_p1, rew_p2};
    for (const void* p : words)
        if (misaligned(p, 4)) return PZ_E_ALIGN;
    const bool separate = present != 0 && w1_p2 != w1_p1;  // (agent 1's own pointers again: one set serves both)
    if ((size_t)rollout_lds_floats(hidden, out_features, separate ? 2 : 1) * sizeof(float) > (size_t)kLdsBytes) return PZ_E_SIZE;
    if (n == 0) return PZ_OK;
    const int q = separate ? 1 : 0;
    const float* sets[2][6] = {{w1_p1, b1_p1, w2_p1, b2_p1, w3_p1, b3_p1}, {w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2}};
    const Args a{state, n, stride, pitch, {sets[0][0], sets[q][0]}, {sets[0][1], sets[q][1]}, {sets[0][2], sets[q][2]}, {sets[0][3], sets[q][3]},
                 {sets[0][4], sets[q][4]}, {sets[0][5], sets[q][5]}, {(char*)obs_p1, (char*)obs_p2}, {act_p1, act_p2}, {logp_p1, logp_p2},
                 {val_p1, val_p2}, {ent_p1, ent_p2}, {(char*)rew_p1, (char*)rew_p2}, terminated, episode_stats, episodes_done, step_dev, step,
                 first_game, k, out_features, A, action_format, separate ? 1 : 0, (uint32_t)seed, (uint32_t)(seed >> 32), *cfg};
    return activation == PZ_NET_ACT_TANH ? launch_hidden<PZ_NET_ACT_TANH>(a, hidden, stream) : launch_hidden<PZ_NET_ACT_RELU>(a, hidden, stream);
}

}  // extern "C"
