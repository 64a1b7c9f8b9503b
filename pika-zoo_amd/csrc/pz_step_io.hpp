// pz_step_io.hpp -- what a launch that runs the frame needs around it: the state columns' accessor and the whole-game
// load / store, the env stream's identity of a lane, the observation rows' staging in every format, the fused reward
// pipeline and the episode statistics.  Shared by pz_kernels.hip (libpikazoo_hip.so) and pz_rollout.hip
// (libpikazoo_rollout.so); the text was moved here from pz_kernels.hip unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pz_physics.hpp"
#include "pz_memory.hpp"

namespace pz {

// One game's column accessor: wave-uniform descriptor + column pitch, per-lane byte offset.
struct StateIO {
    Rsrc rsrc;
    uint32_t pitch;  // bytes between columns = stride * 4 (uniform)
    uint32_t voff;   // this lane's byte offset inside a column = lane index * 4
    __device__ __forceinline__ int ld(int col) const
    {
        return (int)__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (uint32_t)col * pitch, 0);
    }
    __device__ __forceinline__ void st(int col, int v) const
    {
        __builtin_amdgcn_raw_buffer_store_b32((unsigned int)v, rsrc, voff, (uint32_t)col * pitch, kStateAux);
    }
};

// ---- state columns <-> registers -----------------------------------------------------------
__device__ __forceinline__ void load_player(Player& p, const StateIO& io, int c0)
{
    p.x = io.ld(c0 + PZ_P_X);
    p.y = io.ld(c0 + PZ_P_Y);
    p.yv = io.ld(c0 + PZ_P_Y_VELOCITY);
    p.state = io.ld(c0 + PZ_P_STATE);
    p.frame = io.ld(c0 + PZ_P_FRAME_NUMBER);
    p.arm = io.ld(c0 + PZ_P_ARM_SWING_DIRECTION);
    p.delay = io.ld(c0 + PZ_P_DELAY_BEFORE_NEXT_FRAME);
    p.dive = io.ld(c0 + PZ_P_DIVING_DIRECTION);
    p.lying = io.ld(c0 + PZ_P_LYING_DOWN_DURATION_LEFT);
    p.coll = io.ld(c0 + PZ_P_IS_COLLISION_WITH_BALL_HAPPENED);
    p.bold = io.ld(c0 + PZ_P_COMPUTER_BOLDNESS);
    p.standby = io.ld(c0 + PZ_P_COMPUTER_WHERE_TO_STAND_BY);
    p.hitprev = io.ld(c0 + PZ_P_POWER_HIT_KEY_IS_DOWN_PREVIOUS);
}

__device__ __forceinline__ void load_game(Game& g, const StateIO& io)
{
    // env + ball first: the frame starts with the round bookkeeping and the ball-world step
    g.e.round_ended = io.ld(PZ_E_ROUND_ENDED);
    g.e.game_ended = io.ld(PZ_E_GAME_ENDED);
    g.e.rng = (uint32_t)io.ld(PZ_E_RNG_DRAW_COUNTER);
    g.e.s1 = io.ld(PZ_E_SCORE_P1);
    g.e.s2 = io.ld(PZ_E_SCORE_P2);
    g.e.p2serve = io.ld(PZ_E_IS_PLAYER2_SERVE);
    g.b.x = io.ld(PZ_B_X);
    g.b.y = io.ld(PZ_B_Y);
    g.b.xv = io.ld(PZ_B_X_VELOCITY);
    g.b.yv = io.ld(PZ_B_Y_VELOCITY);
    g.b.power = io.ld(PZ_B_IS_POWER_HIT);
    g.b.px = io.ld(PZ_B_PREVIOUS_X);
    g.b.py = io.ld(PZ_B_PREVIOUS_Y);
    g.b.ppx = io.ld(PZ_B_PREVIOUS_PREVIOUS_X);
    g.b.ppy = io.ld(PZ_B_PREVIOUS_PREVIOUS_Y);
    g.b.rot = io.ld(PZ_B_FINE_ROTATION);
    g.b.ex = io.ld(PZ_B_EXPECTED_LANDING_POINT_X);
    g.b.punch = io.ld(PZ_B_PUNCH_EFFECT_X);
    load_player(g.p1, io, 0);
    load_player(g.p2, io, PZ_P_WORDS);
}

__device__ __forceinline__ void store_player(const Player& p, const StateIO& io, int c0)
{
    io.st(c0 + PZ_P_X, p.x);
    io.st(c0 + PZ_P_Y, p.y);
    io.st(c0 + PZ_P_Y_VELOCITY, p.yv);
    io.st(c0 + PZ_P_STATE, p.state);
    io.st(c0 + PZ_P_FRAME_NUMBER, p.frame);
    io.st(c0 + PZ_P_ARM_SWING_DIRECTION, p.arm);
    io.st(c0 + PZ_P_DELAY_BEFORE_NEXT_FRAME, p.delay);
    io.st(c0 + PZ_P_DIVING_DIRECTION, p.dive);
    io.st(c0 + PZ_P_LYING_DOWN_DURATION_LEFT, p.lying);
    io.st(c0 + PZ_P_IS_COLLISION_WITH_BALL_HAPPENED, p.coll);
    io.st(c0 + PZ_P_COMPUTER_BOLDNESS, p.bold);
    io.st(c0 + PZ_P_COMPUTER_WHERE_TO_STAND_BY, p.standby);
    io.st(c0 + PZ_P_POWER_HIT_KEY_IS_DOWN_PREVIOUS, p.hitprev);
}

// skip_ex: the lane's expected_landing_point_x is stored by the scout wave (step_games<..., SCOUT>)
__device__ __forceinline__ void store_game(const Game& g, const StateIO& io, bool skip_ex = false)
{
    store_player(g.p1, io, 0);
    store_player(g.p2, io, PZ_P_WORDS);
    io.st(PZ_B_X, g.b.x);
    io.st(PZ_B_Y, g.b.y);
    io.st(PZ_B_X_VELOCITY, g.b.xv);
    io.st(PZ_B_Y_VELOCITY, g.b.yv);
    io.st(PZ_B_IS_POWER_HIT, g.b.power);
    io.st(PZ_B_PREVIOUS_X, g.b.px);
    io.st(PZ_B_PREVIOUS_Y, g.b.py);
    io.st(PZ_B_PREVIOUS_PREVIOUS_X, g.b.ppx);
    io.st(PZ_B_PREVIOUS_PREVIOUS_Y, g.b.ppy);
    io.st(PZ_B_FINE_ROTATION, g.b.rot);
    if (!skip_ex) io.st(PZ_B_EXPECTED_LANDING_POINT_X, g.b.ex);
    io.st(PZ_B_PUNCH_EFFECT_X, g.b.punch);
    io.st(PZ_E_SCORE_P1, g.e.s1);
    io.st(PZ_E_SCORE_P2, g.e.s2);
    io.st(PZ_E_IS_PLAYER2_SERVE, g.e.p2serve);
    io.st(PZ_E_ROUND_ENDED, g.e.round_ended);
    io.st(PZ_E_GAME_ENDED, g.e.game_ended);
    io.st(PZ_E_RNG_DRAW_COUNTER, (int32_t)g.e.rng);
}

__device__ __forceinline__ RngId make_rng_id(const pz_config& cfg, int64_t lane_index)
{
    const uint64_t gid = (uint64_t)(cfg.env_id_base + lane_index);
    return RngId{(uint32_t)gid, (uint32_t)(gid >> 32), make_rolling_key(cfg.seed)};
}

// ---- observation pack: _get_obs (pikazoo_env.py:576-624) ------------------------------------
// Row layout: player(13) | opponent(13) | ball(9).  Rows go to LDS at stride 35 words (odd,
// so the 64 lanes of a ds_write_b32 hit 32 distinct banks twice = conflict-free), then the
// wave copies the contiguous 64x35-word span to HBM with 16-byte lanes.
// F: the staged word's format (enum pz_obs_format; int16 rows stage what int32 rows do, flush_rows16 narrows them).
// PZ_OBS_F32_NORM: NormalizeObservation fused (normalize_observation.py:22,30): every entry becomes
// float32 (v - low) / (high - low) with the bounds of pikazoo_env.py:485-562.  The reference
// divides in float64; for these small integers the correctly rounded float32 quotient is the
// float32 rounding of that double, so an IEEE float division reproduces it bit for bit.
// The float16 / bfloat16 formats: the float32 value of format 0 (exact) or 1, rounded to nearest even by a plain cast
// (v_cvt_f16_f32 / v_cvt_pk_bf16_f32; never the round-toward-zero v_cvt_pkrtz_f16_f32), its 16-bit pattern
// zero-extended into the staged dword -- the 2-byte flushes keep the low half of every staged dword.
constexpr bool obs_norm(int f) { return f == PZ_OBS_F32_NORM || f == PZ_OBS_F16_NORM || f == PZ_OBS_BF16_NORM; }
template <int F>
__device__ __forceinline__ int32_t obs_word(int v, int low, int range)
{
    if constexpr (F == PZ_OBS_I32 || F == PZ_OBS_I16) {
        return v;
    } else {
        const float f = !obs_norm(F) ? (float)v : (range == 1) ? (float)(v - low) : (float)(v - low) / (float)range;
        if constexpr (F == PZ_OBS_F32_NORM)
            return (int32_t)__float_as_uint(f);
        else if constexpr (F == PZ_OBS_F16 || F == PZ_OBS_F16_NORM)
            return (int32_t)(uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
        else
            return (int32_t)(uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f);
    }
}

template <int F>
__device__ __forceinline__ void player_words(const Player& p, int32_t (&w)[13])
{
    w[0] = obs_word<F>(p.x, 32, 368);
    w[1] = obs_word<F>(p.y, 108, 136);
    w[2] = obs_word<F>(p.yv, -15, 31);
    w[3] = obs_word<F>(p.dive, -1, 2);
    w[4] = obs_word<F>(p.lying, -2, 5);
    w[5] = obs_word<F>(p.frame, 0, 4);
    w[6] = obs_word<F>(p.delay, 0, 4);
    w[7] = obs_word<F>(p.state == 0, 0, 1);
    w[8] = obs_word<F>(p.state == 1, 0, 1);
    w[9] = obs_word<F>(p.state == 2, 0, 1);
    w[10] = obs_word<F>(p.state == 3, 0, 1);
    w[11] = obs_word<F>(p.state == 4, 0, 1);
    w[12] = obs_word<F>(p.hitprev, 0, 1);
}

template <int F>
__device__ __forceinline__ void stage_obs_t(const Game& g, int32_t* __restrict__ s1, int32_t* __restrict__ s2, int lane)
{
    int32_t p1[13], p2[13], bw[9];
    player_words<F>(g.p1, p1);
    player_words<F>(g.p2, p2);
    bw[0] = obs_word<F>(g.b.x, 20, 412);
    bw[1] = obs_word<F>(g.b.y, 0, 252);
    bw[2] = obs_word<F>(g.b.px, 0, 432);
    bw[3] = obs_word<F>(g.b.py, 0, 252);
    bw[4] = obs_word<F>(g.b.ppx, 0, 432);
    bw[5] = obs_word<F>(g.b.ppy, 0, 252);
    bw[6] = obs_word<F>(g.b.xv, -20, 40);
    bw[7] = obs_word<F>(g.b.yv, -124, 248);
    bw[8] = obs_word<F>(g.b.power, 0, 1);
    int32_t* r1 = s1 + lane * PZ_OBS_DIM;
    int32_t* r2 = s2 + lane * PZ_OBS_DIM;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        r1[k] = p1[k];
        r1[13 + k] = p2[k];
        r2[k] = p2[k];
        r2[13 + k] = p1[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        r1[26 + k] = bw[k];
        r2[26 + k] = bw[k];
    }
}

// one agent's row: [own player | opponent | ball] (pair kernel: each wave packs its own agent's tensor)
template <int F>
__device__ __forceinline__ void stage_one_obs_t(const Player& me, const Player& opp, const Ball& b,
                                                int32_t* __restrict__ dst, int lane)
{
    int32_t pa[13], pb[13];
    player_words<F>(me, pa);
    player_words<F>(opp, pb);
    int32_t* r = dst + lane * PZ_OBS_DIM;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        r[k] = pa[k];
        r[13 + k] = pb[k];
    }
    r[26] = obs_word<F>(b.x, 20, 412);
    r[27] = obs_word<F>(b.y, 0, 252);
    r[28] = obs_word<F>(b.px, 0, 432);
    r[29] = obs_word<F>(b.py, 0, 252);
    r[30] = obs_word<F>(b.ppx, 0, 432);
    r[31] = obs_word<F>(b.ppy, 0, 252);
    r[32] = obs_word<F>(b.xv, -20, 40);
    r[33] = obs_word<F>(b.yv, -124, 248);
    r[34] = obs_word<F>(b.power, 0, 1);
}

// The staging of the run-time format `fmt` (cfg.normalize_obs: wave-uniform, a config scalar).  ROWS: the formats the
// calling kernel can meet -- the trajectory kernels compile the row width in (OBS16), so theirs carry the staging of
// their own width only.  The single-frame kernels carry all of them: +0.9 % on the headline, +1.2 % on config 3
// (profiles/obs_formats_ab.log); staging format 0 / 1 and narrowing the row in place instead measured +1.0 % there and
// made the 16-bit single-frame launches a third slower.
enum ObsRows { kRows4 = 1, kRows2 = 2, kRowsAny = 3 };  // 140-byte rows (formats 0, 1) / 70-byte rows (2 - 6) / both
template <int ROWS = kRowsAny>
__device__ __forceinline__ void stage_obs(const Game& g, int32_t* __restrict__ s1, int32_t* __restrict__ s2, int lane,
                                          int fmt)
{
    if ((ROWS & kRows4) && fmt == PZ_OBS_F32_NORM)
        stage_obs_t<PZ_OBS_F32_NORM>(g, s1, s2, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_F16)
        stage_obs_t<PZ_OBS_F16>(g, s1, s2, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_BF16)
        stage_obs_t<PZ_OBS_BF16>(g, s1, s2, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_F16_NORM)
        stage_obs_t<PZ_OBS_F16_NORM>(g, s1, s2, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_BF16_NORM)
        stage_obs_t<PZ_OBS_BF16_NORM>(g, s1, s2, lane);
    else  // int32 / int16: the raw integers
        stage_obs_t<PZ_OBS_I32>(g, s1, s2, lane);
}

template <int ROWS = kRowsAny>
__device__ __forceinline__ void stage_one_obs(const Player& me, const Player& opp, const Ball& b,
                                              int32_t* __restrict__ dst, int lane, int fmt)
{
    if ((ROWS & kRows4) && fmt == PZ_OBS_F32_NORM)
        stage_one_obs_t<PZ_OBS_F32_NORM>(me, opp, b, dst, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_F16)
        stage_one_obs_t<PZ_OBS_F16>(me, opp, b, dst, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_BF16)
        stage_one_obs_t<PZ_OBS_BF16>(me, opp, b, dst, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_F16_NORM)
        stage_one_obs_t<PZ_OBS_F16_NORM>(me, opp, b, dst, lane);
    else if ((ROWS & kRows2) && fmt == PZ_OBS_BF16_NORM)
        stage_one_obs_t<PZ_OBS_BF16_NORM>(me, opp, b, dst, lane);
    else
        stage_one_obs_t<PZ_OBS_I32>(me, opp, b, dst, lane);
}

// The reward pipeline of one frame (see pz_config in the header): the reference's wrapper
// stack RewardInNormalState / RewardByBallPosition in either order, fused.
struct Rewards {
    int i1, i2;      // the env's own +1/-1/0 (pikazoo_env.py:217-228)
    float f1, f2;    // after the fused reward wrappers
};

// one entry of RewardByBallPosition's table in a per-lane register, through an opaque move.  Indexing the kernel
// argument with the (per-lane) zone is a global load from the kernarg segment -- and the compiler turns a select
// over the eight scalars back into exactly that load -- whose wait also drains every store issued before it (gfx9
// counts loads and stores in one in-order vmcnt): a dependent memory round trip in front of the reward store.
__device__ __forceinline__ float zone_reward(const pz_config& cfg, int k)
{
    float v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(cfg.additional_reward[k]));
    return v;
}

// The k-frame kernels hold the table in eight per-lane registers for the whole launch (`parked`): as scalars the
// compiler carries it around the frame loop in eight SGPRs of a budget of ~100, spills it and brings all eight back
// through v_readlane in front of every use (a lone wave per SIMD has hundreds of VGPRs to spare).
struct ZoneTable {
    float z[8];
};
__device__ __forceinline__ ZoneTable park_zone_table(const pz_config& cfg)
{
    ZoneTable t;
#pragma unroll
    for (int k = 0; k < 8; ++k) t.z[k] = zone_reward(cfg, k);
    return t;
}

__device__ __forceinline__ Rewards shape_rewards(const pz_config& cfg, const Game& g, int reward, bool frozen,
                                                 const ZoneTable* parked = nullptr)
{
    Rewards r{reward, -reward, (float)reward, (float)(-reward)};
    if (frozen) return r;
    if (cfg.normal_state_mode == 1) {  // reward_in_normal_state.py:12-14, inside RewardByBallPosition
        r.f1 = (r.f1 == 0.0f) ? cfg.normal_state_reward : r.f1;
        r.f2 = (r.f2 == 0.0f) ? cfg.normal_state_reward : r.f2;
    }
    if (cfg.ballpos_reward) {  // reward_by_ball_position.py:22-29: zone from the post-step ball position
        // additional_reward[i * 4 + zone], zone = (y > y_line) + 2 * (x >= x_line)
        const bool low = g.b.y > cfg.y_line, right = g.b.x >= cfg.x_line;
        auto z = [&](int k) { return parked != nullptr ? parked->z[k] : zone_reward(cfg, k); };
        r.f1 += right ? (low ? z(3) : z(2)) : (low ? z(1) : z(0));
        r.f2 += right ? (low ? z(7) : z(6)) : (low ? z(5) : z(4));
    }
    if (cfg.normal_state_mode == 2) {  // the wrapper outside RewardByBallPosition
        r.f1 = (r.f1 == 0.0f) ? cfg.normal_state_reward : r.f1;
        r.f2 = (r.f2 == 0.0f) ? cfg.normal_state_reward : r.f2;
    }
    return r;
}

// RecordEpisodeStatistics (record_episode_statistics.py:27-40): per game the two running returns as float64 -- the
// reference sums Python floats (:31), and so do we: float32 rewards are widened before the add, the env's own +-1/0
// sum exactly -- and the episode length.  Buffer layout (pz_step in the header): double[2][stride], int32[stride].
struct EpisodeStats {
    double r1, r2;
    int len;
};
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct StatsIO {
    Rsrc rsrc;
    uint32_t stride;  // games per row
    uint32_t lane;    // this lane's game index inside the batch
    __device__ __forceinline__ double ld_ret(int agent) const
    {
        const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lane * 8u, (uint32_t)agent * stride * 8u, 0);
        return __hiloint2double((int)w.y, (int)w.x);
    }
    __device__ __forceinline__ void st_ret(int agent, double v) const
    {
        const u32x2 w = {(unsigned int)__double2loint(v), (unsigned int)__double2hiint(v)};
        __builtin_amdgcn_raw_buffer_store_b64(w, rsrc, lane * 8u, (uint32_t)agent * stride * 8u, 0);
    }
    __device__ __forceinline__ int ld_len() const
    {
        return (int)__builtin_amdgcn_raw_buffer_load_b32(rsrc, lane * 4u, stride * 16u, 0);
    }
    __device__ __forceinline__ void st_len(int v) const
    {
        __builtin_amdgcn_raw_buffer_store_b32((unsigned int)v, rsrc, lane * 4u, stride * 16u, 0);
    }
    __device__ __forceinline__ void load(EpisodeStats& st) const
    {
        st.r1 = ld_ret(0);
        st.r2 = ld_ret(1);
        st.len = ld_len();
    }
    __device__ __forceinline__ void store(const EpisodeStats& st) const
    {
        st_ret(0, st.r1);
        st_ret(1, st.r2);
        st_len(st.len);
    }
};

// `enabled` false: an empty descriptor (loads return 0, stores are dropped)
__device__ __forceinline__ StatsIO make_stats_io(const void* episode_stats, bool enabled, int64_t stride, int64_t lane)
{
    return StatsIO{make_rsrc(episode_stats, enabled ? (uint32_t)(stride * 20) : 0u), (uint32_t)stride, (uint32_t)lane};
}

__device__ __forceinline__ void stats_update(EpisodeStats& st, const pz_config& cfg, const Rewards& r, bool was_reset,
                                             bool counted, bool as_float)
{
    if (was_reset) st = EpisodeStats{0.0, 0.0, 0};  // reset() zeroes the sums (:23-25)
    if (!counted) return;
    const bool raw = cfg.episode_stats_mode == 1 || !as_float;
    st.r1 += raw ? (double)r.i1 : (double)r.f1;
    st.r2 += raw ? (double)r.i2 : (double)r.f2;
    st.len += 1;
}

}  // namespace pz
