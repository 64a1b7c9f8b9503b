// pz_dispatch.hpp -- which step-kernel instantiation a launch of the C ABI runs, and so which instantiations exist.
//
// choose_step_kernel() is the whole choice, from what a launch knows on the host: the entry point, k, n, the pz_config
// words it reads, whether a statistics pointer and the power-hit table are passed.  The library builds exactly its
// image over the inputs that can tell two launches apart (step_kernel_image): an instantiation no launch reaches is
// never built.  Host C++17 without HIP: tests/test_dispatch_host.py compiles it with the host compiler
// (tests/dispatch_shim.cpp) and holds it against tests/kernel_matrix.py dispatch(), the independent restatement.
#pragma once
#include <stdint.h>

#include "pikazoo_hip.h"

namespace pz {

// template argument MODE of the step kernels, the entry point: pz_step / pz_step_bound, pz_step_random,
// pz_rollout_random, pz_step_many (pz_kernels.hip: step_kernel)
enum StepMode { kActions = 0, kRandom = 1, kRollout = 2, kTape = 3 };
// template argument SCOUT: the second wave beside a single-wave frame (pz_physics.hpp: frame_head / frame_tail)
enum ScoutMode { kNoScout = 0, kScoutLoads = 1, kScoutPosted = 2 };
// the kernel families, in the order of their bits in a diagnostic subset (pz_kernels.hip: dev_keep)
enum StepFamily { kStepPairKernel = 0, kRolloutPairKernel = 1, kStepKernel = 2 };

// Kernel selection by batch size (interleaved A/B on MI355X, tools/ab.py; us per pz_step launch):
//   human-vs-human, pair kernel | single-wave kernel, both with the changed-only write-back:
//       65 536: 7.58 | 8.01    131 072: 11.1 | 11.5    262 144: 22.4 | 23.8    294 912: 25.3 | 26.5
//      524 288: 47.2 | 46.5    1 048 576: 93.9 | 90.6      (single-wave without changed-only at 65 536: 8.52)
//   player 2 = computer, scout kernel | single-wave changed-only:   262 144: 36.5 | 38.2    524 288: 70.3 | 66.4
constexpr int64_t kTwoWaveMaxLanes = 393216;  // below: two waves per workgroup (pair kernels / scout)
//   the changed-only write-back also pays in the scout kernel (65 536: 14.3 | 14.65 without, 262 144: 35.6 | 36.6)
//   and is used by every launch that writes the state back after ONE frame; a trajectory launch writes it once
//   per k frames, where the plain write-back is always right.

// An instantiation: its family and that family's template arguments (the others false / 0)
//   step_pair_kernel<AI1, AI2, PACKED, RANDOM = MODE == kRandom>
//   rollout_pair_kernel<AI1, AI2, MODE, PACKED, OBS16, PLAIN>
//   step_kernel<AI1, AI2, MODE, SPARSE, SCOUT, PACKED, OBS16, PLAIN>
struct StepKernel {
    int family;
    bool ai1, ai2;
    int mode;
    bool sparse;
    int scout;
    bool packed, obs16, plain;
};

// one number per instantiation, below kStepKernelCodes: the index of the launcher's kernel table
constexpr int kStepKernelCodes = 3 * 2 * 2 * 4 * 2 * 3 * 2 * 2 * 2;
constexpr int code(const StepKernel& s)
{
    return (((((((s.family * 2 + s.ai1) * 2 + s.ai2) * 4 + s.mode) * 2 + s.sparse) * 3 + s.scout) * 2 + s.packed) * 2 +
            s.obs16) * 2 + s.plain;
}

constexpr bool is_packed(const pz_config& cfg) { return (cfg.packed_state & 1) != 0; }
// formats 2 - 6 (int16 / float16 / bfloat16): 70-byte rows, an even number per frame (the OBS16 instantiations)
constexpr bool rows16(int format) { return format >= PZ_OBS_I16; }
// no fused wrapper, no episode statistics, raw integer rows: what the PLAIN k-frame kernels are compiled for
// (`stats`: a statistics pointer is passed -- a statistics mode without one is PLAIN)
constexpr bool is_plain(const pz_config& cfg, bool stats)
{
    return cfg.simplify_action == 0 && cfg.ballpos_reward == 0 && cfg.normal_state_mode == 0 &&
           (cfg.normalize_obs == PZ_OBS_I32 || cfg.normalize_obs == PZ_OBS_I16) && (cfg.episode_stats_mode == 0 || !stats);
}

// the families a diagnostic build switches off (pz_diagnostic.hpp, bits 1 - 3); the product: none
struct LeftOut {
    bool pair_kernel, rollout_pair_kernel, scout_wave;
};

// `mode`: StepMode; `power_hit`: the power-hit table is passed.  With it the six candidate flights of a deciding player
// are one gather, and the frame splits by player; the landing table is optional on top of it (without it the kernel
// predicts the landing point itself), so a launch with the landing table alone dispatches like one without tables.
constexpr StepKernel choose_step_kernel(int mode, int k, int64_t n, const pz_config& cfg, bool stats, bool power_hit,
                                        LeftOut off = {})
{
    const bool ai1 = cfg.p1_computer != 0, ai2 = cfg.p2_computer != 0, human = !ai1 && !ai2;
    const bool packed = is_packed(cfg), obs16 = rows16(cfg.normalize_obs), plain = is_plain(cfg, stats);
    const bool traj = mode == kRollout || mode == kTape, small = n < kTwoWaveMaxLanes;
    // one frame on two waves per 64 games, split by player: below the switch, and the packed format at every size (524 288
    // games, us per launch, pair | single wave: human 30.25 | 30.13, player 2 = computer 38.6 | 40.6; 1 048 576 human
    // 56.2 | 56.4).  One frame of the on-device random policy is the same launch with the policy's Philox block in place
    // of the two action loads (65 536 games: 8.2 -> 7.0 us against the single-wave kernel)
    if (!off.pair_kernel && (mode == kActions || (mode == kRandom && k == 1)) && (small || packed) && (power_hit || human))
        return {kStepPairKernel, ai1, ai2, mode, false, kNoScout, packed, false, false};
    // the k-frame launches on two waves below the switch: a computer player on the table (interleaved A/B, us per frame
    // at k = 32: 3.49 vs 4.34 on one wave), human vs human on 2-byte rows only (2.47 -> 2.23; on int32 rows one wave is
    // at the write ceiling already: 3.62 on two waves vs 3.63 on one, profiles/r03_experiments/).  No packed PLAIN form
    if (!off.rollout_pair_kernel && traj && small && ((power_hit && !human) || (human && obs16)))
        return {kRolloutPairKernel, ai1, ai2, mode, false, kNoScout, packed, obs16, plain && !packed};
    // one wave per 64 games from here on; the packed format: no scout (a computer player's flights are computed in the
    // frame's wave), no PLAIN form
    if (packed) return {kStepKernel, ai1, ai2, mode, false, kNoScout, true, traj && obs16, false};
    const bool sparse = !traj;  // the changed-only write-back (one frame per launch)
    // a computer player without the table below the switch: a scout wave computes its flights beside the frame
    if (!off.scout_wave && small && !power_hit && !human)
        return {kStepKernel, ai1, ai2, mode, sparse, mode == kActions ? kScoutLoads : kScoutPosted, false, traj && obs16, false};
    // the k-frame launches run their PLAIN form where the configuration allows -- but for the human-vs-human rollout: it
    // runs at the write ceiling of its two tensors either way, and its PLAIN form measured 0.6 - 3.4 % slower (k = 32:
    // 2.91 vs 2.81 - 2.84 us per frame, profiles/r04_experiments/ab_rollout_hh_*), while the tape kernel and every
    // computer-player launch gain 1 - 2 % from theirs
    return {kStepKernel, ai1, ai2, mode, sparse, kNoScout, false, traj && obs16, traj && plain && !(mode == kRollout && human)};
}

// The instantiations: the image of choose_step_kernel over entry point x {k = 1, k > 1} x {below, at/above the switch}
// x state format x row width x PLAIN or fused x power-hit table x player mix, each once
constexpr int kStepInputs = 4 * 2 * 2 * 2 * 2 * 2 * 2 * 4;
struct StepKernelSet {
    StepKernel at[kStepInputs];
    int count;
};
constexpr StepKernelSet step_kernel_image(LeftOut off = {})
{
    StepKernelSet set{};
    bool seen[kStepKernelCodes] = {};
    for (int i = 0; i < kStepInputs; ++i) {
        pz_config cfg{};
        cfg.p1_computer = i & 1;
        cfg.p2_computer = (i >> 1) & 1;
        cfg.packed_state = (i >> 2) & 1;
        cfg.normalize_obs = ((i >> 3) & 1) ? PZ_OBS_I16 : PZ_OBS_I32;
        cfg.simplify_action = (i >> 4) & 1;  // a fused wrapper
        const int k = ((i >> 5) & 1) ? 2 : 1;
        const int64_t n = ((i >> 6) & 1) ? kTwoWaveMaxLanes : 0;
        const StepKernel s = choose_step_kernel(i >> 8, k, n, cfg, false, ((i >> 7) & 1) != 0, off);
        if (!seen[code(s)]) {
            seen[code(s)] = true;
            set.at[set.count++] = s;
        }
    }
    return set;
}

}  // namespace pz
