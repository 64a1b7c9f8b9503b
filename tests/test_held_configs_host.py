"""The rules of tests/held_configs.py (CPU only): what tests/test_gpu_held_configs.py launches on the two frame-skip
kernel families, and that every one of those launches bites.

Every instantiation of ``hold_kernel`` / ``held_traj_kernel`` receives every level of every factor that applies to it, in
at least MIN_PER_KERNEL configurations; across each family every pair of levels of two factors occurs; a configuration's
row format agrees with its instantiation's OBS16.  The levels an instantiation takes are written down here by hand, apart
from held_configs.domain.  Then, on the CPU judge alone (tests/frame_skip_judge.py) and for every configuration below the
size switch: games end inside the launch, with hold >= 2 inside a repeat, come back one slab later under auto_reset, a
shaped launch puts a running game's ball exactly on a line, the cancelling table under RewardInNormalState has a point
cancelled and replaced, the large ids wrap -- asserted, so that no GPU test passes vacuously.  The whole module takes
about 25 s on 8 threads (the judge: 10 - 50 ms per configuration).
"""
import collections
import dataclasses
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

import held_configs as hc
import kernel_configs as kc
import kernel_matrix as km
from frame_skip_judge import HeldOracle

REPO = Path(__file__).resolve().parent.parent
CONFIGS, DOMAINS = hc.generated()
STRUCTURES = {s.kernel: s for s in hc.structures()}
# every other kernel of the code object: none of them steps a game
NOT_STEP_KERNELS = {"build_landing_table_kernel", "build_power_hit_table_kernel", "count_misfits_kernel", "init_kernel",
                    "observe_kernel", "pack_state_kernel", "probe_write_kernel", "random_actions_kernel", "render_kernel",
                    "reset_kernel", "scenery_init_kernel", "scenery_tick_kernel", "scenery_track_kernel",
                    "unpack_state_kernel"}


def _expected_domain(kernel):
    """By hand, from the instantiation's name: hold_kernel<AI1, AI2, PACKED> takes every factor of kernel_configs with
    every action element type and holds of 2 / 4 / 7; held_traj_kernel<AI1, AI2, MODE, PACKED, OBS16> takes int32 tapes
    alone, the row formats of its width, holds {2, 3, 4, 8} and k {1, 5, 20, 70}.  The table mode is a factor where a
    computer player exists."""
    family, args = kernel.rstrip(">").split("<")
    args = args.split(", ")
    dom = {f: set(v) for f, v in kc.FACTORS.items()}
    if family == "hold_kernel":
        dom["hold"] = {2, 4, 7}
    else:
        del dom["action_format"]
        dom["obs_format"] = {2, 3, 4, 5, 6} if args[4] == "true" else {0, 1}
        dom["hold"], dom["k"] = {2, 3, 4, 8}, {1, 5, 20, 70}
    if "true" in args[:2]:
        dom["tables"] = {"both", "power_hit", "none"}
    return dom


def _level_gaps(configs, domains):
    got = collections.defaultdict(lambda: collections.defaultdict(set))
    count = collections.Counter()
    for c in configs:
        count[c.kernel] += 1
        for f, lv in c.levels().items():
            got[c.kernel][f].add(lv)
    gaps = []
    for kernel, dom in domains.items():
        if count[kernel] < kc.MIN_PER_KERNEL:
            gaps.append((kernel, "configurations", count[kernel]))
        gaps += [(kernel, f, sorted(set(levels) - got[kernel][f], key=str)) for f, levels in dom.items()
                 if set(levels) - got[kernel][f]]
    return gaps


def _pair_gaps(configs, domains):
    gaps = {}
    for fam in hc.FAMILIES:
        side = [c for c in configs if c.kernel.startswith(fam)]
        need = kc.required_pairs([dom for kernel, dom in domains.items() if kernel.startswith(fam)])
        have = set()
        for c in side:
            have |= set(itertools.combinations(sorted(c.levels().items()), 2))
        gaps[fam] = sorted(need - have, key=str)
    return gaps


def test_the_forty_instantiations_and_their_domains():
    assert len(hc.KERNELS) == 40 and len(hc.hold_kernels()) == 8 and hc.held_traj_kernels() < hc.KERNELS
    assert set(DOMAINS) == hc.KERNELS == set(STRUCTURES)
    for kernel, dom in DOMAINS.items():
        assert {f: set(v) for f, v in dom.items()} == _expected_domain(kernel), kernel
    # the factors are kernel_configs' own objects, not copies that could drift
    assert hc.FACTORS is kc.FACTORS and hc.SHAPING is kc.SHAPING and hc.IDS is kc.IDS and hc.SEED == kc.SEED
    assert hc.NORMAL_STATE_REWARD == kc.NORMAL_STATE_REWARD and hc.MIN_PER_KERNEL == kc.MIN_PER_KERNEL == 4


def test_every_instantiation_gets_every_level_of_every_factor():
    assert {c.kernel for c in CONFIGS} == hc.KERNELS
    assert not _level_gaps(CONFIGS, DOMAINS)


def test_every_pair_of_levels_occurs_in_each_family():
    gaps = _pair_gaps(CONFIGS, DOMAINS)
    assert not any(gaps.values()), gaps
    for fam in hc.FAMILIES:  # and the pairs are many: every factor's every level is in the family
        seen = collections.defaultdict(set)
        for c in CONFIGS:
            if c.kernel.startswith(fam):
                for f, lv in c.levels().items():
                    seen[f].add(lv)
        want = {f: set(v) for f, v in kc.FACTORS.items() if f != "action_format" or fam == "hold_kernel<"}
        assert {f: seen[f] for f in want} == want, fam
        assert seen["tables"] == {"both", "power_hit", "none"}


def test_every_configuration_names_the_instantiation_its_structure_dispatches():
    names = [c.name for c in hc.configs()]
    assert len(names) == len(set(names))
    tf = {False: "false", True: "true"}
    for c in hc.configs():
        # launch_held / launch_held_traj (pz_kernels.hip): who plays, the state format; the launch mode and the row width
        if c.entry == "held":
            want = f"hold_kernel<{tf[c.p1]}, {tf[c.p2]}, {tf[c.packed]}>"
            assert c.k == hc.STEP_LAUNCHES and c.hold in hc.STEP_HOLDS
        else:
            mode = {"rollout": 2, "many": 3}[c.entry]
            want = f"held_traj_kernel<{tf[c.p1]}, {tf[c.p2]}, {mode}, {tf[c.packed]}, {tf[c.obs_format >= 2]}>"
            assert c.action_format == "i32" and (c.hold, c.k) in set(itertools.product(hc.HOLDS, hc.KS))
        assert c.kernel == want, c.name
        assert c.n == (km.N_ABOVE if c.above else km.N_BELOW) and c.n % 8 == 0 and c.n % 64 != 0
        assert c.stride in (c.n, c.n + 64)
        assert c.tables == "none" or c.p1 or c.p2
    above = [c for c in hc.configs() if c.above]
    assert sorted(c.entry for c in above) == ["held", "many", "rollout"] and hc.configs()[:len(CONFIGS)] == CONFIGS
    assert not any(c.above for c in CONFIGS)
    # hold_kernel at a stride of exactly n on a ragged n, and every action element type on every instantiation
    for kernel in hc.hold_kernels():
        mine = [c for c in CONFIGS if c.kernel == kernel]
        assert any(c.stride_pad == 0 for c in mine) and {c.action_format for c in mine} == set(kc.ACTION_FORMATS)


def test_plant_states_is_the_recipe_of_the_single_frame_configurations():
    c = CONFIGS[0]
    planted, over = kc.plant_states(c)
    assert np.array_equal(planted, c.start_state()) and planted.shape == (44, c.n)
    for ws in (1, 3, 15):
        planted, over = kc.plant_states(dataclasses.replace(c, winning_score=ws))
        s1, s2 = planted[38], planted[39]
        assert 0.08 < over.mean() < 0.17
        assert np.array_equal(over, planted[42] != 0) and np.array_equal(over, planted[41] != 0)
        assert np.array_equal(over, np.maximum(s1, s2) == ws), "over: a winner at the winning score, and only there"
        assert ((np.maximum(s1, s2) == ws - 1) & ~over).mean() >= 0.2, "a quarter of the games one point from the end"


def test_every_configuration_bites_on_the_judge_alone():
    hc.measure.cache_clear()  # measured here, not remembered from the generator
    last = collections.Counter()
    for c in CONFIGS:
        f = hc.measure(c)
        assert f.ended_inside + f.ended_last > 0, (c.name, "no game terminates inside the launch")
        if c.hold >= 2:
            assert f.ended_inside > 0, (c.name, "no game ends inside a repeat")
        if c.auto_reset and c.k >= 5:
            assert f.revived > 0, (c.name, "no game terminated in one slab and running in the next")
        if c.shaped:
            assert f.on_line, (c.name, "no post-step ball of a running game on x_line or y_line")
        if c.shaping == "cancel" and c.normal_state_mode == 2:
            assert f.cancelled, (c.name, "no point cancelled by the table and replaced by RewardInNormalState")
        if c.ids == "large":
            assert c.env_id_base >= 1 << 32 and (c.env_id_base + c.n) >> 32 > c.env_id_base >> 32, c.name
            if c.entry == "rollout" and c.k >= 3:
                assert c.t0 < 1 << 32 < c.t0 + c.k, c.name
        assert hc.misses(c, f) == []
        last[c.kernel] += f.ended_last > 0
    assert all(last[kernel] > 0 for kernel in hc.KERNELS), sorted(k for k in hc.KERNELS if not last[k])
    # the policy index counts policy steps, in 64 bits: every pz_rollout_random_held instantiation takes it across 2^32
    crossing = {c.kernel for c in CONFIGS if c.entry == "rollout" and c.ids == "large" and c.k >= 3}
    assert crossing == {s.kernel for s in hc.structures() if s.entry == "rollout"} and len(crossing) == 16
    # the sharp cases exist: the cancelling table replaced by RewardInNormalState in both families, a statistics mode
    # without a pointer and statistics of the env's reward under a float reward stack on every instantiation's family
    for fam in hc.FAMILIES:
        side = [c for c in CONFIGS if c.kernel.startswith(fam)]
        assert any(c.shaping == "cancel" and c.normal_state_mode == 2 for c in side)
        assert any(c.episode_stats == "1-null" for c in side)
        assert any(c.episode_stats == 1 and (c.shaped or c.normal_state_mode) for c in side)
        assert any(c.serve == "random" and c.ids == "large" for c in side)


def test_the_conditions_bite():
    """misses() says so when a launch is too short for a game to come back, or never meets the line"""
    c = next(c for c in CONFIGS if c.shaped and c.auto_reset and c.entry != "held" and c.k >= 5)
    f = hc.measure(c)
    assert hc.misses(c, dataclasses.replace(f, revived=0)) == ["no game terminated in one slab and running in the next"]
    assert hc.misses(c, dataclasses.replace(f, on_line=False)) == ["no post-step ball of a running game on a shaping line"]
    assert "no game ends inside a repeat" in hc.misses(c, dataclasses.replace(f, ended_inside=0))
    assert len(hc.misses(c, hc.Facts(0, 0, 0, False, False))) >= 4


@pytest.mark.parametrize("what", ["level", "pair"])
def test_dropping_a_level_breaks_the_coverage(what):
    configs = list(CONFIGS)
    if what == "level":
        kernel = "held_traj_kernel<true, false, 3, true, true>"
        for i, c in enumerate(configs):
            if c.kernel == kernel and c.serve == "random":
                configs[i] = dataclasses.replace(c, serve="alternate")
        assert (kernel, "serve", ["random"]) in _level_gaps(configs, DOMAINS)
    else:
        victims = [i for i, c in enumerate(configs) if c.entry == "held" and c.shaping == "cancel" and c.hold == 7]
        assert victims
        for i in victims:
            configs[i] = dataclasses.replace(configs[i], hold=4)
        assert (("hold", 7), ("shaping", "cancel")) in _pair_gaps(configs, DOMAINS)["hold_kernel<"]


def test_generation_is_deterministic():
    again, _ = hc.generated.__wrapped__(hc.SEED)
    assert again == CONFIGS


def test_the_per_frame_callback_changes_nothing_in_the_judge(oracle):
    c = next(c for c in CONFIGS if c.shaped and c.entry == "many" and c.k == 5)
    plain, watched = hc.make_judge(oracle, c), hc.make_judge(oracle, c)
    assert isinstance(plain, HeldOracle) and plain.on_frame is None
    frames = []
    watched.on_frame = lambda j, env, frozen: frames.append((j, [r.copy() for r in env.rew], frozen.copy()))
    for t in range(c.k):
        a = hc.policy(oracle, c, t)
        (o1, r1, t1), (o2, r2, t2) = plain.step(*a), watched.step(*a)
        assert all(np.array_equal(x, y) for x, y in zip(o1 + r1 + [t1], o2 + r2 + [t2]))
        mine = frames[-c.hold:]
        assert [j for j, _, _ in mine] == list(range(c.hold))
        for p in range(2):  # the slab's reward is the frame rewards summed in frame order from +0.0
            total = np.zeros(c.n, np.float32)
            for _, rew, _ in mine:
                total = total + rew[p]
            assert np.array_equal(total.view(np.int32), r2[p].view(np.int32))
        for _, rew, frozen in mine:  # a frame that found the game frozen adds exactly 0
            assert not rew[0][frozen].any() and not rew[1][frozen].any()
    assert np.array_equal(plain.state, watched.state)
    assert (plain.ended_inside, plain.ended_last) == (watched.ended_inside, watched.ended_last) and plain.ended_inside > 0
    assert len(frames) == c.k * c.hold


def test_no_shipped_step_kernel_lacks_a_configuration_sweep():
    """The code object's ``pz::`` kernels are the 137 of tests/kernel_matrix.py, the 40 here, and the kernels that step
    no game: a step kernel added without a systematic sweep (tests/kernel_configs.py or tests/held_configs.py) fails."""
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    sys.path.insert(0, str(REPO / "tools"))
    import build as pz_build
    import kernel_digest

    lib = pz_build.build()
    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    shipped = {name.replace("pz::", "", 1) for name in kernel_digest.kernels(lib) if name.startswith("pz::")}
    step = {name for name in shipped if name.split("<")[0] not in NOT_STEP_KERNELS}
    assert not km.KERNELS & hc.KERNELS
    assert step == km.KERNELS | hc.KERNELS, (sorted(step - km.KERNELS - hc.KERNELS), sorted((km.KERNELS | hc.KERNELS) - step))
    assert len(step) == 177 and {c.kernel for c in kc.configs()} | {c.kernel for c in CONFIGS} == step
