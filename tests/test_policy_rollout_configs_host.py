"""The rules of tests/policy_rollout_configs.py (CPU only): what tests/test_gpu_policy_rollout_configs.py launches on the six
``rollout_policy_kernel<H, ACT>``, that every one of those launches bites, and that the comparison the GPU test uses would
notice a kernel that is subtly wrong.

Every instantiation receives every level of every factor that applies to it, in at least MIN_PER_KERNEL configurations; every
compatible pair of levels of two factors occurs; every level of the issue's table appears.  The levels an instantiation takes
and the pairs that cannot occur are written down here by hand, apart from the generator's own predicates.  Then, on the CPU
restatement of the whole launch alone (the C oracle for the frame, the float32 restatements of the net and of the draw): games
end before the last slab, are reset and move on under auto_reset or stay frozen and unpaid without it, games are over at entry,
a shaped launch puts a running game's ball exactly on a line, the cancelling table has a point cancelled and replaced, the
large ids have games and steps on both sides of each of their three wraps, a masked head would have drawn a masked action, and
no slab holds more ambiguous rows than the judge's cap -- asserted, and printed per configuration, so that no GPU test passes
vacuously.  Last, ``compare()`` passes the restatement of every configuration and rejects each of the eleven mutants.
"""
import collections
import contextlib
import dataclasses
import io
import itertools

import numpy as np
import pytest

import act_judge as AJ
import kernel_configs as kc
import policy_judge as J
import policy_rollout_configs as pc

CONFIGS, DOMAINS = pc.generated()
ALL = {
    "winning_score": {1, 3, 15}, "serve": {"winner", "alternate", "random"}, "auto_reset": {1, 0}, "simplify_action": {0, 1},
    "shaping": {"off", "default", "shifted", "degenerate", "cancel"}, "normal_state_mode": {0, 1, 2}, "episode_stats": {0, 1, 2, "1-null"},
    "obs_format": {0, 1}, "action_format": {"i32", "i64"}, "entropy": {1, 0}, "stride": {"n", "n+64"}, "pitch": {"n", "n+4", "n+3"},
    "step": {"value", "device"}, "head": {"random", "masked", "bad"}, "ids": {"small", "large"},
    "shape": {(36, 8), (68, 8), (132, 8), (132, 1), (67, 5)}, "weights": {"shared", "separate"},
}
# by hand: the pairs of levels no launch can hold (module docstring of policy_rollout_configs: what cannot be combined)
IMPOSSIBLE = ({(("head", "bad"), ("weights", "shared")), (("pitch", "n+4"), ("shape", (67, 5))), (("ids", "large"), ("shape", (36, 8))),
               (("ids", "large"), ("shape", (132, 1)))})


def quiet(call, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args)


def _expected_domain(kernel):
    hidden = int(kernel.split("<")[1].split(",")[0])
    dom = {f: set(v) for f, v in ALL.items()}
    if hidden == 128:
        dom["weights"], dom["head"] = {"shared"}, {"random", "masked"}
    return dom


def _level_gaps(configs):
    got = collections.defaultdict(lambda: collections.defaultdict(set))
    count = collections.Counter(c.kernel for c in configs)
    for c in configs:
        for f, lv in c.levels().items():
            got[c.kernel][f].add(lv)
    gaps = [(kernel, "configurations", count[kernel]) for kernel in pc.KERNELS if count[kernel] < kc.MIN_PER_KERNEL]
    for kernel in pc.KERNELS:
        gaps += [(kernel, f, sorted(lv - got[kernel][f], key=str)) for f, lv in _expected_domain(kernel).items() if lv - got[kernel][f]]
    return gaps


def _pair_gaps(configs):
    need = {((f, a), (g, b)) for f, g in itertools.combinations(sorted(ALL), 2) for a in ALL[f] for b in ALL[g]} - IMPOSSIBLE
    have = set()
    for c in configs:
        have |= set(itertools.combinations(sorted(c.levels().items()), 2))
    return sorted(need - have, key=str)


def test_the_six_instantiations_and_their_domains():
    from test_policy_rollout_host import KERNELS as CENSUS

    assert [f"pz_rollout::{k}" for k in sorted(pc.KERNELS)] == CENSUS and len(pc.KERNELS) == 6 and set(DOMAINS) == set(pc.KERNELS)
    for kernel, dom in DOMAINS.items():
        assert {f: set(v) for f, v in dom.items()} == _expected_domain(kernel), kernel
    # the factors, the tables and the recipe are kernel_configs' own objects, not copies that could drift
    assert pc.FACTORS is kc.FACTORS and pc.SHAPING is kc.SHAPING and pc.SEED == kc.SEED and pc.plant_states is kc.plant_states
    assert pc.random_valid_states is kc.random_valid_states and pc.NORMAL_STATE_REWARD == kc.NORMAL_STATE_REWARD and pc.MIN_PER_KERNEL == 4
    for f in ("winning_score", "serve", "auto_reset", "simplify_action", "shaping", "normal_state_mode", "episode_stats", "stride", "ids"):
        assert pc.RUNTIME[f] is kc.FACTORS[f], f
    assert pc.required_pairs() == {((f, a), (g, b)) for f, g in itertools.combinations(sorted(ALL), 2) for a in ALL[f] for b in ALL[g]} - IMPOSSIBLE
    big = pc.IDS["large"]
    assert big == dict(env_id_base=(5 << 32) + 0xFFFFFFC0, first_game=2 ** 32 - 40, step=2 ** 32 - 2)


def test_every_instantiation_gets_every_level_of_every_factor():
    assert {c.kernel for c in CONFIGS} == set(pc.KERNELS)
    assert not _level_gaps(CONFIGS)
    seen = collections.defaultdict(set)
    for c in CONFIGS:
        for f, lv in c.levels().items():
            seen[f].add(lv)
    assert dict(seen) == ALL   # every level of the issue's table is in the generated set
    names = [c.name for c in CONFIGS]
    assert len(names) == len(set(names)) and 30 <= len(CONFIGS) <= 80, len(CONFIGS)


def test_every_compatible_pair_of_levels_occurs():
    assert not _pair_gaps(CONFIGS)


def test_every_configuration_is_one_the_launch_takes():
    for c in CONFIGS:
        assert pc.compatible(c.levels()) and c.kernel == pc.kernel_name(c.hidden, c.activation), c.name
        assert (c.n, c.k) in pc.SHAPES and c.stride_games in (c.n, c.n + 64) and c.pitch_games in (c.n, c.n + 4, c.n + 3)
        assert not (c.separate and c.hidden == 128) and (c.head != "bad" or c.separate)
        if (c.n, c.k) == (67, 5):      # the C ABI alone, the dword flush in the second workgroup
            assert c.pitch_games in (67, 70) and c.pitch_games % 4 != 0 and not c.binding
        sets = c.params()
        assert (sets[0] is sets[1]) == (not c.separate) and sets[0][4].shape == (c.n_actions + 1, c.hidden)
        b3 = [ps[5] for ps in sets]
        if c.head == "masked":
            assert all(int(np.isneginf(b).sum()) == 5 and np.isneginf(b[c.n_actions - 1]) and np.isfinite(b[c.n_actions]) for b in b3)
            assert int(c.masked().sum()) == 5
        elif c.head == "bad":
            assert np.isfinite(b3[0]).all() and int(np.isnan(b3[1]).sum()) == 1 and np.isnan(b3[1][:c.n_actions]).any()
        else:
            assert np.isfinite(b3[0]).all() and np.isfinite(b3[1]).all() and not c.masked().any()
    assert any(c.binding for c in CONFIGS if c.shaped and c.episode_stats == 1) and sum(c.binding for c in CONFIGS) >= 6
    for kernel in pc.KERNELS:   # every instantiation has a launch the binding can repeat
        assert any(c.binding for c in CONFIGS if c.kernel == kernel), kernel


def test_the_start_is_the_recipe_of_the_step_kernel_configurations():
    c = CONFIGS[0]
    planted, over = c.start_state()
    again, over2 = kc.plant_states(c, c.n)
    assert np.array_equal(planted, again) and np.array_equal(over, over2) and planted.shape == (44, c.n)
    assert np.array_equal(over, planted[42] != 0) and np.array_equal(over, np.maximum(planted[38], planted[39]) == c.winning_score)


def test_the_uniforms_are_the_judges():
    for seed, first, T in ((7, 0, 0), (0x9E3779B97F4A7C15, 2 ** 32 - 40, 2 ** 32 - 2), (3, (1 << 32) + 5, (1 << 33) + 1)):
        games = np.arange(132, dtype=np.uint64) + np.uint64(first)
        assert np.array_equal(pc.uniforms(seed, games, T), J.uniforms(seed, first, T, None, 132))


def test_every_configuration_bites_on_the_restatement_alone():
    pc.measure.cache_clear()  # measured here, not remembered from the generator
    for c in CONFIGS:
        f = pc.measure(c)
        print(f"{c.name} n = {c.n} k = {c.k}: {f.ended_early} games end before the last slab, {f.revived} are reset and move, "
              f"{f.frozen_unpaid} stay frozen unpaid, {f.over_at_entry} over at entry, {f.on_line} balls on a line, {f.cancelled} points "
              f"cancelled, {f.masked_hits} uniforms in a masked interval, {f.bad_rows} step-6 rows, {f.wrap_side} running games on a wrap's thinnest side; worst ambiguity {f.worst_ambiguity} "
              f"of a cap of {AJ.CAP(c.n)}")
        if c.k > 1:
            assert f.ended_early > 0, (c.name, "no game ends before the last slab")
        if c.auto_reset:
            assert f.revived > 0, (c.name, "no game is reset and moves afterwards")
        else:
            assert f.frozen_unpaid > 0, (c.name, "no game stays frozen with reward 0")
        assert f.over_at_entry > 0, c.name
        if c.shaped:
            assert f.on_line > 0, (c.name, "no post-step ball of a running game on x_line or y_line")
        if c.shaping == "cancel" and c.normal_state_mode == 2:
            assert f.cancelled > 0, (c.name, "no point cancelled by the table and replaced by RewardInNormalState")
        if c.ids == "large":
            assert c.n > 64 and c.env_id_base + 63 < 6 << 32 <= c.env_id_base + 64, c.name       # the low env-id word, at game 64
            assert c.n > 40 and c.first_game + 39 < 1 << 32 == c.first_game + 40, c.name          # first_game + g, at game 40
            assert c.k >= 4 and c.t0 + 1 < 1 << 32 == c.t0 + 2, c.name                            # T0 + t, at t = 2
            assert f.wrap_side > 0, (c.name, "a side of a wrap without a running game")
        if c.head == "masked":
            assert f.masked_hits > 0, c.name
        if c.head == "bad":
            assert f.bad_rows == c.n * c.k, c.name
        assert f.worst_ambiguity <= AJ.CAP(c.n), (c.name, "the restated trajectory leaves the judge's cap")
        assert pc.misses(c, f) == []
    # the sharp cases exist
    assert any(c.shaping == "cancel" and c.normal_state_mode == 2 and c.k == 8 for c in CONFIGS)
    assert any(c.episode_stats == "1-null" for c in CONFIGS)
    assert any(c.episode_stats == 1 and c.shaped for c in CONFIGS)
    assert any(c.serve == "random" and c.ids == "large" for c in CONFIGS)
    assert any(c.winning_score == 3 and not c.auto_reset for c in CONFIGS)
    assert any(c.stride == "n+64" and c.n == 132 for c in CONFIGS) and any(c.pitch != "n" and c.n == 132 for c in CONFIGS)


def test_the_conditions_bite():
    c = next(c for c in CONFIGS if c.shaped and c.auto_reset and c.k > 1)
    f = pc.measure(c)
    assert pc.misses(c, dataclasses.replace(f, revived=0)) == ["no game is reset and moves afterwards"]
    assert pc.misses(c, dataclasses.replace(f, on_line=0)) == ["no post-step ball of a running game on a shaping line"]
    assert pc.misses(c, dataclasses.replace(f, ended_early=0)) == ["no game ends before the last slab"]
    assert pc.misses(c, dataclasses.replace(f, worst_ambiguity=2)) == ["a slab with more ambiguous rows than the judge's cap"]
    assert "a wrap of the large ids without live games or steps on both sides" in pc.misses(dataclasses.replace(c, ids="large", shape=(36, 8)), f)
    c = next(c for c in CONFIGS if not c.auto_reset)
    assert pc.misses(c, dataclasses.replace(pc.measure(c), frozen_unpaid=0)) == ["no game stays frozen with reward 0"]
    c = next(c for c in CONFIGS if c.head == "masked")
    assert pc.misses(c, dataclasses.replace(pc.measure(c), masked_hits=0)) == ["no uniform falls into a masked action's interval"]


@pytest.mark.parametrize("what", ["level", "pair"])
def test_dropping_a_level_breaks_the_coverage(what):
    configs = list(CONFIGS)
    if what == "level":
        kernel = pc.kernel_name(64, "relu")
        configs = [dataclasses.replace(c, serve="alternate") if c.kernel == kernel and c.serve == "random" else c for c in configs]
        assert (kernel, "serve", ["random"]) in _level_gaps(configs)
    else:
        assert any(c.shaping == "cancel" and c.pitch == "n+3" for c in configs)
        configs = [dataclasses.replace(c, pitch="n") if c.shaping == "cancel" and c.pitch == "n+3" else c for c in configs]
        assert (("pitch", "n+3"), ("shaping", "cancel")) in _pair_gaps(configs)


def test_the_head_judge_takes_the_mask_and_nothing_else():
    """net_judge.worst_share: -inf on both sides (a masked logit) is no error; +inf, an infinity against a finite value and a
    NaN on one side stay infinite"""
    import net_judge as N

    inf = np.inf
    tol = np.array([[inf, 1e-6]])
    assert N.worst_share(np.array([[-inf, 1.0]]), np.array([[-inf, 1.0]]), tol)[0] == 0
    for have, ref in ((inf, inf), (-inf, 0.0), (0.0, -inf), (inf, -inf), (np.nan, -inf), (-inf, np.nan), (0.0, np.nan)):
        assert N.worst_share(np.array([[have, 1.0]]), np.array([[ref, 1.0]]), tol)[0] == inf, (have, ref)
    assert N.worst_share(np.array([[np.nan, 1.0]]), np.array([[np.nan, 1.0]]), tol)[0] == 0


def test_generation_is_deterministic():
    again, _ = pc.generated.__wrapped__(pc.SEED)
    assert again == CONFIGS


def test_the_comparison_passes_the_restatement_within_the_cap(oracle):
    """compare() on restate(): no failure, and in every slab of every configuration the ambiguous rows stay within
    act_judge.CAP(n) -- the cap is a condition on the cases, asserted here on the restatement's own trajectory"""
    for c in CONFIGS:
        got = pc.restate(c)
        fails, ambiguous = quiet(pc.compare, c, got)
        assert not fails, (c.name, fails[:3])
        assert len(ambiguous) == c.k and max(max(row) for row in ambiguous) <= AJ.CAP(c.n), (c.name, ambiguous)
        assert got["obs"][0].shape == (c.k + 1, c.n, 35) and got["values"][1].shape == (c.k + 1, c.n) and (got["entropy"] is None) == (not c.entropy)
        assert (got["returns"] is None) == (not c.stats_ptr)
    print(f"{len(CONFIGS)} configurations, {sum(c.binding for c in CONFIGS)} of them also through the binding")


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_the_comparison_rejects_the_mutant(mutant, oracle):
    """each mutant of the restatement is rejected on at least one generated configuration: a mutant no configuration rejects is
    a gap in the generator"""
    rejected = []
    for c in CONFIGS:
        fails, _ = quiet(pc.compare, c, pc.restate(c, mutant))
        if fails:
            rejected.append((c.name, fails[0]))
    print(f"{mutant}: rejected on {len(rejected)} of {len(CONFIGS)} configurations, first {rejected[:1]}")
    assert rejected, mutant
