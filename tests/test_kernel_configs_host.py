"""The coverage rules of tests/kernel_configs.py (CPU only): what tests/test_gpu_kernel_configs.py launches.

Every instantiation of the kernel matrix receives every level of every runtime factor that applies to it, in at least
MIN_PER_KERNEL configurations; on each side of the size switch every pair of levels of two factors occurs; and every
configuration dispatches the instantiation it is assigned to.  The levels a kind of kernel takes are written down here
by hand, apart from the domain search in kernel_configs, so that a generator that silently narrowed a domain fails.
"""
import collections
import dataclasses
import itertools

import pytest

import kernel_configs as kc
import kernel_matrix as km

CONFIGS, DOMAINS = kc.generated()


def _traj(row):
    return row.entry in ("pz_rollout_random", "pz_step_many")


def _forms(row):
    """(PLAIN instantiation, fused instantiation) of the row's structure and row width"""
    fmt = kc.OBS_I16 if row.obs16 else kc.OBS_I32
    plain = kc.config_fields(p1_computer=row.p1, p2_computer=row.p2, packed_state=row.packed, normalize_obs=fmt)
    fused = dict(plain, simplify_action=1)
    return (km.dispatch(row.entry, row.k, row.n, plain, False, row.tables),
            km.dispatch(row.entry, row.k, row.n, fused, False, row.tables))


def _expected_domain(row):
    """The levels by hand: the single-frame kernels take every row format; a k-frame kernel's row width is a template
    argument (formats 0 - 1 on int32 rows, 2 - 6 on 2-byte rows), and its PLAIN form takes only configurations without
    a fused wrapper or statistics (a statistics mode without a pointer included).  action_format: pz_step alone."""
    dom = dict(kc.FACTORS)
    if row.entry != "pz_step":
        del dom["action_format"]
    plain_kernel, fused_kernel = _forms(row)
    if _traj(row):
        dom["obs_format"] = (2, 3, 4, 5, 6) if row.obs16 else (0, 1)
    if plain_kernel != fused_kernel and row.kernel == plain_kernel:
        dom.update(simplify_action=(0,), shaping=("off",), normal_state_mode=(0,), episode_stats=(0, "1-null"),
                   obs_format=(2,) if row.obs16 else (0,))
    return dom


def test_factors_hold_the_required_levels():
    want = {"winning_score": {1, 3, 15}, "serve": {"winner", "alternate", "random"}, "auto_reset": {0, 1},
            "simplify_action": {0, 1}, "shaping": {"off", "default", "shifted", "degenerate", "cancel"},
            "normal_state_mode": {0, 1, 2}, "obs_format": set(range(7)), "episode_stats": {0, 1, 2, "1-null"},
            "action_format": {"i32", "i64", "u8", "i16"}, "ids": {"small", "large"}, "stride": {"n", "n+64"}}
    assert {f: set(v) for f, v in kc.FACTORS.items()} == want
    big_id, big_t0 = kc.IDS["large"]
    assert big_id >= 1 << 32 and (big_id + km.N_BELOW - 1) >> 32 > big_id >> 32, "the low id word wraps in a launch"
    assert big_t0 < 1 << 32 < big_t0 + 5, "t0 crosses 2^32 inside every k-frame launch"
    assert kc.SHAPING["degenerate"][1:] == (0, 252)  # every ball in zone 2; y == 252 is a ground touch
    # the cancelling table: +-1 of a point plus the zone it was scored from is exactly 0 (zone 3: player 1's point)
    table = kc.SHAPING["cancel"][0]
    assert table[3] + 1 == 0 and table[7] - 1 == 0 and table[1] - 1 == 0 and table[5] + 1 == 0


def test_the_domains_are_the_kernels_own():
    rows = {r.kernel: r for r in reversed(km.ROWS)}
    assert set(DOMAINS) == km.KERNELS
    for kernel, dom in DOMAINS.items():
        want = _expected_domain(rows[kernel])
        assert {f: set(v) for f, v in dom.items()} == {f: set(v) for f, v in want.items()}, kernel


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
    for above in (False, True):
        side = [c for c in configs if c.above == above]
        need = kc.required_pairs([domains[k] for k in {c.kernel for c in side}])
        have = set()
        for c in side:
            lv = sorted(c.levels().items())
            have |= set(itertools.combinations(lv, 2))
        gaps[above] = sorted(need - have, key=str)
    return gaps


def test_every_instantiation_gets_every_level_of_every_factor():
    assert {c.kernel for c in CONFIGS} == km.KERNELS
    assert not _level_gaps(CONFIGS, DOMAINS)


def test_every_pair_of_levels_occurs_on_each_side_of_the_switch():
    gaps = _pair_gaps(CONFIGS, DOMAINS)
    assert not gaps[False] and not gaps[True], gaps
    # both sides hold configurations of every factor's every level
    for above in (False, True):
        seen = collections.defaultdict(set)
        for c in CONFIGS:
            if c.above == above:
                for f, lv in c.levels().items():
                    seen[f].add(lv)
        assert {f: set(v) for f, v in seen.items()} == {f: set(v) for f, v in kc.FACTORS.items()}, above


def test_every_configuration_dispatches_its_instantiation():
    names = [c.name for c in CONFIGS]
    assert len(names) == len(set(names))
    by_form = collections.defaultdict(set)
    for c in CONFIGS:
        assert km.dispatch(c.entry, c.k, c.n, c.fields(), c.stats_ptr, c.tables) == c.kernel, c.name
        assert (c.n >= km.SWITCH) == c.above and c.stride in (c.n, c.n + km.STRIDE_PAD)
        assert c.n % 8 == 0  # 2-byte rows of a k-frame launch
        if c.entry != "pz_step":
            assert c.action_format == "i32"  # pz_step_many returns PZ_E_CONFIG for the other element types
        by_form[c.kernel].add(c.plain_form)
    # both forms of every k-frame kernel that has a PLAIN form receive configurations, and the PLAIN ones include a
    # statistics mode without a pointer
    pairs = 0
    for r in km.ROWS:
        plain_kernel, fused_kernel = _forms(r)
        if plain_kernel != fused_kernel:
            pairs += 1
            assert by_form[plain_kernel] == {True} and False in by_form[fused_kernel], r.id
            assert any(c.kernel == plain_kernel and c.episode_stats == "1-null" for c in CONFIGS), plain_kernel
    assert pairs > 0


@pytest.mark.parametrize("what", ["level", "pair"])
def test_dropping_a_level_breaks_the_coverage(what):
    """The rules bite: replace one level of one instantiation's configurations by another valid level (the config
    still dispatches there) and the level rule -- or, for a pair, the pairwise rule -- fails."""
    configs = list(CONFIGS)
    kernel = next(c.kernel for c in configs if c.entry == "pz_step" and c.above)
    if what == "level":
        victims = [i for i, c in enumerate(configs) if c.kernel == kernel and c.action_format == "u8"]
        for i in victims:
            configs[i] = dataclasses.replace(configs[i], action_format="i16")
        assert (kernel, "action_format", ["u8"]) in _level_gaps(configs, DOMAINS)
    else:
        # every configuration above the switch with winning score 15 and the cancelling table: drop the score
        victims = [i for i, c in enumerate(configs) if c.above and c.winning_score == 15 and c.shaping == "cancel"]
        assert victims
        for i in victims:
            configs[i] = dataclasses.replace(configs[i], winning_score=3)
        assert (("shaping", "cancel"), ("winning_score", 15)) in _pair_gaps(configs, DOMAINS)[True]


def test_generation_is_deterministic_and_other_seeds_meet_the_rules():
    assert kc.configs() == kc.generated.__wrapped__(kc.SEED)[0]
    other, doms = kc.generated(kc.SEED + 1)
    assert other != CONFIGS
    assert not _level_gaps(other, doms)
    gaps = _pair_gaps(other, doms)
    assert not gaps[False] and not gaps[True]
