"""CPU tests of the wrapper-stack sweep (tests/wrapper_stacks.py): the judge of tests/test_gpu_wrapper_stacks.py --
``oracle.wrappers_oracle.WrappedOracle`` on every stack of depth one to four -- is tied to the unmodified reference
(tests/golden/stack_sweep_*.npz, recorded by ``oracle/ref_capture.capture_stack_sweep``), the cases are shown to bite on
the oracle alone, and the comparison rule is shown to tell a stack from its neighbours.
"""
import json

import numpy as np
import pytest

import wrapper_stacks as ws
from conftest import GOLDEN
from oracle import ref_capture

T = ws.RECIPE["T"]


@pytest.fixture(scope="module")
def sweep():
    """The recordings: {"shared": arrays, k: (rew [T, 2, L], term [T, L], ep_r [T, 2, L], ep_l [T, L])}."""
    out = {"shared": dict(np.load(GOLDEN / "stack_sweep_shared.npz"))}
    for depth in (1, 2, 3, 4):
        d = np.load(GOLDEN / f"stack_sweep_depth{depth}.npz")
        for j, k in enumerate(d["index"]):
            out[int(k)] = (d["rew"][j], d["term"][j], d["ep_r"][j], d["ep_l"][j])
    return out


def test_the_table_is_the_340_stacks_with_a_rotating_simplify_action():
    assert ws.n_stacks() == 4 + 16 + 64 + 256 == len({ws.all_names()[k] for k in range(ws.n_stacks())})
    places = set()
    for k in range(ws.n_stacks()):
        st = ws.stack(k)
        names = [n for n, _ in st]
        assert tuple(n for n in names if n != "SimplifyAction") == ws.all_names()[k]
        assert names.count("SimplifyAction") == (k % 4 != 0)
        if k % 4:
            at, depth = names.index("SimplifyAction"), len(names) - 1
            places.add("innermost" if at == 0 else "outermost" if at == depth else "middle")
            # (a stack of one wrapper has no middle: there it goes on top)
            assert at == {1: 0, 2: (depth + 1) // 2, 3: depth}[k % 4] and (not 0 < at < depth or k % 4 == 2)
        # instance i takes parameter set i; integer lines exactly below every NormalizeObservation
        balls = [(p, kw) for p, (n, kw) in enumerate(st) if n == "RewardByBallPosition"]
        for i, (p, kw) in enumerate(balls):
            assert tuple(kw["additional_reward"]) == tuple(ws.BALLPOS_SETS[i][0])
            above = "NormalizeObservation" in names[:p]
            assert (kw["x_line"], kw["y_line"]) == (ws.BALLPOS_SETS[i][3:5] if above else ws.BALLPOS_SETS[i][1:3])
            assert (0 < kw["x_line"] < 1 and 0 < kw["y_line"] < 1) == above
        assert [kw["reward"] for n, kw in st if n == "RewardInNormalState"] == \
            list(ws.NORMAL_REWARDS[:names.count("RewardInNormalState")])
    assert places == {"innermost", "middle", "outermost"}
    assert tuple(ws.BALLPOS_SETS[2][:3]) == (ref_capture.TEST_TABLE, 216, 176)
    assert tuple(ws.BALLPOS_SETS[3][:3]) == (ref_capture.INT_TABLE, 200, 150)
    for table, *_ in ws.BALLPOS_SETS[:2]:   # distinct dyadic values: exact in float32, a wrong zone / agent is another value
        assert len(set(table)) == 8 and all(float(v) * 8 == int(float(v) * 8) for v in table)
    assert len(set(ws.NORMAL_REWARDS)) == 4 and {1.0, -1.0} <= set(ws.ZERO_TABLE)
    g = ws.groups()
    assert len(g) == 17 and len(g["depth1"]) == 4 and all(len(v) == 21 for key, v in g.items() if key != "depth1")
    assert sorted(k for v in g.values() for k in v) == list(range(ws.n_stacks()))
    n = ws.NUM_ENVS
    assert n > 64 and n % 64 not in (0, 32) and ws.FIXTURE_LANES < n


def test_the_judge_equals_the_recorded_reference_on_every_stack(sweep):
    """``WrappedOracle`` on each of the 340 stacks against what the unmodified reference returned for it, float64 against
    float64: the rule of tests/test_oracle_golden.py (the last bit or two of a double)."""
    shared, L = sweep["shared"], ws.FIXTURE_LANES
    meta = json.loads(bytes(shared["meta"]).decode())
    assert meta["recipe"] == ws.RECIPE and meta["lanes"] == L and meta["stacks"] == ws.n_stacks()
    for simplify, a in ((False, "a18"), (True, "a13")):
        run, batch = ws.raw_run(L, simplify), ws.raw_run(ws.NUM_ENVS, simplify)
        assert np.array_equal(run["actions"], shared[f"actions_{a}"])
        assert np.array_equal(run["state_ctor"], shared[f"state_ctor_{a}"])
        assert np.array_equal(run["state0"], shared[f"state0_{a}"])
        assert np.array_equal(run["state"], shared[f"states_{a}"])
        for key in run:  # the batch's first games ARE the recorded ones
            assert np.array_equal(batch[key][..., :L, :] if key in ("obs0", "obs") else batch[key][..., :L], run[key]), key
    terminal = 0
    for k in range(ws.n_stacks()):
        st = ws.stack(k)
        a, count, what = ("a13" if ws.simplified(st) else "a18"), ws.n_normalize(st), f"stack {k} {ws.label(st)}"
        got = ws.judge_run(st, L)
        rew, term, ep_r, ep_l = sweep[k]
        np.testing.assert_allclose(got["obs0"], np.moveaxis(shared[f"obs0_{a}_{count}"], 1, 0), rtol=0, atol=1e-15, err_msg=what)
        np.testing.assert_allclose(got["obs"], shared[f"obs_{a}_{count}"], rtol=0, atol=1e-15, err_msg=what)
        np.testing.assert_allclose(got["rew"], rew, rtol=0, atol=1e-12, err_msg=what)
        assert np.array_equal(got["term"], term), what
        done = ep_l >= 0
        if ws.has_stats(st):
            assert np.array_equal(done, term.astype(bool)), what
            assert np.array_equal(got["ep_l"][done], ep_l[done]), what
            for i in range(2):
                np.testing.assert_allclose(got["ep_r"][:, i][done], ep_r[:, i][done], rtol=0, atol=1e-9, err_msg=what)
            terminal += int(done.sum())
        else:
            assert not done.any() and np.isnan(ep_r).all(), what
    assert terminal > 170 * 4  # (every stack with statistics reports several finished episodes)


def test_the_cases_bite_on_the_oracle_alone():
    """On the batch of the GPU sweep AND on the recorded games, for every stack: some game finishes two episodes (the
    sums are zeroed at least once); every RewardByBallPosition with integer lines pays all four zones, one above a
    normalisation at least two; every RewardInNormalState replaces a reward -- except the instances that cannot (another
    one below, no RewardByBallPosition between: they replace nothing) -- and somewhere one replaces a reward that was not
    0 before the wrapper below it (-1 + 1 of ZERO_TABLE on a lost point)."""
    for n in (ws.NUM_ENVS, ws.FIXTURE_LANES):
        revived = 0
        for k in range(ws.n_stacks()):
            st = ws.stack(k)
            what = f"stack {k} {ws.label(st)} on {n} games"
            assert (ws.raw_run(n, ws.simplified(st))["term"].sum(axis=0) >= 2).any(), what
            did, hidden, normalized = ws.trace(st, n), ws.shadowed(st), False
            for p, (name, kw) in enumerate(st):
                if name == "NormalizeObservation":
                    normalized = True
                elif name == "RewardByBallPosition":
                    assert len(did[p]["zones"]) >= (2 if normalized else 4), (what, p, did[p])
                elif name == "RewardInNormalState":
                    assert (did[p]["replaced"] == 0) == (p in hidden), (what, p, did[p])
                    revived += did[p]["replaced_nonzero"] > 0
        assert revived > 0
    # the shortest T (in tens) does it: ten frames less and a condition fails on the recorded games
    short = ws.raw_run(ws.FIXTURE_LANES, False, T - 10)
    zone = (short["obs"][:, 0, :, 27] > 120).astype(int) + 2 * (short["obs"][:, 0, :, 26] >= 232)
    assert len(np.unique(zone)) < 4 or not (short["term"].sum(axis=0) >= 2).any()


def _as_the_product_returns_it(st, run):
    """A judge's run in the product's number formats: float32 (or integer) observations and rewards."""
    normalized = ws.n_normalize(st) > 0
    wrapped = any(n in ws.REWARD_WRAPPERS for n, _ in st)
    out = dict(run, obs=run["obs"].astype(np.float32) if normalized else run["obs"].astype(np.int32),
               rew=run["rew"].astype(np.float32) if wrapped else run["rew"].astype(np.int32))
    return out


def _semantically_equal(a, b):
    return all(np.array_equal(a[key], b[key]) for key in a if key != "state") and a.keys() == b.keys()


def test_the_comparison_rule_tells_a_stack_from_its_transpositions(capsys):
    """What a wrongly placed fused wrapper looks like: two neighbours of the stack exchanged, every instance keeping its
    parameters.  Wherever the exchange changes what the judge computes at all, the GPU test's rule -- applied to the
    exchanged run in the product's number formats -- must reject it; and it must accept every stack's own run."""
    n = ws.NUM_ENVS
    different = same = 0
    for k in range(ws.n_stacks()):
        names = ws.all_names()[k]
        base = ws.with_parameters(names)
        st = ws.stack(k)
        want = ws.judge_run(st, n)
        assert ws.mismatches(st, _as_the_product_returns_it(st, want), want) == [], (k, ws.label(st))
        for i in range(len(names) - 1):
            if names[i] == names[i + 1]:
                continue
            swapped = base[:i] + [base[i + 1], base[i]] + base[i + 2:]
            mutant = ws.insert_simplify(swapped, k)
            run = ws.judge_run(mutant, n)
            found = ws.mismatches(st, _as_the_product_returns_it(mutant, run), want)
            if _semantically_equal(run, want):
                same += 1
                assert found == [], (k, ws.label(st), ws.label(mutant), found)
            else:
                different += 1
                assert found, f"stack {k} {ws.label(st)}: the rule cannot tell it from {ws.label(mutant)}"
    with capsys.disabled():
        print(f"\n[wrapper stacks] adjacent transpositions: {different} change the results and are rejected, "
              f"{same} change nothing")
    assert different > 300 and same > 100


@pytest.mark.parametrize("outer", ["RewardInNormalState", "RewardByBallPosition"])
def test_the_rule_rejects_a_reward_wrapper_moved_below_the_second_statistics(outer):
    """[Statistics, Statistics, reward wrapper]: fused into the kernel, the reward wrapper would sit BELOW the second
    (un-fused) statistics wrapper, whose sums would then hold the shaped returns."""
    kw = dict(reward=0.25) if outer == "RewardInNormalState" else \
        dict(additional_reward=list(ws.ZERO_TABLE), x_line=232, y_line=120)
    stats = ("RecordEpisodeStatistics", {})
    st, moved = [stats, stats, (outer, kw)], [stats, (outer, kw), stats]
    assert st == ws.with_parameters([n for n, _ in st])  # (stack 4 + 16 + 3*16 + 3*4 + {1, 0} of the table, its SimplifyAction aside)
    want, wrong = ws.judge_run(st, ws.NUM_ENVS), ws.judge_run(moved, ws.NUM_ENVS)
    assert np.array_equal(want["rew"], wrong["rew"])  # only the statistics tell
    found = ws.mismatches(st, _as_the_product_returns_it(moved, wrong), want)
    assert len(found) == 1 and found[0].startswith("episode returns differ"), found


def test_tolerances_come_from_the_number_formats():
    """The bound of wrapper_stacks.reward_error_bound on the table's extremes (derived, not measured): one table of
    dyadic values at magnitude 2 costs half an ulp there; the four tables together reach magnitude 12 and 1.7e-6, beyond
    the 1e-6 of the fixed rule -- and the float32 evaluation of every stack stays inside its bound."""
    b = "RewardByBallPosition"
    assert ws.reward_error_bound(ws.with_parameters(["RecordEpisodeStatistics", "NormalizeObservation"])) == 0.0
    assert ws.reward_error_bound(ws.with_parameters([b])) == 2.0 ** -24 + 2.0 ** -23
    four = ws.reward_error_bound(ws.with_parameters([b] * 4))
    assert 1e-6 < four < 1.8e-6 and ws.tolerances(ws.with_parameters([b] * 4))[0] == four
    assert ws.tolerances(ws.with_parameters([b, "RewardInNormalState"]))[0] == 1e-6
    assert ws.reward_error_bound(ws.with_parameters(["RewardInNormalState"])) == 0.25 * 2.0 ** -24
    run = ws.raw_run(ws.NUM_ENVS, False)
    for names in (n for n in ws.all_names() if len(n) == 4 and set(n) <= set(ws.REWARD_WRAPPERS)):
        st = ws.with_parameters(names)
        zones = run["obs"][:, 0].astype(np.float64)
        r32, r64 = run["rew"].astype(np.float32), run["rew"].astype(np.float64)
        for name, kw in st:
            if name == b:
                zone = (zones[..., 27] > kw["y_line"]).astype(int) + 2 * (zones[..., 26] >= kw["x_line"])
                t64 = np.asarray(kw["additional_reward"], np.float64)
                r64 = np.stack([r64[:, i] + t64[i * 4 + zone] for i in range(2)], axis=1)
                r32 = np.stack([r32[:, i] + t64.astype(np.float32)[i * 4 + zone] for i in range(2)], axis=1)
                assert r32.dtype == np.float32
            else:
                assert np.array_equal(r32 == 0, r64 == 0)  # both sides replace the same rewards
                r64 = np.where(r64 == 0, float(kw["reward"]), r64)
                r32 = np.where(r32 == 0, np.float32(kw["reward"]), r32)
        assert np.abs(r32.astype(np.float64) - r64).max() <= ws.reward_error_bound(st), names


def test_fusable_is_defined_on_every_stack_and_predicts_what_the_fused_oracle_can_express(oracle):
    """``ref_capture.fusable`` answers for all 340 stacks (a second RecordEpisodeStatistics is refused like every other
    second instance, it no longer overrides the first), and where it says yes the kernel's branches, as pz_oracle.c
    restates them under ``fused_options``, compute what the stack computes."""
    n, yes = ws.NUM_ENVS, 0
    for k in range(ws.n_stacks()):
        st = ws.stack(k)
        names = [name for name, _ in st]
        wr = dict(stack=[[name, kw] for name, kw in st])
        ok = ref_capture.fusable(wr)
        repeated = any(names.count(name) > 1 for name in ws.ALPHABET)
        assert not (ok and repeated), (k, ws.label(st))
        if not ok:
            with pytest.raises(AssertionError):
                ref_capture.fused_options(wr)
            continue
        yes += 1
        opt = ref_capture.fused_options(wr)
        env = oracle.OracleEnv(n, oracle.make_config(auto_reset=True, winning_score=ws.RECIPE["winning_score"],
                                                     seed=ws.RECIPE["seed"], env_id_base=ws.RECIPE["env_id_base"], **opt))
        env.reset()
        want, run = ws.judge_run(st, n), ws.raw_run(n, ws.simplified(st))
        for t in range(T):
            obs, rew, term = env.step(run["actions"][t, 0], run["actions"][t, 1])
            got = dict(state=env.state, term=term, obs=np.stack(obs), rew=np.stack(rew))
            if ws.has_stats(st):
                got.update(ep_l=env.episode_lengths, ep_r=env.episode_returns)
            found = ws.mismatches(st, got, {key: v[t] for key, v in want.items() if key != "obs0"})
            assert not found, (k, ws.label(st), t, found)
    # one of each at most, RewardByBallPosition below NormalizeObservation, no statistics between two reward wrappers
    assert yes == 39
    with pytest.raises(AssertionError, match="one RecordEpisodeStatistics"):
        ref_capture.fused_options(dict(stack=[["RecordEpisodeStatistics", {}], ["RecordEpisodeStatistics", {}]]))
