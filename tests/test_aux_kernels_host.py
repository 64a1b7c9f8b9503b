"""The cases of tests/aux_cases.py without a GPU: every axis value occurs in some case, and, on the oracle alone, the
cases bite -- a reset that ignored its mask, leaked into an unmasked game, dropped a carry-over word or cleared the
statistics of the wrong lane, and a policy stream that dropped the high word of an id or of the frame number, would
each leave something other than what the judge holds."""
import numpy as np
import pytest

import aux_cases as ac

RESET_CASES = ac.reset_cases()
WITH_MASK = [c for c in RESET_CASES if c.mask in ("ones", "lane", "random")]


# ---- every axis value occurs --------------------------------------------------------------------------------------------
def test_the_reset_cases_cover_every_axis():
    cases = RESET_CASES
    assert len({c.name for c in cases}) == len(cases) and 18 <= len(cases) <= 24
    assert {(c.n, c.stride) for c in cases} == set(ac.SIZES)
    assert {c.packed for c in cases} == {False, True}
    assert {c.obs_format for c in cases} == set(ac.FORMATS)
    for packed in (False, True):  # every row format in both state formats
        assert {c.obs_format for c in cases if c.packed == packed} == set(ac.FORMATS)
    assert {c.serve for c in cases} == set(ac.SERVES)
    assert {c.mask for c in cases} == set(ac.MASKS)
    assert {c.pointers for c in cases} == set(ac.POINTERS)
    assert {c.stats for c in cases} == {False, True}
    assert {c.start for c in cases} == set(ac.STARTS)
    # the named pairs
    assert any(c.packed and c.obs_format >= 2 and c.mask == "random" and c.stats for c in cases)
    assert any(not c.packed and c.obs_format == 1 and c.mask == "lane" for c in cases)
    # a mask together with a row format other than int32, in either state format; a statistics pointer with a mask; an
    # odd batch on 2-byte rows at its own pitch; ids beyond 2^32
    for packed in (False, True):
        assert any(c.packed == packed and c.obs_format != 0 and c.mask in ("lane", "random") for c in cases)
        assert any(c.packed == packed and c.stats and c.mask in ("lane", "random") for c in cases)
    assert any(c.n % 2 == 1 and c.n == c.stride and c.obs_format >= 2 for c in cases)
    assert any(c.env_id_base <= 2**32 <= c.env_id_base + c.n for c in cases) and any(c.env_id_base > 2**40 for c in cases)


def test_the_masks_are_what_their_names_say():
    for c in RESET_CASES:
        m = c.mask_array()
        if c.mask == "null":
            assert m is None and c.masked().all()
            continue
        assert m.dtype == np.uint8 and m.shape == (c.n,)
        if c.mask == "zeros":
            assert not m.any()
        elif c.mask == "ones":
            assert m.all()
        elif c.mask == "lane":
            (lane,) = np.flatnonzero(m)
            assert lane % ac.LANES == ac.LANES - 1
        elif c.n > 1:
            assert m.any() and not m.all()


def test_the_other_case_lists_cover_their_axes():
    obs = ac.observe_cases()
    assert {(c.packed, c.obs_format) for c in obs if c.pointers == "both"} == {(p, f) for p in (False, True) for f in ac.FORMATS}
    assert sorted(c.pointers for c in obs if c.pointers != "both") == ["p1", "p2"]
    init = ac.init_cases()
    assert {(c.packed, c.env_id_base, c.seed) for c in init} == {(p, b, s) for p in (False, True) for b in ac.ID_BASES
                                                                for s in ac.SEEDS}
    assert {(c.n, c.stride) for c in init} == set(ac.SIZES)
    assert ac.ID_BASES == (0, 2**32 - 3, 2**40 + 5)
    ra = ac.random_action_cases()
    assert len(set(ra)) == len(ra) == 4 * 2 * 3 * 3
    assert {c[0] for c in ra} == {1, 255, 256, 257} and {c[1] for c in ra} == {13, 18}
    assert {c[2] for c in ra} == {0, 2**32 - 1, 2**32 + 7} and {c[3] for c in ra} == set(ac.ID_BASES)
    states = ac.observe_states()
    assert states.shape[0] == ac.WORDS and states.shape[1] % 2 == 1 and states.shape[1] % ac.LANES != 0


# ---- the reset cases bite -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WITH_MASK, ids=[c.name for c in WITH_MASK])
def test_a_masked_reset_changes_its_games_and_no_other(case, oracle):
    j = ac.reset_judgement(oracle, case)
    changed = (j.state != j.start).any(axis=0)
    assert changed[j.masked].any(), "no masked game changes"
    assert not changed[~j.masked].any(), "the judge's reset leaks into an unmasked game"
    carry = list(ac.CARRY_OVER)
    assert np.array_equal(j.state[carry], j.start[carry]), "the judge's reset touches a carry-over word"
    if case.start != "constructed":
        # a carry-over word of a masked game is not what the constructor left, before and after: re-constructing the
        # game instead of resetting it would show
        differs = (j.start[carry] != j.constructor[carry]) & (j.state[carry] != j.constructor[carry])
        assert differs[:, j.masked].any(), "every masked game carries the constructor's values"
    if case.stats:
        assert (j.returns[:, j.masked] == 0).all() and (j.lengths[j.masked] == 0).all()
        assert np.array_equal(j.returns[:, ~j.masked], j.returns0[:, ~j.masked])
        assert np.array_equal(j.lengths[~j.masked], j.lengths0[~j.masked])


def test_over_the_reset_cases_an_unmasked_game_is_mid_game_or_over(oracle):
    mid = over = both_kinds_seeded = 0
    for case in RESET_CASES:
        if case.mask in ("null", "ones"):
            continue
        j = ac.reset_judgement(oracle, case)
        un = ~j.masked
        # mid-game: not the constructor's state and not a game that is over
        mid += int((un & (j.start[42] == 0) & (j.start != j.constructor).any(axis=0)).sum())
        over += int((un & (j.start[42] != 0)).sum())
        if case.stats and j.masked.any() and un.any():
            assert (j.returns0 != 0).all() and (j.lengths0 != 0).all()
            both_kinds_seeded += 1
    assert mid > 0 and over > 0, (mid, over)
    assert both_kinds_seeded > 0, "no case seeds a statistic on both a masked and an unmasked lane"


def test_the_played_start_holds_games_in_every_phase(oracle):
    st = ac.start_state(oracle, "played", 200, ac.SEEDS[0], 1 << 20)
    con = ac.constructed_state(oracle, 200, ac.SEEDS[0], 1 << 20)
    assert (st[42] != 0).any() and (st[42] == 0).any(), "the played start has no finished / no running game"
    assert (st[38:40] > 0).any() and (st[list(ac.CARRY_OVER)] != con[list(ac.CARRY_OVER)]).any()


def test_every_serve_mode_decides_some_reset(oracle):
    """The same start under the three serve modes: the ball's side after the reset is not the same in all of them."""
    case = next(c for c in RESET_CASES if c.start == "played" and c.mask == "null")
    sides = []
    for serve in ac.SERVES:
        c = ac.ResetCase(**{**case.__dict__, "serve": serve})
        sides.append(ac.reset_judgement(oracle, c).state[26])
    assert not np.array_equal(sides[0], sides[2]) or not np.array_equal(sides[0], sides[1])


# ---- the constructor and the policy stream depend on the whole id ------------------------------------------------------
def test_the_constructor_depends_on_both_id_words_and_the_seed(oracle):
    n = 200
    states = {(b, s): ac.constructed_state(oracle, n, s, b) for b in ac.ID_BASES for s in ac.SEEDS}
    for s in ac.SEEDS:
        crossing = states[(2**32 - 3, s)]
        assert np.array_equal(crossing[:, 3:], ac.constructed_state(oracle, n - 3, s, 2**32))  # ids, not lanes
        # the games past 2^32 are not the games 0, 1, ... of a kernel that dropped the high word
        assert not np.array_equal(crossing[:, 3:], states[(0, s)][:, :n - 3])
        assert not np.array_equal(states[(2**40 + 5, s)], ac.constructed_state(oracle, n, s, 5))
    for b in ac.ID_BASES:
        assert not np.array_equal(states[(b, ac.SEEDS[0])], states[(b, ac.SEEDS[1])])


def test_the_judge_takes_the_ids_and_frame_numbers_whole(oracle):
    """oracle.random_actions on the cases' ids and frames: in range, a function of the 64-bit id (not of the lane) and
    of the 64-bit frame number, and different from what either high word dropped would give."""
    for n, n_actions, t, base in ac.random_action_cases():
        a1, a2 = oracle.random_actions(n, base, ac.ACTION_SEED, t, n_actions)
        assert a1.dtype == np.int32 and a1.shape == (n,)
        assert 0 <= min(a1.min(), a2.min()) and max(a1.max(), a2.max()) < n_actions
        one = [oracle.random_actions(1, base + i, ac.ACTION_SEED, t, n_actions) for i in (0, n - 1)]
        assert (a1[0], a2[0]) == (one[0][0][0], one[0][1][0]) and (a1[-1], a2[-1]) == (one[1][0][0], one[1][1][0])
    for n_actions in ac.RA_ACTIONS:
        for t in ac.RA_FRAMES:
            crossing = np.stack(oracle.random_actions(257, 2**32 - 3, ac.ACTION_SEED, t, n_actions))
            at_zero = np.stack(oracle.random_actions(257, 0, ac.ACTION_SEED, t, n_actions))
            wrapped = np.stack(ac.low_word_ids_actions(oracle, 257, 2**32 - 3, t, n_actions))
            assert np.array_equal(wrapped[:, :3], crossing[:, :3]) and np.array_equal(wrapped[:, 3:], at_zero[:, :254])
            assert not np.array_equal(crossing, at_zero) and not np.array_equal(crossing, wrapped)
            assert (crossing[:, 3:] != wrapped[:, 3:]).mean() > 0.5
            large = np.stack(oracle.random_actions(257, 2**40 + 5, ac.ACTION_SEED, t, n_actions))
            assert not np.array_equal(large, np.stack(ac.low_word_ids_actions(oracle, 257, 2**40 + 5, t, n_actions)))
        for base in ac.ID_BASES:  # the frame number's high word
            high = np.stack(oracle.random_actions(257, base, ac.ACTION_SEED, 2**32 + 7, n_actions))
            assert not np.array_equal(high, np.stack(oracle.random_actions(257, base, ac.ACTION_SEED, 7, n_actions)))
            # and the stream is keyed: another seed, other actions
            assert not np.array_equal(high, np.stack(oracle.random_actions(257, base, ac.ACTION_SEED ^ (1 << 40), 2**32 + 7,
                                                                           n_actions)))


def test_the_chain_masks_finished_and_running_games(oracle):
    """The chain of test_gpu_aux_kernels on the judge alone: after its first 40 frames some games are over and some are
    not, and its masked reset takes both kinds."""
    n = ac.CHAIN_N
    env = oracle.OracleEnv(n, oracle.make_config(winning_score=1, seed=ac.SEEDS[0], env_id_base=ac.CHAIN_ID_BASE,
                                                 auto_reset=False, episode_stats=1))
    env.reset()
    for t in range(ac.CHAIN_FRAMES):
        env.step(*oracle.random_actions(n, ac.CHAIN_ID_BASE, ac.ACTION_SEED, t, 18))
    over = env.term != 0
    mask = ac.chain_mask(env.term).astype(bool)
    assert over.any() and not over.all()
    assert (mask & over).sum() == over.sum() and (mask & ~over).any() and (~mask).any()
    assert (env.episode_lengths[~mask] != 0).all()
