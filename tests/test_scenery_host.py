"""The scenery judge (tests/scenery_judge.py) without a GPU: its batch forms are the render oracle lane by lane, the
planted scenery and the exhaustive track table reach every branch the GPU cases of tests/test_gpu_scenery.py name, a
wrong kernel would show (one mutant of the judge per way of being wrong), and the wide run's recipe reaches its events at
the frame count the module pins."""
import numpy as np
import pytest

import scenery_judge as sj
from oracle import render_oracle as ro

P2 = ro.P_WORDS


@pytest.fixture(scope="module")
def sprite_set():
    return sj.sprite_set("cpu")


@pytest.fixture(scope="module")
def planted(oracle):
    """(state, scenery) as planted, and [(state, scenery)] after each of three ticks: computed once, never changed."""
    base = oracle.OracleEnv(sj.N, oracle.make_config(seed=sj.SEED, env_id_base=sj.ENV_ID_BASE)).state
    st, sc = sj.planted_state(base), sj.planted_scenery()
    ticks = []
    s, c = st.copy(), sc.copy()
    for _ in range(3):
        sj.tick(c, s)
        ticks.append((s.copy(), c.copy()))
    return (st, sc), ticks


# ---- the batch forms -----------------------------------------------------------------------------------------------------
def test_batch_forms_are_the_oracle_lane_by_lane(oracle):
    n = 5
    state = np.zeros((44, n), np.int32)
    state[43] = [2, 7, 1000, 2**31 - 20, -5]  # every lane continues from its own counter (one across the int32 wrap)
    start = state.copy()
    sc = np.full((sj.WORDS, n), -9, np.int32)
    sj.init(sc, state)
    for i in range(n):
        at = int(start[43, i]) & 0xFFFFFFFF
        want = [oracle.env_draw(sj.SEED, sj.ENV_ID_BASE + i, (at + k) & 0xFFFFFFFF, m)
                for k, m in enumerate([500, 152, 2, 11] * 10)]
        assert sc[0:40:4, i].tolist() == [-68 + v for v in want[0::4]] and sc[1:40:4, i].tolist() == want[1::4]
        assert sc[2:40:4, i].tolist() == [1 + v for v in want[2::4]] and sc[3:40:4, i].tolist() == want[3::4]
        assert sc[40:42, i].tolist() == [0, 2] and (sc[42:69, i] == 314).all() and (sc[69:, i] == 0).all()
        assert (int(state[43, i]) - int(start[43, i])) & 0xFFFFFFFF == 40
    # a lane list ticks those lanes only, leaves out what is outside 0..n-1, each from its own id
    before, st0 = sc.copy(), state.copy()
    sj.tick(sc, state, lanes=[3, -1, 0, n])
    assert np.array_equal(sc[:, [1, 2, 4]], before[:, [1, 2, 4]]) and np.array_equal(state[:, [1, 2, 4]], st0[:, [1, 2, 4]])
    for i in (0, 3):
        col, s1 = before[:, i].copy(), st0.copy()
        ro.scenery_tick(col, sj.stream(s1, i, sj.SEED, sj.ENV_ID_BASE))
        assert np.array_equal(sc[:, i], col) and state[43, i] == s1[43, i] != st0[43, i]


@pytest.mark.parametrize("auto_reset,resync", sj.TABLE_RUNS)
def test_the_restated_track_is_the_oracle_track_on_the_whole_table(auto_reset, resync):
    sc, st = sj.track_table()
    a, b = sc.copy(), sc.copy()
    sj.track(a, st, auto_reset, resync)
    sj.track_restated(b, st, auto_reset, resync)
    assert np.array_equal(a, b), np.flatnonzero((a != b).any(axis=0))[:8]
    assert np.array_equal(a[:69], sc[:69])
    if resync:  # as the header states it: radius cleared, the four flags re-read, word 70 untouched
        assert (a[69] == 0).all() and np.array_equal(a[70], sc[70])
        assert np.array_equal(a[71:75], st[[ro.P_COLL, P2 + ro.P_COLL, ro.E_GAME_ENDED, ro.E_ROUND_ENDED]])


def test_the_two_definitions_differ_only_where_the_wide_run_never_gets():
    """track and track_by_reset on the table: equal without auto-reset, under resync, and for every game that was not over;
    they differ only on rows with the previous frame's game_ended AND either a remembered collision flag or no remembered
    round_ended; the wide run, played with both definitions, never meets such a row."""
    sc, st = sj.track_table()
    for auto_reset, resync in sj.TABLE_RUNS:
        a, b = sc.copy(), sc.copy()
        sj.track(a, st, auto_reset, resync)
        sj.track_by_reset(b, st, auto_reset, resync)
        rows = np.flatnonzero((a != b).any(axis=0))
        if not (auto_reset and not resync):
            assert rows.size == 0
        else:
            assert rows.size and ((sc[73, rows] != 0) & ((sc[71, rows] != 0) | (sc[72, rows] != 0) | (sc[74, rows] == 0))).all()


# ---- the planted scenery reaches every situation --------------------------------------------------------------------------
def test_three_ticks_of_the_planted_scenery_reach_every_situation(planted):
    (st, sc), ticks = planted
    assert sc.shape == (sj.WORDS, sj.N) and sj.NAMED == 25
    seen, prev = {}, (st, sc)
    for s, c in ticks:
        for name, count in sj.situations(prev[1], c, prev[0], s).items():  # (asserts word 43: 27 + 2 respawns + re-draws)
            seen[name] = seen.get(name, 0) + count
        assert np.array_equal(s[:43], st[:43])
        prev = (s, c)
    assert len(seen) == 11 + 18 and all(v > 0 for v in seen.values()), seen
    # the named lanes hold what they are named for, on the first tick
    first = ticks[0][1]
    assert sc[0, sj.CLOUD_AT_432] == 431 and first[0, sj.CLOUD_AT_432] == 432 and first[3, sj.CLOUD_AT_432] == 5
    assert np.array_equal(first[1:3, sj.CLOUD_AT_432], sc[1:3, sj.CLOUD_AT_432])       # nothing re-drawn
    assert first[0, sj.CLOUD_RESPAWN] == -68 and first[4, sj.CLOUD_RESPAWN] == -68
    assert ticks[0][0][43, sj.CLOUD_RESPAWN] - st[43, sj.CLOUD_RESPAWN] == 27 + 4
    assert (sc[0:40:4, sj.CLOUD_LEFT_EDGE] == -68).all() and sc[3:40:4, sj.CLOUD_LEFT_EDGE].tolist() == list(range(10))
    assert sc[0, sj.TURN_WRAP] == -68 and (sc[3:40:4, sj.TURN_WRAP] == 10).all() and (first[3:40:4, sj.TURN_WRAP] == 0).all()
    top = first[:, sj.CLOUD_TOP]
    assert (top[1], top[3]) == (0, 5) and (top[5], top[7]) == (151, 5)                 # y = 0 and y = 151 at the largest size
    assert (sc[40, sj.WAVE_CLAMP], sc[41, sj.WAVE_CLAMP]) == (31, 2) and first[40:42, sj.WAVE_CLAMP].tolist() == [32, -1]
    assert first[40:42, sj.WAVE_TOP].tolist() == [31, -1]
    assert first[41, sj.WAVE_REDRAW] == 2 and -39 <= first[40, sj.WAVE_REDRAW] <= 0
    assert ticks[0][0][43, sj.WAVE_REDRAW] - st[43, sj.WAVE_REDRAW] == 28
    assert first[40:42, sj.WAVE_NEGATIVE].tolist() == [-3, 2] and ticks[0][0][43, sj.WAVE_NEGATIVE] - st[43, sj.WAVE_NEGATIVE] == 27
    assert sc[40, sj.WAVE_LOWEST] == -39 and first[40, sj.WAVE_LOWEST] == -37
    punch = slice(sj.PUNCH_FIRST, sj.NAMED)
    assert sc[69, punch].tolist() == list(range(20, -1, -2))
    assert first[69, punch].tolist() == list(range(18, -1, -2)) + [0] and np.array_equal(first[70], sc[70])
    assert set(st[ro.B_PUNCH_X, punch]) >= {20, 412} and {272, 0} <= set(sc[70, punch])
    # the seeded lanes behind stay inside what the constructor and the engine produce
    rest = sc[:, sj.NAMED:]
    assert rest[0:40:4].min() >= -68 and rest[0:40:4].max() <= 432 and rest[1:40:4].min() >= 0 and rest[1:40:4].max() <= 151
    assert set(np.unique(rest[2:40:4])) == {1, 2} and set(np.unique(rest[3:40:4])) <= set(range(11))
    assert rest[40].min() >= -39 and rest[40].max() <= 32 and set(np.unique(rest[41])) == {-1, 2}
    assert set(np.unique(rest[69])) <= set(range(0, 21, 2)) and rest[70].min() >= 0 and rest[70].max() <= 272


def test_the_judge_frame_is_the_oracle_frame(planted, sprite_set):
    s, c = planted[1][0]
    for lane in (sj.CLOUD_AT_432, sj.CLOUDS_OVERLAP, sj.WAVE_LOWEST, sj.PUNCH_FIRST, sj.NAMED - 1, 40, 69):
        want = ro.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane])
        assert np.array_equal(sj.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane]), want)
    # the scaled sprites: the oracle's walk of pygame.transform.scale is the header's floor(k * source / scaled) at every
    # size a cloud (48 x 24 grown by 0..10) and the punch effect (40 -> 2..40) take
    for src, sizes in ((48, range(48, 59, 2)), (24, range(24, 35, 2)), (40, range(2, 41, 2))):
        for dst in sizes:
            assert np.array_equal(ro.stretch_map(src, dst), np.arange(dst) * src // dst), (src, dst)


def test_the_synthetic_sprites_exercise_every_branch_of_the_blend(sprite_set):
    for sid in (ro.SPRITE_CLOUD, ro.SPRITE_WAVE, ro.SPRITE_PUNCH):
        alpha = sprite_set.sprites_host[sid][..., 3]
        assert (alpha == 0).any() and (alpha == 255).any() and ((alpha > 0) & (alpha < 255)).any(), sid


# ---- a wrong kernel would show -----------------------------------------------------------------------------------------------
def _frames_differ(sprite_set, state, a, b, lanes):
    return any(not np.array_equal(ro.frame(state[:, l], sprite_set.sprites_host, sprite_set.background_host, a[:, l]),
                                  ro.frame(state[:, l], sprite_set.sprites_host, sprite_set.background_host, b[:, l]))
               for l in lanes)


@pytest.mark.parametrize("mutant", sj.TICK_MUTANTS)
def test_a_wrong_engine_shows_on_a_planted_lane(planted, sprite_set, mutant):
    (st, sc), ticks = planted
    s, c = st.copy(), sc.copy()
    sj.tick(c, s, mutant=mutant)
    true_s, true_c = ticks[0]
    lanes = np.flatnonzero((c != true_c).any(axis=0))
    named = {"respawn at >= 432": sj.CLOUD_AT_432, "turn modulo 10": sj.TURN_WRAP, "clamp at 31": sj.WAVE_CLAMP,
             "re-draw without vel < 0": sj.WAVE_NEGATIVE, "punch counted down at radius 0": sj.NAMED - 1}[mutant]
    assert named in lanes, (mutant, lanes)
    if mutant in ("respawn at >= 432", "turn modulo 10", "clamp at 31"):  # (a wave with a negative coordinate lies below
        # the frame and a negative radius is not drawn: those two show in the words alone)
        assert _frames_differ(sprite_set, true_s, c, true_c, [named]), mutant
    if mutant in ("respawn at >= 432", "re-draw without vel < 0"):  # and the game's later draws move with it
        assert s[43, named] != true_s[43, named]


@pytest.mark.parametrize("mutant", sj.FRAME_MUTANTS)
def test_a_wrong_draw_shows_in_a_planted_frame(planted, sprite_set, mutant):
    s, c = planted[1][0]
    lanes = {"cloud scaled with the unscaled size": [sj.CLOUDS_OVERLAP, sj.CLOUD_TOP], "wave tile width 15": [sj.WAVE_TOP],
             "punch drawn before its decrement": [sj.PUNCH_FIRST, sj.NAMED - 3]}[mutant]  # the largest and the smallest drawn
    for lane in lanes:
        true = ro.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane])
        assert not np.array_equal(sj.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane], mutant), true), \
            (mutant, lane)


def test_the_punch_effect_at_its_largest_and_smallest_size_shows(planted, sprite_set):
    """Leaving the effect out changes the frame at radius 18 (the largest drawn) and at radius 2 (the smallest)."""
    s, c = planted[1][0]
    for lane, r in ((sj.PUNCH_FIRST, 18), (sj.NAMED - 3, 2)):
        assert c[69, lane] == r
        without = c[:, lane].copy()
        without[69] = 0
        assert _frames_differ(sprite_set, s, c, np.repeat(without[:, None], sj.N, axis=1), [lane]), r


@pytest.mark.parametrize("mutant", sj.TRACK_MUTANTS)
def test_a_wrong_track_shows_on_a_table_row(mutant):
    sc, st = sj.track_table()
    differing = 0
    for auto_reset, resync in sj.TABLE_RUNS:
        a, b = sc.copy(), sc.copy()
        sj.track(a, st, auto_reset, resync)
        sj.track_restated(b, st, auto_reset, resync, mutant=mutant)
        differing += int((a != b).any(axis=0).sum())
    assert differing > 0, mutant


def test_two_named_mutants_change_nothing_and_why(planted, sprite_set):
    """Two of the ways of being wrong have no effect, in the oracle and -- for the same reason -- in the kernel; pinned here
    so that nobody counts them as covered.  A punch effect drawn at radius 0 is a 0 x 0 blit (the draw list gets one more
    entry, no pixel can change; the kernel's `r >= 0` would test `dy < 0` unsigned).  Player 1's power hit overriding player
    2's sets the same radius and the same y: both read the ball's y of the state the frame left."""
    s, c = planted[1][0]
    lane = sj.NAMED - 2  # radius 2 before the tick, 0 after
    assert c[69, lane] == 0
    sizes = [(sp.shape[1], sp.shape[0]) for sp in sprite_set.sprites_host]
    drawn = ro.draw_list(s[:, lane], sizes, c[:, lane], True)
    extra = [b for b in drawn if b[0] == ro.SPRITE_PUNCH]
    assert len(drawn) == len(ro.draw_list(s[:, lane], sizes, c[:, lane])) + 1 and extra[0][4:] == (0, 0)
    assert np.array_equal(sj.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane], "punch drawn at radius 0"),
                          ro.frame(s[:, lane], sprite_set.sprites_host, sprite_set.background_host, c[:, lane]))
    sc, st = sj.track_table()
    for auto_reset, resync in sj.TABLE_RUNS:
        a, b = sc.copy(), sc.copy()
        sj.track(a, st, auto_reset, resync)
        sj.track_restated(b, st, auto_reset, resync, mutant="player 1 overrides")
        assert np.array_equal(a, b)
    assert set(sj.EQUIVALENT_MUTANTS) == {"punch drawn at radius 0", "player 1 overrides"}


# ---- the exhaustive table --------------------------------------------------------------------------------------------------
# bits of a table lane: 0..3 words 71..74, 4 / 5 the collision flags, 6 / 7 the players' states, 8 round_ended, 9 game_ended,
# 10 the radius before, 11 the remembered words as 1 or as another non-zero value.  What each outcome must NOT depend on:
IGNORED = {"resync": range(12), "frozen": (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11), "new-round clear": (9, 10, 11),
           "ground touch": (3, 9, 10, 11), "power hit by player 1 alone": (3, 8, 9, 10, 11),
           "power hit by player 2 alone": (3, 8, 9, 10, 11), "power hit by both": (3, 8, 9, 10, 11), "nothing happens": (9, 10, 11)}


def test_the_track_table_reaches_every_outcome_under_everything_it_ignores():
    sc, st = sj.track_table()
    n = 1 << sj.TABLE_BITS
    assert sc.shape == (sj.WORDS, n) and st.shape == (44, n)
    key = np.stack([sc[71] != 0, sc[72] != 0, sc[73] != 0, sc[74] != 0, st[ro.P_COLL], st[P2 + ro.P_COLL], st[ro.P_STATE] == 2,
                    st[P2 + ro.P_STATE] == 2, st[ro.E_ROUND_ENDED], st[ro.E_GAME_ENDED], sc[69] == 14]).astype(int)
    assert len({tuple(k) for k in key.T}) == 2048 and set(np.unique(sc[69])) == {0, 14}     # every combination, twice
    assert len(set(sc[70])) == n == len(set(st[ro.B_Y])) and not set(sc[70]) & set(st[ro.B_Y]) and 272 not in sc[70]
    lane = np.arange(n)
    occurred = set()
    for auto_reset, resync in sj.TABLE_RUNS:
        out = sc.copy()
        sj.track(out, st, auto_reset, resync)
        outcomes = sj.track_outcomes(sc, st, auto_reset, resync)
        assert np.array_equal(sum(m.astype(int) for m in outcomes.values()), np.ones(n, int))  # a partition of the rows
        for name, rows in outcomes.items():
            if not rows.any():
                continue
            occurred.add(name)
            for b in IGNORED[name]:
                assert {0, 1} == set((lane[rows] >> b) & 1), (name, b)
            # what the judge makes of the rows of this outcome
            want = {"resync": (0 * sc[69], sc[70]), "frozen": (sc[69], sc[70]), "new-round clear": (0 * sc[69], sc[70]),
                    "ground touch": (0 * sc[69] + 20, 0 * sc[70] + 272), "nothing happens": (sc[69], sc[70])}.get(
                        name, (0 * sc[69] + 20, st[ro.B_Y]))
            assert np.array_equal(out[69, rows], want[0][rows]) and np.array_equal(out[70, rows], want[1][rows]), name
        assert np.array_equal(out[71:75], st[[ro.P_COLL, P2 + ro.P_COLL, ro.E_GAME_ENDED, ro.E_ROUND_ENDED]])
        if not resync:  # frozen rows exist exactly without auto-reset; with it the same rows are tracked
            assert outcomes["frozen"].any() == (auto_reset == 0)
    assert occurred == set(IGNORED)


# ---- the wide run ----------------------------------------------------------------------------------------------------------
def test_the_wide_run_reaches_its_events_and_no_sooner():
    """sj.WIDE_FRAMES is the smallest frame count at which, with auto-reset on and off, games have ended and been reset and
    every wave of 64 lanes (and the tail of 8) has seen a ground-touch and a power-hit punch effect; the two definitions of
    the auto-reset case agree on every frame of it (wide_run asserts that, frame by frame, with both=True)."""
    assert sj.WIDE_N == 3 * 64 + 8 and set(sj.WIDE_PERIODS) == {1, 2, 3, 7}
    runs = {auto_reset: sj.wide_record(auto_reset, both=True) for auto_reset in (1, 0)}
    assert all(len(r) == sj.WIDE_FRAMES for r in runs.values())
    for auto_reset, records in runs.items():
        events = sj.wide_events(records, auto_reset)
        assert sj.wide_reached(events), (auto_reset, events)
    assert not all(sj.wide_reached(sj.wide_events(records[:-1], auto_reset)) for auto_reset, records in runs.items())
    # rendering is part of the run: every lane was drawn, and the draws moved the games' streams
    last = runs[1][-1]
    assert sorted({l for rec in runs[1] for l in rec["due"]}) == list(range(sj.WIDE_N))
    assert any((rec["state"][43] != rec["stepped"][43]).any() for rec in runs[1]) and last["scenery"].shape == (sj.WORDS, sj.WIDE_N)
