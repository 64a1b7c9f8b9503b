"""Judge of the scenery kernels and the RGB renderer (``pz_scenery_init``, ``pz_scenery_track``, ``pz_render``): batch
forms of the render oracle (oracle/render_oracle.py, whose ``scenery_init`` / ``scenery_tick`` / ``scenery_track`` /
``draw_list`` / ``frame`` tests/test_render_cpu.py pins to the reference's own ``render()``) over ``int32[75, n]`` scenery
and ``int32[44, n]`` state, the planted scenery and the exhaustive table of the GPU cases (tests/test_gpu_scenery.py),
the wide run's recipe, and the mutants with which tests/test_scenery_host.py shows that the cases bite.

Every lane draws from the env stream of its global id ``env_id_base + i`` and continues from its own word 43
(``oracle.pz_oracle.env_draw``, as ``replay_render_fixture`` of tests/test_render_cpu.py does for one lane).

Two definitions of what a frame does to the punch effect:

* ``track`` is ``ro.scenery_track`` lane by lane, extended with ``resync`` exactly as include/pikazoo_hip.h states it
  (radius cleared, the four remembered flags re-read, word 70 untouched).  It is the source-level definition: the
  exhaustive ``track_table`` is judged by it.
* ``track_by_reset`` states the auto-reset case a second, independent way: a game whose previous frame ended it is first
  reset the way ``raw_env.reset`` clears scenery (words 69, 71..74 to 0), then the frame is tracked as any other.  The two
  agree on every frame of the wide run (tests/test_scenery_host.py plays it with both); they differ on table rows that run
  never meets -- a finished game with a remembered collision flag, or without a remembered round_ended.  The wide run on
  the GPU is judged by this one.
"""
import functools

import numpy as np

import pixel_judge as pj
from oracle import render_oracle as ro

WORDS, STATE_WORDS = ro.SCENERY_WORDS, 44
N = pj.N                                  # the planted batch: one full wave of games and a tail of six
SEED, ENV_ID_BASE = 0x5CE9E12, (1 << 32) + 12345   # a non-default seed; ids whose high word is live
P2 = ro.P_WORDS
REMEMBERED = (71, 72, 73, 74)
RESET_CLEARS = (69, 71, 72, 73, 74)       # raw_env.reset of a game: no punch effect, nothing remembered


def _po():
    from oracle import pz_oracle as po

    po.build()
    return po


def stream(state, i, seed, env_id_base):
    """`draw(n)` = integers(0, n) of lane i's env stream, continuing from (and advancing) word 43 of `state`."""
    po = _po()

    def draw(n):
        v = po.env_draw(seed, env_id_base + i, int(state[43, i]) & 0xFFFFFFFF, n)
        state[43, i] = (int(state[43, i]) + 1 + (1 << 31)) % (1 << 32) - (1 << 31)  # (a uint32 counter kept in an int32 word)
        return v
    return draw


# ---- batch forms (in place) ---------------------------------------------------------------------------------------------
def init(scenery, state, seed=SEED, env_id_base=ENV_ID_BASE):
    """pz_scenery_init of every lane: all 75 words, 40 draws of each lane's stream."""
    for i in range(scenery.shape[1]):
        scenery[:, i] = ro.scenery_init(stream(state, i, seed, env_id_base))


def tick(scenery, state, seed=SEED, env_id_base=ENV_ID_BASE, lanes=None, mutant=None):
    """The engine of pz_render for the games `lanes` (None: all n); a lane outside 0..n-1 is left out."""
    n = scenery.shape[1]
    for i in (range(n) if lanes is None else lanes):
        if not 0 <= i < n:
            continue
        col = scenery[:, i].copy()
        if mutant is None:
            ro.scenery_tick(col, stream(state, i, seed, env_id_base))
        else:
            _tick_mutant(col, stream(state, i, seed, env_id_base), mutant)
        scenery[:, i] = col


def track(scenery, state, auto_reset, resync):
    """pz_scenery_track as the header states it: ro.scenery_track per lane; `resync` clears the radius and re-reads the
    four flags (word 70 stays)."""
    for i in range(scenery.shape[1]):
        col = scenery[:, i].copy()
        if resync:
            col[69] = 0
            col[71], col[72] = state[ro.P_COLL, i], state[P2 + ro.P_COLL, i]
            col[73], col[74] = state[ro.E_GAME_ENDED, i], state[ro.E_ROUND_ENDED, i]
        else:
            ro.scenery_track(col, state[:, i], auto_reset=bool(auto_reset))
        scenery[:, i] = col


def track_restated(scenery, state, auto_reset, resync, mutant=None, by_reset=False):
    """The same frame in numpy over all lanes (an own restatement: tests/test_scenery_host.py holds it to `track`), with the
    mutants of the track kernel, and -- `by_reset` -- the second definition of the auto-reset case (see the module text)."""
    sc = scenery
    coll = (state[ro.P_COLL] != 0, state[P2 + ro.P_COLL] != 0)
    in_2 = (state[ro.P_STATE] == 2, state[P2 + ro.P_STATE] == 2)
    round_ended, game_ended = state[ro.E_ROUND_ENDED] != 0, state[ro.E_GAME_ENDED] != 0
    if resync:
        sc[69] = 0
    else:
        over = sc[73] != 0
        if by_reset:
            was_reset = over & bool(auto_reset)
            sc[np.ix_(RESET_CLEARS, np.flatnonzero(was_reset))] = 0
            frozen = over & ~was_reset
        else:
            frozen = over if mutant == "frozen ignores auto_reset" else over & (not auto_reset)
        radius, y = sc[69].copy(), sc[70].copy()
        radius[sc[74] != 0] = 0
        radius[round_ended], y[round_ended] = 20, 252 + 20
        hits = [coll[p] & (sc[71 + p] == 0) & in_2[p] for p in (0, 1)]
        order = (1, 0) if mutant == "player 1 overrides" else (0, 1)
        for p in order:
            radius[hits[p]] = 20
            y[hits[p]] = sc[70][hits[p]] if mutant == "power hit keeps y" else state[ro.B_Y][hits[p]]
        sc[69] = np.where(frozen, sc[69], radius)
        sc[70] = np.where(frozen, sc[70], y)
    sc[71], sc[72], sc[73], sc[74] = coll[0], coll[1], game_ended, round_ended


def track_by_reset(scenery, state, auto_reset, resync):
    track_restated(scenery, state, auto_reset, resync, by_reset=True)


def clear_reset_games(scenery, mask):
    """What env.reset(mask) does to the scenery of the reset games."""
    scenery[np.ix_(RESET_CLEARS, np.flatnonzero(np.asarray(mask) != 0))] = 0


# ---- mutants of the engine and of the frame ---------------------------------------------------------------------------------
TICK_MUTANTS = ("respawn at >= 432", "turn modulo 10", "clamp at 31", "re-draw without vel < 0", "punch counted down at radius 0")
FRAME_MUTANTS = ("cloud scaled with the unscaled size", "wave tile width 15", "punch drawn before its decrement")
TRACK_MUTANTS = ("frozen ignores auto_reset", "power hit keeps y")
# restated for the record: both are no-ops in the oracle AND in the kernel (tests/test_scenery_host.py pins that) -- a
# punch effect of radius 0 is a 0 x 0 blit, and both players' power hits take y from the same state word
EQUIVALENT_MUTANTS = ("punch drawn at radius 0", "player 1 overrides")


def _tick_mutant(sc, draw, mutant):
    for i in range(10):
        sc[4 * i] += sc[4 * i + 2]
        if sc[4 * i] >= 432 if mutant == "respawn at >= 432" else sc[4 * i] > 432:
            sc[4 * i] = -68
            sc[4 * i + 1] = draw(152)
            sc[4 * i + 2] = 1 + draw(2)
        sc[4 * i + 3] = (sc[4 * i + 3] + 1) % (10 if mutant == "turn modulo 10" else 11)
    sc[40] += sc[41]
    top = 31 if mutant == "clamp at 31" else 32
    if sc[40] > top:
        sc[40], sc[41] = top, -1
    elif sc[40] < 0 and (sc[41] < 0 or mutant == "re-draw without vel < 0"):
        sc[41] = 2
        sc[40] = -draw(40)
    for i in range(27):
        sc[42 + i] = 314 - sc[40] + draw(3)
    if sc[69] > 0 or (mutant == "punch counted down at radius 0" and sc[69] == 0):
        sc[69] -= 2


def frame(col, sprites, background, scenery, mutant=None):
    """ro.frame with scenery (`scenery` = the game's words after its tick), blit by blit, so that a mutant can change one."""
    screen = background.copy()
    sizes = [(s.shape[1], s.shape[0]) for s in sprites]
    punch_drawn = True if mutant == "punch drawn at radius 0" and int(scenery[69]) == 0 else None
    if mutant == "punch drawn before its decrement" and int(scenery[69]) > 0:
        scenery = np.array(scenery)
        scenery[69] += 2  # (what a renderer that drew first and counted down afterwards would draw)
    blits = ro.draw_list(col, sizes, scenery, punch_drawn)
    wave = 0
    for sid, flip, x, y, w, h in blits:
        if sid == ro.SPRITE_CLOUD and mutant == "cloud scaled with the unscaled size":
            w, h = sizes[sid]
        if sid == ro.SPRITE_WAVE:
            if mutant == "wave tile width 15":
                x = 15 * wave
            wave += 1
        spr = ro.scaled(sprites[sid], w, h)
        ro._blit(screen, spr[:, ::-1] if flip else spr, x, y)
    return screen


# ---- the planted scenery ------------------------------------------------------------------------------------------------------
(CLOUD_AT_432, CLOUD_RESPAWN, CLOUD_LEFT_EDGE, TURN_WRAP, CLOUD_TOP, CLOUDS_OVERLAP, CLOUD_LEFT_CLIP, CLOUD_RIGHT_CLIP,
 CLOUD_ABOVE, WAVE_CLAMP, WAVE_TOP, WAVE_REDRAW, WAVE_NEGATIVE, WAVE_LOWEST) = range(14)
PUNCH_FIRST = 14                          # lanes 14..24: punch radius 20, 18, ..., 2, 0 before the tick
PUNCH_RADII = tuple(range(20, -1, -2))
NAMED = PUNCH_FIRST + len(PUNCH_RADII)    # 25 named lanes
# word 70 of the punch lanes: the ground touch's 272 and power-hit heights down to 0; word 37 (state): the reachable extremes
PUNCH_Y = (272, 0, 150, 272, 20, 1, 272, 96, 0, 272, 40)
PUNCH_X = (20, 412, 412, 20, 20, 412, 216, 412, 20, 412, 20)


def planted_scenery(n=N):
    """int32 [75, n]: the named lanes above, each there for one situation (tests assert it from the words themselves), seeded
    lanes behind them drawn from the ranges the reference's constructor and engine produce (x -68..432, y 0..151,
    x_vel 1..2, turn 0..10; vc -39..32 with vel 2 or -1; radius even 0..20, y 0..272)."""
    assert n >= NAMED
    rng = np.random.default_rng(75)
    sc = np.zeros((WORDS, n), np.int32)
    for c in range(10):
        sc[4 * c], sc[4 * c + 1] = rng.integers(-68, 433, n), rng.integers(0, 152, n)
        sc[4 * c + 2], sc[4 * c + 3] = rng.integers(1, 3, n), rng.integers(0, 11, n)
    sc[40] = rng.integers(-39, 33, n)
    sc[41] = np.where(rng.integers(0, 2, n) == 1, 2, -1)
    sc[42:69] = 314 - sc[40] + rng.integers(0, 3, (27, n))
    sc[69], sc[70] = 2 * rng.integers(0, 11, n), rng.integers(0, 273, n)
    sc[71:75] = rng.integers(0, 2, (4, n))
    # the named lanes: calm defaults (clouds in the middle of the sky, a resting wave, no punch effect), then the situation
    for lane in range(NAMED):
        for c in range(10):
            sc[4 * c:4 * c + 4, lane] = (40 + 30 * c, 20 + 10 * c, 1 + c % 2, c)
        sc[40, lane], sc[41, lane], sc[42:69, lane] = 10, 2, 304
        sc[69:75, lane] = 0

    def cloud(lane, c, x=None, y=None, x_vel=None, turn=None):
        for w, v in enumerate((x, y, x_vel, turn)):
            if v is not None:
                sc[4 * c + w, lane] = v

    cloud(CLOUD_AT_432, 0, x=431, x_vel=1, turn=4)      # becomes 432: no respawn, only its grown margin shows
    cloud(CLOUD_RESPAWN, 0, x=431, x_vel=2)             # 433: respawns to -68, two draws
    cloud(CLOUD_RESPAWN, 1, x=432, x_vel=1)             # 433 too
    for c in range(10):
        cloud(CLOUD_LEFT_EDGE, c, x=-68, turn=c)        # at the respawn position at every size (turn 10: TURN_WRAP)
        cloud(TURN_WRAP, c, turn=10)                    # wraps to 0
        cloud(CLOUD_TOP, c, y=0 if c % 2 == 0 else 151, turn=(4, 4, 0, 9, 2, 7, 3, 5, 1, 10)[c])  # turn 4 -> the largest size
        cloud(CLOUDS_OVERLAP, c, x=200 + 3 * c, y=60 + 2 * c, turn=c)
        cloud(CLOUD_LEFT_CLIP, c, x=-30 - c, x_vel=1, turn=c)
        cloud(CLOUD_RIGHT_CLIP, c, x=395 + 3 * c, x_vel=1, turn=c)
        cloud(CLOUD_ABOVE, c, y=-6, turn=c)             # (above what the constructor draws: size 0 at the top edge too)
    cloud(TURN_WRAP, 0, x=-68)
    for lane, vc, vel in ((WAVE_CLAMP, 31, 2), (WAVE_TOP, 32, -1), (WAVE_REDRAW, 0, -1), (WAVE_NEGATIVE, -5, 2),
                          (WAVE_LOWEST, -39, 2)):
        sc[40, lane], sc[41, lane] = vc, vel
    for k, r in enumerate(PUNCH_RADII):
        sc[69, PUNCH_FIRST + k], sc[70, PUNCH_FIRST + k] = r, PUNCH_Y[k]
    return sc


def planted_state(initialised, n=N):
    """`initialised` (int32 [44, n], an env's state) with the drawn words of pixel_judge.states() and the punch effect's x
    (word 37: the ball x of its event, 20..412) written into it."""
    st = pj.plant(initialised, pj.states(n))
    st[ro.B_PUNCH_X] = np.random.default_rng(37).integers(20, 413, n)
    st[ro.B_PUNCH_X, PUNCH_FIRST:NAMED] = PUNCH_X
    return st


def situations(before, after, state_before, state_after):
    """What one tick reached, counted from the judge's own words before and after it (int32 [75, m] / [44, m] of the ticked
    games): {name: number of clouds / lanes}."""
    x0, vel, turn0 = before[0:40:4].astype(np.int64), before[2:40:4], before[3:40:4]
    moved = x0 + vel
    x1, y1, turn1 = after[0:40:4], after[1:40:4], after[3:40:4]
    d = 5 - np.abs(turn1 - 5)
    left, top = x1 - d, y1 - d
    width, height = 48 + 2 * d, 24 + 2 * d
    vc = before[40] + before[41]
    respawns, redraws = (moved > 432).sum(axis=0), (vc < 0) & (before[41] < 0)
    out = {"cloud respawn": int((moved > 432).sum()), "no respawn at exactly 432": int(((moved == 432) & (x1 == 432)).sum()),
           "turn wrap": int(((turn0 == 10) & (turn1 == 0)).sum()), "wave clamp": int(((vc > 32) & (after[40] == 32)).sum()),
           "wave re-draw": int(redraws.sum()), "negative vc, positive vel: no re-draw": int(((vc < 0) & (before[41] > 0)).sum()),
           "lowest wave": int((before[40] == -39).sum()),
           "punch decrement to 0": int(((before[69] == 2) & (after[69] == 0)).sum()),
           "largest punch drawn": int((after[69] == 18).sum()), "smallest punch drawn": int((after[69] == 2).sum()),
           "ten clouds overlapping": int((((x1.max(axis=0) - x1.min(axis=0)) < 48) & ((y1.max(axis=0) - y1.min(axis=0)) < 24)).sum())}
    for size in range(6):
        at = d == size
        out[f"size {size} clipped at the left"] = int((at & (left < 0) & (left + width > 0)).sum())
        out[f"size {size} clipped at the top"] = int((at & (top < 0) & (top + height > 0) & (left + width > 0) & (left < ro.W)).sum())
        out[f"size {size} clipped at the right"] = int((at & (left < ro.W) & (left + width > ro.W)).sum())
    draws = (state_after[43].astype(np.int64) - state_before[43]).astype(np.int64)
    assert np.array_equal(draws, 27 + 2 * respawns + redraws), "word 43 must advance by 27 + 2 respawns + re-draws"
    return out


# ---- the exhaustive table of scenery_track_kernel ---------------------------------------------------------------------------------
TABLE_BITS = 12
OTHER_STATE = (0, 5)  # "one other value" than 2 per player


def track_table():
    """(scenery int32 [75, 4096], state int32 [44, 4096]): one lane per combination of the four remembered words, both
    collision flags, each player's state (2 / another), round_ended, game_ended and the radius before (0 / 14).  Ball y
    (1000 + lane) and word 70 (10000 + lane) are distinct per lane and from each other and the ground's 272, so a wrong
    source of y shows; words 0..68 carry a pattern the kernel must leave alone."""
    n = 1 << TABLE_BITS
    lane = np.arange(n)
    bit = lambda k: (lane >> k) & 1  # noqa: E731
    sc = (np.arange(WORDS)[:, None] * 7919 + lane[None, :] * 31 + 1).astype(np.int32)
    st = (np.arange(STATE_WORDS)[:, None] * 104729 + lane[None, :] * 17 + 3).astype(np.int32)
    for k, w in enumerate(REMEMBERED):
        sc[w] = bit(k)
    st[ro.P_COLL], st[P2 + ro.P_COLL] = bit(4), bit(5)
    st[ro.P_STATE] = np.where(bit(6) == 1, 2, OTHER_STATE[0])
    st[P2 + ro.P_STATE] = np.where(bit(7) == 1, 2, OTHER_STATE[1])
    st[ro.E_ROUND_ENDED], st[ro.E_GAME_ENDED] = bit(8), bit(9)
    sc[69] = 14 * bit(10)
    # bit 11 doubles the table with the flags as "any non-zero value" (the kernel tests != 0, the oracle truth)
    big = bit(11) == 1
    for w in REMEMBERED:
        sc[w] = np.where(big & (sc[w] != 0), 3 + lane % 5, sc[w])
    sc[70], st[ro.B_Y] = 10000 + lane, 1000 + lane
    return sc, st


TABLE_RUNS = [(auto_reset, resync) for auto_reset in (0, 1) for resync in (0, 1)]


def track_outcomes(sc, st, auto_reset, resync):
    """{outcome: bool [n]} of the kernel's source-level outcomes on the table's rows, from the inputs alone."""
    rise = [(st[p * P2 + ro.P_COLL] != 0) & (sc[71 + p] == 0) & (st[p * P2 + ro.P_STATE] == 2) for p in (0, 1)]
    rs = np.full(sc.shape[1], bool(resync))
    frozen = ~rs & (sc[73] != 0) & (not auto_reset)
    live = ~rs & ~frozen
    hit = rise[0] | rise[1]
    return {"resync": rs, "frozen": frozen, "new-round clear": live & (sc[74] != 0) & (st[ro.E_ROUND_ENDED] == 0) & ~hit,
            "ground touch": live & (st[ro.E_ROUND_ENDED] != 0) & ~hit, "power hit by player 1 alone": live & rise[0] & ~rise[1],
            "power hit by player 2 alone": live & rise[1] & ~rise[0], "power hit by both": live & rise[0] & rise[1],
            "nothing happens": live & (sc[74] == 0) & (st[ro.E_ROUND_ENDED] == 0) & ~hit}


# ---- the wide run ---------------------------------------------------------------------------------------------------------------
WIDE_N = 200                 # three waves and a tail of 8
WIDE_SEED, WIDE_BASE, WIDE_ACTION_SEED, WIDE_WINNING_SCORE = 31, (1 << 33) + 7, 5, 2
WIDE_PERIODS = tuple((1, 2, 3, 7)[i % 4] for i in range(WIDE_N))
WIDE_RESET_EVERY = 40        # auto_reset off: a masked reset of the finished games
# The smallest frame count at which, with either auto_reset, a game has ended and been reset and every wave of 64 lanes
# (and the tail) has seen a ground-touch and a power-hit punch effect: chosen on the CPU and pinned by
# tests/test_scenery_host.py::test_the_wide_run_reaches_its_events_and_no_sooner
WIDE_FRAMES = 80


def wide_due(t):
    return [i for i in range(WIDE_N) if (t + 1) % WIDE_PERIODS[i] == 0]


def wide_run(auto_reset, frames, both=False):
    """The wide run on the CPU oracle + this judge: yields per frame t a dict -- `stepped` / `tracked`: state after the step
    and scenery after its track; `due`: the lanes rendered; `state` / `scenery`: both after the render; `mask`: the masked
    reset behind the frame (auto_reset off, every 40 frames) or None, with `state_reset` / `scenery_reset` behind it.
    `both`: track with both definitions and assert that they agree."""
    po = _po()
    env = po.OracleEnv(WIDE_N, po.make_config(winning_score=WIDE_WINNING_SCORE, seed=WIDE_SEED, env_id_base=WIDE_BASE,
                                              auto_reset=bool(auto_reset)))
    sc = np.zeros((WORDS, WIDE_N), np.int32)
    init(sc, env.state, WIDE_SEED, WIDE_BASE)
    env.reset()
    clear_reset_games(sc, np.ones(WIDE_N))
    for t in range(frames):
        a1, a2 = po.random_actions(WIDE_N, WIDE_BASE, WIDE_ACTION_SEED, t, 18)
        env.step(a1, a2)
        other = sc.copy() if both else None
        track_by_reset(sc, env.state, auto_reset, 0)
        if both:
            track(other, env.state, auto_reset, 0)
            assert np.array_equal(sc, other), (t, np.flatnonzero((sc != other).any(axis=0)))
        rec = dict(stepped=env.state.copy(), tracked=sc.copy(), due=wide_due(t), mask=None)
        tick(sc, env.state, WIDE_SEED, WIDE_BASE, lanes=rec["due"])
        rec["state"], rec["scenery"] = env.state.copy(), sc.copy()
        if not auto_reset and t % WIDE_RESET_EVERY == WIDE_RESET_EVERY - 1:
            rec["mask"] = (env.state[ro.E_GAME_ENDED] != 0).astype(np.uint8)
            env.reset(rec["mask"])
            clear_reset_games(sc, rec["mask"])
            rec["state_reset"], rec["scenery_reset"] = env.state.copy(), sc.copy()
        yield rec


def wide_events(records, auto_reset):
    """What a recorded wide run reached: games reset inside it, and per group of lanes (the three waves, the tail) whether a
    ground-touch and a power-hit punch effect were set -- from the judge's words behind each frame's track."""
    groups = [slice(0, 64), slice(64, 128), slice(128, 192), slice(192, WIDE_N)]
    ground, power = np.zeros(WIDE_N, bool), np.zeros(WIDE_N, bool)
    over, resets = np.zeros(WIDE_N, bool), 0
    for rec in records:
        st, sc = rec["stepped"], rec["tracked"]
        now_over = st[ro.E_GAME_ENDED] != 0
        if auto_reset:
            resets += int((over & ~now_over).sum())  # the step behind a game's last frame reset it in place
        elif rec["mask"] is not None:
            resets += int(rec["mask"].sum())
        over = now_over
        ground |= (sc[69] == 20) & (sc[70] == 272) & (st[ro.E_ROUND_ENDED] != 0)
        power |= (sc[69] == 20) & (sc[70] == st[ro.B_Y]) & (st[ro.E_ROUND_ENDED] == 0)
    return dict(resets=resets, ground=[bool(ground[g].any()) for g in groups], power=[bool(power[g].any()) for g in groups])


def wide_reached(events):
    return events["resets"] > 0 and all(events["ground"]) and all(events["power"])


@functools.lru_cache(maxsize=None)
def wide_record(auto_reset, both=False):
    """wide_run(auto_reset) over WIDE_FRAMES recorded once (the GPU cases of both state formats share it; nothing changes it)."""
    return tuple(wide_run(auto_reset, WIDE_FRAMES, both=both))


def sprite_set(device):
    """The synthetic sprites of the GPU cases (opaque cores, soft rims, transparent corners: test_scenery_host.py asserts
    that the cloud, the wave and the punch effect hold alpha 0, 255 and values between)."""
    from pikazoo_amd.render import synthetic_sprites

    return synthetic_sprites(13, device)
