"""The scenery kernels and the RGB renderer on the GPU, through the C ABI, against the judge of tests/scenery_judge.py:
``pz_scenery_init`` (scenery_init_kernel), ``pz_scenery_track`` (scenery_track_kernel) on its exhaustive table, ``pz_render``
(scenery_tick_kernel + render_kernel) on planted scenery and, without scenery, on the planted lanes of tests/pixel_judge.py;
a wide run of 200 games through the env; ``pz_probe_write``.  Every comparison is bit for bit; every buffer carries a sentinel
past its live part.  tests/test_scenery_host.py shows on the judge alone that these cases reach every branch and bite.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pixel_judge as pj
import scenery_judge as sj
from oracle import render_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, FRAME_SENT = -0x5A5A5A5B, 0xA5
FRAME_BYTES = ro.H * ro.W * 3
P2 = ro.P_WORDS


def cpu(t):
    return t.cpu().numpy()


def _lib():
    from pikazoo_amd import _native

    return _native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cfg(oracle, **kw):
    from pikazoo_amd import _native

    return _native.PzConfig.from_buffer_copy(oracle.make_config(**kw))


def _columns(host, words, pitch):
    """int32 [words, pitch] on the device: `host` in its first columns, the sentinel behind them."""
    t = torch.full((words, pitch), SENT, dtype=torch.int32, device=DEV)
    if host is not None and host.shape[1]:
        t[:, :host.shape[1]] = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    return t


def _first(got, want, what):
    w, l = np.argwhere(got != want)[0]
    return f"{what}: lane {l} word {w}: hip {got[w, l]} != judge {want[w, l]}"


@pytest.fixture(scope="module")
def sprites():
    return sj.sprite_set(DEV)


# ---- pz_scenery_init --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_scenery_init_vs_judge(n, oracle):
    pitch, seed, base = 256, sj.SEED, sj.ENV_ID_BASE
    start = oracle.OracleEnv(n, oracle.make_config(seed=seed, env_id_base=base)).state.copy()
    start[43] = 2 + 1000 * (np.arange(n) % 7) + 3 * np.arange(n)   # every lane continues from a counter of its own
    assert len(set(start[43])) == n
    want_state, want = start.copy(), np.zeros((sj.WORDS, n), np.int32)
    sj.init(want, want_state, seed, base)
    state, scenery = _columns(start, 44, pitch), _columns(None, sj.WORDS, pitch)
    cfg = _cfg(oracle, seed=seed, env_id_base=base)
    assert _lib().pz_scenery_init(scenery.data_ptr(), state.data_ptr(), n, pitch, C.byref(cfg), _stream()) == 0
    torch.cuda.synchronize()
    got, got_state = cpu(scenery), cpu(state)
    assert np.array_equal(got[:, :n], want), _first(got[:, :n], want, "scenery")
    assert np.array_equal(got_state[43, :n], start[43] + 40) and np.array_equal(got_state[43, :n], want_state[43])
    assert np.array_equal(got_state[:43, :n], start[:43])
    assert (got[:, n:] == SENT).all() and (got_state[:, n:] == SENT).all()


def test_scenery_init_of_no_game_writes_nothing(oracle):
    state, scenery = _columns(None, 44, 256), _columns(None, sj.WORDS, 256)
    cfg = _cfg(oracle, seed=sj.SEED, env_id_base=sj.ENV_ID_BASE)
    assert _lib().pz_scenery_init(scenery.data_ptr(), state.data_ptr(), 0, 256, C.byref(cfg), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((scenery == SENT).all()) and bool((state == SENT).all())


# ---- pz_scenery_track on its exhaustive table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset,resync", sj.TABLE_RUNS)
def test_scenery_track_vs_judge_on_the_whole_table(auto_reset, resync, oracle):
    sc, st = sj.track_table()
    n = sc.shape[1]
    pitch = n + 64
    want = sc.copy()
    sj.track(want, st, auto_reset, resync)
    state, scenery = _columns(st, 44, pitch), _columns(sc, sj.WORDS, pitch)
    cfg = _cfg(oracle, auto_reset=bool(auto_reset))
    assert _lib().pz_scenery_track(scenery.data_ptr(), state.data_ptr(), n, pitch, C.byref(cfg), resync, _stream()) == 0
    torch.cuda.synchronize()
    got, got_state = cpu(scenery), cpu(state)
    assert np.array_equal(got[69:, :n], want[69:]), _first(got[69:, :n], want[69:], f"words 69.. (auto_reset {auto_reset}, resync {resync})")
    assert np.array_equal(got[:69, :n], sc[:69])
    assert np.array_equal(got_state[:, :n], st)
    assert (got[:, n:] == SENT).all() and (got_state[:, n:] == SENT).all()


# ---- pz_render --------------------------------------------------------------------------------------------------------------
def _render(sprites, state, n, pitch, cfg, lanes, m, scenery, frames):
    lane_t = None if lanes is None else torch.tensor(lanes, dtype=torch.int32, device=DEV)
    err = _lib().pz_render(state.data_ptr(), n, pitch, None if cfg is None else C.byref(cfg),
                           None if lane_t is None else lane_t.data_ptr(), m, sprites.atlas.data_ptr(), sprites.table.data_ptr(),
                           sprites.background.data_ptr(), None if scenery is None else scenery.data_ptr(), frames.data_ptr(),
                           _stream())
    torch.cuda.synchronize()
    return err


def _planted_state(oracle, cfg, n, pitch):
    """An initialised state (pz_init at `pitch`, the sentinel behind lane n) with the planted words written into it."""
    state = _columns(None, 44, pitch)
    assert _lib().pz_init(state.data_ptr(), n, pitch, C.byref(cfg), _stream()) == 0
    torch.cuda.synchronize()
    host = sj.planted_state(cpu(state)[:, :n], n)
    state[:, :n] = torch.from_numpy(host).to(DEV)
    return state, host


def _frame_difference(got, want, lane):
    y, x, c = np.argwhere(got != want)[0]
    return f"lane {lane} pixel ({x},{y}) channel {c}: hip {got[y, x, c]} != judge {want[y, x, c]}"


def test_render_with_planted_scenery_vs_judge(sprites, oracle):
    """Three renders in a row of all 70 games, then a lane list: after each, all 75 scenery words and the state of every
    game against the judge's tick, and EVERY frame against ro.frame (2.8 ms each on the host: all 3 x 70 are compared)."""
    n, pitch = sj.N, 128
    cfg = _cfg(oracle, seed=sj.SEED, env_id_base=sj.ENV_ID_BASE)
    state, st = _planted_state(oracle, cfg, n, pitch)
    sc = sj.planted_scenery(n)
    scenery = _columns(sc, sj.WORDS, pitch)
    frames = torch.full((n + 1, ro.H, ro.W, 3), FRAME_SENT, dtype=torch.uint8, device=DEV)
    seen = {}
    for render in range(3):
        before_sc, before_st = cpu(scenery)[:, :n], cpu(state)[:, :n]
        sj.tick(sc, st, sj.SEED, sj.ENV_ID_BASE)
        assert _render(sprites, state, n, pitch, cfg, None, n, scenery, frames) == 0
        got_sc, got_st, got = cpu(scenery), cpu(state), cpu(frames)
        assert np.array_equal(got_sc[:, :n], sc), _first(got_sc[:, :n], sc, f"scenery after render {render}")
        assert np.array_equal(got_st[43, :n], st[43]) and np.array_equal(got_st[:43, :n], before_st[:43])
        assert (got_sc[:, n:] == SENT).all() and (got_st[:, n:] == SENT).all() and (got[n] == FRAME_SENT).all()
        for lane in range(n):
            want = ro.frame(st[:, lane], sprites.sprites_host, sprites.background_host, sc[:, lane])
            assert np.array_equal(got[lane], want), f"render {render}: " + _frame_difference(got[lane], want, lane)
        for name, count in sj.situations(before_sc, got_sc[:, :n], before_st, got_st[:, :n]).items():  # the words rendered
            seen[name] = seen.get(name, 0) + count
    assert len(seen) == 29 and all(v > 0 for v in seen.values()), seen

    # a lane list: out of order, across the wave boundary, with -1 and n (legal at the C ABI: their frames stay unwritten)
    lanes = [69, 3, -1, 64, 0, n, 63, 10, 65]
    frames.fill_(FRAME_SENT)
    before_sc, before_st = sc.copy(), st.copy()
    sj.tick(sc, st, sj.SEED, sj.ENV_ID_BASE, lanes=lanes)
    assert _render(sprites, state, n, pitch, cfg, lanes, len(lanes), scenery, frames) == 0
    got_sc, got_st, got = cpu(scenery), cpu(state), cpu(frames)
    assert np.array_equal(got_sc[:, :n], sc), _first(got_sc[:, :n], sc, "scenery after the lane list")
    assert np.array_equal(got_st[:, :n], st)
    others = [l for l in range(n) if l not in lanes]
    assert np.array_equal(got_sc[:, others], before_sc[:, others]) and np.array_equal(got_st[:, others], before_st[:, others])
    assert (sc[:, [l for l in lanes if 0 <= l < n]] != before_sc[:, [l for l in lanes if 0 <= l < n]]).any(axis=0).all()
    assert (got_sc[:, n:] == SENT).all() and (got_st[:, n:] == SENT).all()
    for j, lane in enumerate(lanes):
        if 0 <= lane < n:
            want = ro.frame(st[:, lane], sprites.sprites_host, sprites.background_host, sc[:, lane])
            assert np.array_equal(got[j], want), "lane list: " + _frame_difference(got[j], want, lane)
        else:
            assert (got[j] == FRAME_SENT).all(), f"the frame of lane {lane} was written"
    assert (got[len(lanes):] == FRAME_SENT).all()

    # m == 0: no launch
    assert _render(sprites, state, n, pitch, cfg, lanes, 0, scenery, frames) == 0
    assert np.array_equal(cpu(scenery), got_sc) and np.array_equal(cpu(state), got_st) and np.array_equal(cpu(frames), got)


def test_render_without_scenery_on_the_planted_lanes_vs_judge(sprites, oracle):
    """The planted lanes of the grey kernel (tests/pixel_judge.py) through render_kernel: 4 pixels per thread, 3-dword
    packing.  cfg is NULL and nothing is written to the state."""
    n, pitch = pj.N, 128
    state, st = _planted_state(oracle, _cfg(oracle, seed=4), n, pitch)
    start = cpu(state)
    frames = torch.full((n + 1, ro.H, ro.W, 3), FRAME_SENT, dtype=torch.uint8, device=DEV)
    assert _render(sprites, state, n, pitch, None, None, n, None, frames) == 0
    got = cpu(frames)
    for lane in range(n):
        want = ro.frame(st[:, lane], sprites.sprites_host, sprites.background_host)
        assert np.array_equal(got[lane], want), _frame_difference(got[lane], want, lane)
    assert (got[n] == FRAME_SENT).all() and np.array_equal(cpu(state), start)
    # out-of-range lanes without scenery: the draw's own guard
    lanes = [n, 5, -1, 66]
    frames.fill_(FRAME_SENT)
    assert _render(sprites, state, n, pitch, None, lanes, len(lanes), None, frames) == 0
    listed = cpu(frames)
    assert np.array_equal(listed[1], got[5]) and np.array_equal(listed[3], got[66])
    assert (listed[0] == FRAME_SENT).all() and (listed[2] == FRAME_SENT).all() and (listed[4:] == FRAME_SENT).all()
    assert np.array_equal(cpu(state), start)
    dive1 = np.isin(st[ro.P_STATE], (3, 4)) & (st[ro.P_DIVE] == -1)
    dive2 = np.isin(st[P2 + ro.P_STATE], (3, 4)) & (st[P2 + ro.P_DIVE] == 1)
    seen = {"power": (st[ro.B_POWER] != 0).sum(), "mirrored dive of player 1": dive1.sum(),
            "unmirrored dive of player 2": dive2.sum(), "scores >= 10": ((st[ro.E_S1] >= 10) & (st[ro.E_S2] >= 10)).sum(),
            "ball at the top": (st[ro.B_Y] < 20).sum(), "ball at the left": (st[ro.B_X] < 20).sum(),
            "ball at the right": (st[ro.B_X] > 412).sum(), "ball at the bottom": (st[ro.B_Y] > 284).sum(),
            "diver at the left wall": (np.isin(st[ro.P_STATE], (3, 4)) & (st[ro.P_X] < 32)).sum(),
            "diver at the right wall": (np.isin(st[P2 + ro.P_STATE], (3, 4)) & (st[P2 + ro.P_X] > 400)).sum()}
    assert all(v > 0 for v in seen.values()), seen


# ---- the wide run through the env -------------------------------------------------------------------------------------------
def _env(sprites, fmt, **kw):
    from pikazoo_amd import pikazoo_v0

    args = dict(num_envs=sj.WIDE_N, device=DEV, seed=sj.WIDE_SEED, env_id_base=sj.WIDE_BASE, render_mode="rgb_array",
                sprites=sprites, scenery=True, winning_score=sj.WIDE_WINNING_SCORE, validate_actions=False, state_format=fmt)
    args.update(kw)
    return pikazoo_v0.env(**args)


def _same(env, state, scenery, what):
    got_st, got_sc = cpu(env.read_state()), cpu(env._scenery[:, :env.num_envs])
    assert np.array_equal(got_st, state), _first(got_st, state, f"{what}: state")
    assert np.array_equal(got_sc, scenery), _first(got_sc, scenery, f"{what}: scenery")


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto-reset", "masked-reset"])
@pytest.mark.parametrize("fmt", ["int32", "packed"])
def test_wide_run_through_the_env_vs_judge(fmt, auto_reset, sprites):
    """200 games, winning_score 2, random actions, a rotating subset rendered behind every frame: state and all 75 scenery
    words after every step and every render against the CPU oracle + the judge (its reset-first definition of the auto-reset
    case); every 16th rendered frame against ro.frame.  sj.WIDE_FRAMES frames: pinned by tests/test_scenery_host.py."""
    records = sj.wide_record(int(auto_reset))
    env = _env(sprites, fmt, auto_reset=auto_reset)
    env.reset()
    k = compared = 0
    for t, rec in enumerate(records):
        env.step(env.random_actions(sj.WIDE_ACTION_SEED, t))
        _same(env, rec["stepped"], rec["tracked"], f"frame {t} stepped")
        due = rec["due"]
        picked = [j for j in range(len(due)) if (k + j) % 16 == 0]
        frames = env.render(lanes=due)[picked].cpu().numpy()
        k += len(due)
        _same(env, rec["state"], rec["scenery"], f"frame {t} rendered")
        for got, j in zip(frames, picked):
            want = ro.frame(rec["state"][:, due[j]], sprites.sprites_host, sprites.background_host, rec["scenery"][:, due[j]])
            assert np.array_equal(got, want), f"frame {t}: " + _frame_difference(got, want, due[j])
            compared += 1
        if rec["mask"] is not None:
            env.reset(mask=torch.from_numpy(rec["mask"]).to(DEV))
            _same(env, rec["state_reset"], rec["scenery_reset"], f"frame {t} reset")
    assert compared >= k // 16 and sj.wide_reached(sj.wide_events(records, int(auto_reset)))


@pytest.mark.parametrize("fmt", ["int32", "packed"])
def test_the_resync_callers_vs_the_judge(fmt, sprites, oracle):
    """A frame_skip=4 env for 30 policy steps and one step_many of 8 frames on a plain env: behind a k-frame launch the env
    resyncs -- radius cleared, the four flags re-read from the state the launch left, word 70 untouched."""
    from frame_skip_judge import HeldOracle

    n, seed, base = sj.WIDE_N, sj.WIDE_SEED, sj.WIDE_BASE
    cfg = oracle.make_config(winning_score=sj.WIDE_WINNING_SCORE, seed=seed, env_id_base=base, auto_reset=True)
    # frame skip: every step is a held launch
    env = _env(sprites, fmt, frame_skip=4)
    ref = HeldOracle(oracle, n, 4, cfg)
    sc = np.zeros((sj.WORDS, n), np.int32)
    sj.init(sc, ref.state, seed, base)
    env.reset(), ref.reset()
    for t in range(30):
        env.step(env.random_actions(sj.WIDE_ACTION_SEED, t))
        ref.step(*oracle.random_actions(n, base, sj.WIDE_ACTION_SEED, t, 18))
        sj.track_by_reset(sc, ref.state, 1, 1)
        _same(env, ref.state, sc, f"policy step {t}")
        due = sj.wide_due(t)
        env.render(lanes=due)
        sj.tick(sc, ref.state, seed, base, lanes=due)
        _same(env, ref.state, sc, f"policy step {t} rendered")
    assert (sc[69] == 0).all() and sc[71:75].any()
    # step_many on a plain env: single frames first, so that live punch effects are there to be cleared
    env = _env(sprites, fmt)
    ref = oracle.OracleEnv(n, cfg)
    sc = np.zeros((sj.WORDS, n), np.int32)
    sj.init(sc, ref.state, seed, base)
    env.reset(), ref.reset()
    for t in range(60):
        env.step(env.random_actions(sj.WIDE_ACTION_SEED, t))
        ref.step(*oracle.random_actions(n, base, sj.WIDE_ACTION_SEED, t, 18))
        sj.track_by_reset(sc, ref.state, 1, 0)
    _same(env, ref.state, sc, "before step_many")
    assert (sc[69] > 0).any()
    tape = np.stack([np.stack(oracle.random_actions(n, base, sj.WIDE_ACTION_SEED, t, 18)) for t in range(60, 68)])
    env.step_many(torch.from_numpy(tape).to(DEV))
    for t in range(8):
        ref.step(tape[t, 0], tape[t, 1])
    word_70 = sc[70].copy()
    sj.track_by_reset(sc, ref.state, 1, 1)
    assert (sc[69] == 0).all() and np.array_equal(sc[70], word_70)
    _same(env, ref.state, sc, "after step_many")


# ---- pz_probe_write ---------------------------------------------------------------------------------------------------------
def _probe_pattern(frames, side):
    """The documented pattern of `frames` frames: per 16-byte slot {frame, slot index within the span, side, 0}, 560 slots
    per 8 960-byte span, 1024 spans per frame."""
    out = np.zeros((frames, 1024, 560, 4), np.uint32)
    out[..., 0] = np.arange(frames, dtype=np.uint32)[:, None, None]
    out[..., 1] = np.arange(560, dtype=np.uint32)[None, None, :]
    out[..., 2] = side
    return out.reshape(-1)


@pytest.mark.parametrize("short", [False, True], ids=["two-frames-and-a-tail", "one-byte-short-of-three-frames"])
def test_probe_write_writes_its_pattern_and_stops(short):
    lib = _lib()
    frame_bytes = int(lib.pz_probe_frame_bytes())
    assert frame_bytes == 1024 * 8960
    size = 3 * frame_bytes if short else 2 * frame_bytes + 4096
    said = size - 1 if short else size
    words = size // 4
    want = [_probe_pattern(2, side) for side in (0, 1)]
    for use in ((True, False), (False, True), (True, True)):
        bufs = [torch.full((words,), SENT, dtype=torch.int32, device=DEV) for _ in range(2)]
        err = lib.pz_probe_write(bufs[0].data_ptr() if use[0] else None, bufs[1].data_ptr() if use[1] else None, said, _stream())
        torch.cuda.synchronize()
        assert err == 0
        for side in (0, 1):
            got = cpu(bufs[side]).view(np.uint32)
            if use[side]:
                assert np.array_equal(got[:2 * frame_bytes // 4], want[side]), (use, side)
                assert (got[2 * frame_bytes // 4:].view(np.int32) == SENT).all(), (use, side, "written past two frames")
            else:
                assert (got.view(np.int32) == SENT).all(), (use, side, "the buffer that was not passed")
