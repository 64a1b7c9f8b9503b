"""Per-game computer players on the GPU: pz_step_mixed through the C ABI against the judge of tests/mixed_judge.py --
every state word and every output of every frame --, and the mixed env on top of it.

The batch (mixed_judge.role_codes): 200 games at a pitch of 256 -- wave 0 without a computer player, wave 1 computer vs
computer, wave 2 with the four role codes cycling by lane, a tail of 8 lanes with random codes.  winning_score 2 and
320 frames of random actions: games end and are reset in place inside every run.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mixed_judge as mj

pytestmark = pytest.mark.gpu

N, STRIDE, WORDS, OBS = mj.N, mj.STRIDE, 44, 35
ACT_DTYPES = {"i32": torch.int32, "i64": torch.int64, "u8": torch.uint8, "i16": torch.int16}
A1, A2 = "player_1", "player_2"
CASES = mj.cases()


def cpu(t):
    return t.cpu().numpy()


def _tables(dev, mode):
    from pikazoo_amd.env import flight_tables

    return {"both": lambda: flight_tables(dev)[0], "power_hit": lambda: flight_tables(dev, landing=False)[0],
            "none": lambda: None}[mode]()


def _expected(oracle, case, frames, switch=None, reset_every=None):
    """The judge's run, recorded: per frame the two tensors of rows, rewards and terminations; the masks of the resets
    between frames (auto_reset off); the final state and statistics.  switch: (frame, codes) of a role change."""
    judge = mj.judge_for(oracle, case)
    start = judge.state
    n_act = 13 if case.simplify_action else 18
    acts = np.stack([np.stack(mj.actions(oracle, t, n_act)) for t in range(frames)])
    rec = dict(start=start, acts=acts, obs=[[], []], rew=[[], []], term=[], resets={}, codes=judge.codes.copy())
    for t in range(frames):
        if switch is not None and t == switch[0]:
            judge.set_codes(switch[1])
        judge.step(acts[t, 0], acts[t, 1])
        for p in range(2):
            rec["obs"][p].append(mj.rows_as(judge.obs(p), case.obs_format))
            rec["rew"][p].append(judge.rew(p).view(np.int32))
        rec["term"].append(judge.term)
        if reset_every and t % reset_every == reset_every - 1:  # reset() of the games that are over, as a caller would
            mask = judge.term.astype(np.uint8)
            judge.reset(mask)
            rec["resets"][t] = mask
    rec["state"], rec["stats"] = judge.state, judge.stats
    return rec


def _launch(case, rec, frames, switch=None, faults=None):
    """The same run through pz_step_mixed, every frame's outputs into its own slot; returns what the device holds."""
    from pikazoo_amd import _native
    from oracle import pz_oracle

    lib = _native.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cfg = _native.PzConfig.from_buffer_copy(pz_oracle.make_config(**case.oracle_kwargs()))
    cfg.packed_state = int(case.packed)
    cfg.normalize_obs = case.obs_format
    cfg.action_format = mj_action_format(case)
    cfg.p1_computer = cfg.p2_computer = 1 if case.tables == "power_hit" else 0  # ignored: the role codes decide
    if faults is not None:
        cfg.action_faults = faults.data_ptr()
    tables = _tables(dev, case.tables)
    tb = None if tables is None else C.byref(tables)

    state = torch.full((WORDS, STRIDE), -99, dtype=torch.int32, device=dev)
    state[:, :N] = torch.from_numpy(rec["start"]).to(dev)
    packed = torch.full((36 * STRIDE,), 0xA5, dtype=torch.uint8, device=dev)
    if case.packed:
        misfits = torch.zeros(1, dtype=torch.int64, device=dev)
        assert lib.pz_pack_state(state.data_ptr(), N, STRIDE, packed.data_ptr(), STRIDE, misfits.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert int(misfits.item()) == 0
    state_ptr = packed.data_ptr() if case.packed else state.data_ptr()
    stats = torch.zeros(20 * STRIDE, dtype=torch.uint8, device=dev)
    sp = stats.data_ptr() if case.shaped else None
    odt = torch.int16 if case.obs_format >= 2 else torch.int32
    obs = [torch.full((frames + 1, N, OBS), -7, dtype=odt, device=dev) for _ in range(2)]
    rew = [torch.full((frames + 1, N), -7, dtype=torch.int32, device=dev) for _ in range(2)]
    term = torch.full((frames + 1, N), 9, dtype=torch.uint8, device=dev)
    acts = torch.from_numpy(rec["acts"]).to(dev).to(ACT_DTYPES[case.action_format])
    codes = torch.from_numpy(rec["codes"]).to(dev)
    masks = {t: torch.from_numpy(m).to(dev) for t, m in rec["resets"].items()}
    new_codes = None if switch is None else torch.from_numpy(np.asarray(switch[1], np.uint8)).to(dev)
    torch.cuda.synchronize()
    for t in range(frames):
        if switch is not None and t == switch[0]:
            codes.copy_(new_codes)  # between two launches, on their stream: no synchronisation
        err = lib.pz_step_mixed(state_ptr, N, STRIDE, C.byref(cfg), codes.data_ptr(), acts[t, 0].data_ptr(),
                                acts[t, 1].data_ptr(), obs[0][t].data_ptr(), obs[1][t].data_ptr(), rew[0][t].data_ptr(),
                                rew[1][t].data_ptr(), term[t].data_ptr(), sp, tb, stream)
        assert err == 0, (case.name, t, err)
        if t in masks:
            assert lib.pz_reset(state_ptr, N, STRIDE, C.byref(cfg), masks[t].data_ptr(), None, None, sp, stream) == 0
    torch.cuda.synchronize()

    # nothing past lane n of the state, past the last frame of an output
    if case.packed:
        assert all(bool((part == 0xA5).all()) for part in (packed[16 * N:16 * STRIDE], packed[16 * STRIDE + 16 * N:32 * STRIDE],
                                                         packed[32 * STRIDE + 4 * N:])), "packed state past lane n"
        flagged = torch.zeros(1, dtype=torch.int64, device=dev)
        assert lib.pz_unpack_state(packed.data_ptr(), N, STRIDE, state.data_ptr(), STRIDE, flagged.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert int(flagged.item()) == 0
    assert bool((state[:, N:] == -99).all()), "state past lane n"
    assert all(bool((o[frames] == -7).all()) for o in obs) and all(bool((r[frames] == -7).all()) for r in rew)
    assert bool((term[frames] == 9).all())
    ret = stats[:16 * STRIDE].view(torch.float64).view(2, STRIDE)
    lengths = stats[16 * STRIDE:].view(torch.int32)
    assert bool((ret[:, N:] == 0).all()) and bool((lengths[N:] == 0).all()), "statistics past lane n"
    if not case.shaped:
        assert bool((stats == 0).all()), "statistics written without a statistics pointer"
    return dict(state=cpu(state[:, :N]), obs=[cpu(o[:frames]).astype(np.int32) for o in obs],
                rew=[cpu(r[:frames]) for r in rew], term=cpu(term[:frames]), ret=cpu(ret[:, :N]), lengths=cpu(lengths[:N]))


def mj_action_format(case):
    return {"i32": 0, "i64": 1, "u8": 2, "i16": 3}[case.action_format]


def _compare(case, rec, got, frames, oracle):
    for t in range(frames):
        for p in range(2):
            assert np.array_equal(got["obs"][p][t], rec["obs"][p][t]), (case.name, t, f"observations of player {p + 1}",
                                                                       np.flatnonzero((got["obs"][p][t] != rec["obs"][p][t]).any(axis=1)))
            assert np.array_equal(got["rew"][p][t], rec["rew"][p][t]), (case.name, t, f"rewards of player {p + 1}")
        assert np.array_equal(got["term"][t], rec["term"][t]), (case.name, t, "terminations")
    if not np.array_equal(got["state"], rec["state"]):
        f, l = np.argwhere(got["state"] != rec["state"])[0]
        pytest.fail(f"{case.name}: lane {l} (role code {rec['codes'][l]}) word {oracle.FIELD_NAMES[f]}: hip "
                    f"{got['state'][f, l]} != judge {rec['state'][f, l]}")
    if case.shaped:
        assert np.array_equal(got["ret"], rec["stats"][0]), (case.name, "episode returns")
        assert np.array_equal(got["lengths"], rec["stats"][1]), (case.name, "episode lengths")
    assert np.stack(rec["term"]).any(), "no game ended inside the run"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_mixed_step_vs_judge(case, oracle):
    rec = _expected(oracle, case, mj.FRAMES, reset_every=None if case.auto_reset else 40)
    got = _launch(case, rec, mj.FRAMES)
    _compare(case, rec, got, mj.FRAMES, oracle)
    if not case.auto_reset:
        assert rec["resets"] and any(m.any() for m in rec["resets"].values()), "no masked reset of a finished game"


@pytest.mark.parametrize("packed", [False, True], ids=["int32", "packed"])
def test_a_role_change_in_the_middle_of_a_run(packed, oracle):
    """The mask is rewritten between two launches: every game continues from its state under its new roles."""
    case = mj.Case("role-change", packed=packed)
    rng = np.random.default_rng(5)
    new = mj.role_codes().copy()
    new[:64] = rng.integers(0, 4, 64)   # the human-vs-human wave gets computer players
    new[64:128] = 0                     # computer vs computer becomes self-play
    new[128:] = (new[128:] + 1 + rng.integers(0, 3, N - 128)) % 4   # every one of these changes
    switch = (150, new.astype(np.uint8))
    rec = _expected(oracle, case, mj.FRAMES, switch=switch)
    got = _launch(case, rec, mj.FRAMES, switch=switch)
    _compare(case, rec, got, mj.FRAMES, oracle)


def test_an_out_of_range_action_on_a_computer_lane_is_counted(oracle):
    case = mj.Case("faults")
    rec = _expected(oracle, case, 2)
    codes = rec["codes"]
    assert codes[70] == 3 and codes[130] == 2 and codes[5] == 0
    rec["acts"] = rec["acts"].copy()
    rec["acts"][1, 0, 70] = 18    # player 1 of a computer-vs-computer game
    rec["acts"][1, 1, 130] = -1   # the computer side of a game against the computer
    rec["acts"][1, 1, 5] = 18     # and a human's
    faults = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _launch(case, rec, 2, faults=faults)
    assert int(faults.item()) == 3


# ---- through the env ----------------------------------------------------------------------------------------------------
def _env(codes, **kw):
    from pikazoo_amd import pikazoo_v0

    kw = {"validate_actions": False, **kw}
    return pikazoo_v0.env(num_envs=N, device="cuda:0", seed=mj.SEED, env_id_base=mj.ENV_ID_BASE, winning_score=mj.WINNING_SCORE,
                          is_player1_computer=(codes & 1).astype(bool), is_player2_computer=list((codes & 2) != 0), **kw)


def _tape(oracle, frames):
    return torch.as_tensor(np.stack([np.stack(mj.actions(oracle, t, 18)) for t in range(frames)]), device="cuda:0")


@pytest.mark.parametrize("fmt", ["int32", "packed"])
def test_eager_env_steps_equal_the_judge(fmt, oracle):
    """env.step() on a mixed env is the C-ABI run of test_mixed_step_vs_judge: the same judge, from the constructor."""
    frames, codes = 200, mj.role_codes()
    env = _env(codes, state_format=fmt)
    assert env.computer_players.dtype == torch.uint8 and np.array_equal(cpu(env.computer_players), codes)
    assert env.flight_tables == "both"
    judge = mj.judge_for(oracle, mj.Case("env"))
    tape = _tape(oracle, frames)
    env.reset(), judge.reset()
    for t in range(frames):
        obs, rew, term, _, _ = env.step({A1: tape[t, 0], A2: tape[t, 1]})
        judge.step(*cpu(tape[t]))
        if t % 50 == 49:
            assert np.array_equal(cpu(obs[A1]), judge.obs(0)) and np.array_equal(cpu(obs[A2]), judge.obs(1)), t
            assert np.array_equal(cpu(rew[A1]), judge.rew(0)) and np.array_equal(cpu(term[A1]).astype(np.uint8), judge.term), t
    assert np.array_equal(cpu(env.read_state()), judge.state)
    # roles rewritten between steps: one side for every game, the other per game
    env.set_computer_players(player_1=False, player_2=torch.as_tensor((codes & 1) != 0))
    new = ((codes & 1) << 1).astype(np.uint8)
    assert np.array_equal(cpu(env.computer_players), new)
    judge.set_codes(new)
    for t in range(60):
        env.step({A1: tape[t, 0], A2: tape[t, 1]})
        judge.step(*cpu(tape[t]))
    assert np.array_equal(cpu(env.read_state()), judge.state)


def test_an_output_ring_keeps_the_last_steps_of_a_mixed_env(oracle):
    """output_ring=3: the tensors of three successive steps are three buffer sets, each still that frame's results
    after the later steps; the fourth step takes the first set again."""
    frames, codes = 7, mj.role_codes()
    env = _env(codes, output_ring=3)
    judge = mj.judge_for(oracle, mj.Case("env"))
    tape = _tape(oracle, frames)
    env.reset(), judge.reset()
    got, want = [], []
    for t in range(frames):
        got.append(env.step({A1: tape[t, 0], A2: tape[t, 1]}))
        judge.step(*cpu(tape[t]))
        want.append((judge.obs(0), judge.obs(1), judge.rew(0), judge.rew(1), judge.term))
    torch.cuda.synchronize()
    for t in range(frames - 3, frames):  # the last three steps' results, read after all of them ran
        obs, rew, term, _, _ = got[t]
        assert np.array_equal(cpu(obs[A1]), want[t][0]) and np.array_equal(cpu(obs[A2]), want[t][1]), t
        assert np.array_equal(cpu(rew[A1]), want[t][2]) and np.array_equal(cpu(rew[A2]), want[t][3]), t
        assert np.array_equal(cpu(term[A1]).astype(np.uint8), want[t][4]), t
    assert len({got[t][0][A1].data_ptr() for t in range(frames - 3, frames)}) == 3
    assert got[frames - 4][0][A1].data_ptr() == got[frames - 1][0][A1].data_ptr()
    assert np.array_equal(cpu(env.read_state()), judge.state)


def test_hipgraph_replay_equals_eager(oracle):
    frames, codes = 48, mj.role_codes()
    tape = _tape(oracle, frames)
    results = {}
    for mode in ("eager", "graph"):
        env = _env(codes)
        env.reset()
        env.step({A1: tape[0, 0], A2: tape[0, 1]})  # (allocates and binds; a capture records launches only)
        if mode == "graph":
            torch.cuda.synchronize()
            side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                    for t in range(1, frames):
                        obs, rew, term, _, _ = env.step({A1: tape[t, 0], A2: tape[t, 1]})
                graph.replay()
            side.synchronize()
        else:
            for t in range(1, frames):
                obs, rew, term, _, _ = env.step({A1: tape[t, 0], A2: tape[t, 1]})
        results[mode] = (env.read_state().clone(), obs[A1].clone(), obs[A2].clone(), rew[A1].clone(), term[A1].clone())
    for a, b in zip(results["eager"], results["graph"]):
        assert torch.equal(a, b)


def test_checkpoint_round_trip_carries_the_roles(oracle):
    codes = mj.role_codes()
    tape = _tape(oracle, 80)
    env = _env(codes)
    env.reset()
    for t in range(40):
        env.step({A1: tape[t, 0], A2: tape[t, 1]})
    sd = env.state_dict()
    assert np.array_equal(cpu(sd["computer_players"]), codes)
    for t in range(40, 80):
        env.step({A1: tape[t, 0], A2: tape[t, 1]})
    other = _env(np.zeros(N, np.uint8) + (np.arange(N) % 2 == 0).astype(np.uint8))  # other roles: the checkpoint's win
    other.load_state_dict(sd)
    assert np.array_equal(cpu(other.computer_players), codes)
    for t in range(40, 80):
        other.step({A1: tape[t, 0], A2: tape[t, 1]})
    assert torch.equal(other.read_state(), env.read_state())
    # a uniform env's checkpoint carries no roles and loads as before; the two kinds do not load into each other
    from pikazoo_amd import pikazoo_v0

    kw = dict(num_envs=N, device="cuda:0", seed=mj.SEED, env_id_base=mj.ENV_ID_BASE, winning_score=mj.WINNING_SCORE)
    uniform = pikazoo_v0.env(**kw)
    usd = uniform.state_dict()
    assert usd["computer_players"] is None
    pikazoo_v0.env(**kw).load_state_dict(usd)
    del usd["computer_players"]  # (a checkpoint from before mixed envs)
    pikazoo_v0.env(**kw).load_state_dict(usd)
    with pytest.raises(ValueError, match="per-game computer players"):
        env.load_state_dict(usd)


def test_what_a_mixed_env_refuses(oracle):
    codes = mj.role_codes()
    env = _env(codes)
    env.reset()
    tape = _tape(oracle, 4).to(torch.int32)
    for call in (lambda: env.step_random(1), lambda: env.rollout_random(1, 4), lambda: env.step_many(tape),
                 lambda: env.step_many_held(tape), lambda: env.rollout_random_held(1, 4)):
        with pytest.raises(ValueError, match="mixed env"):
            call()
    with pytest.raises(ValueError, match="mixed env"):
        _env(codes, frame_skip=2)
    from pikazoo_amd import pikazoo_v0

    with pytest.raises(ValueError, match="one value per game"):
        pikazoo_v0.env(num_envs=N, device="cuda:0", is_player2_computer=[True] * (N - 1))
    with pytest.raises(ValueError, match="mixed env"):
        pikazoo_v0.env(num_envs=N, device="cuda:0", is_player2_computer=True).set_computer_players(player_1=True)


def test_two_python_bools_never_reach_the_mixed_launch(oracle, monkeypatch):
    """With two plain bools the env takes exactly today's path: cfg's two flags, the bound pz_step."""
    from pikazoo_amd import pikazoo_v0

    env = pikazoo_v0.env(num_envs=N, device="cuda:0", seed=3, is_player1_computer=False, is_player2_computer=True,
                         validate_actions=False)
    assert env.computer_players is None and (env._cfg.p1_computer, env._cfg.p2_computer) == (0, 1)

    def refuse(*a, **k):
        raise AssertionError("pz_step_mixed called by a uniform env")

    monkeypatch.setattr(type(env), "_step_mixed", refuse)
    calls = []
    bound = env._step_bound
    env._step_bound = lambda *a: calls.append(1) or bound(*a)
    ref = oracle.OracleEnv(N, oracle.make_config(is_player2_computer=True, seed=3))
    env.reset(), ref.reset()
    for t in range(20):
        a1, a2 = oracle.random_actions(N, 0, 11, t, 18)
        env.step({A1: torch.as_tensor(a1, device="cuda:0"), A2: torch.as_tensor(a2, device="cuda:0")})
        ref.step(a1, a2)
    assert len(calls) == 20 and np.array_equal(cpu(env.read_state()), ref.state)
