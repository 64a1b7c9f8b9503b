"""float16 / bfloat16 observation rows (include/pikazoo_hip.h enum pz_obs_format 3 - 6) on the GPU.

Every 16-bit row is defined bit for bit against a format already pinned to the reference: formats 3 / 4 are the int32
rows (format 0) converted to float32 and rounded to nearest even to float16 / bfloat16, formats 5 / 6 the fused
NormalizeObservation's float32 rows (format 1) rounded the same way.  So every test runs the same games in the pinned
format and in a 16-bit one and compares the rows as int16 bit patterns after that conversion in torch; states,
rewards and terminations must be identical.
"""
import contextlib
import ctypes as C
import itertools
import zlib

import numpy as np
import pytest
import torch
from torch.profiler import ProfilerActivity, profile

import kernel_matrix as km
from kernel_configs import config_fields
from test_gpu_packed import _random_valid_states
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
FORMAT = {(torch.float16, False): 3, (torch.bfloat16, False): 4, (torch.float16, True): 5, (torch.bfloat16, True): 6}
OBS = 35


def as16(pinned, dt):
    """The contract: a pinned row (int32, or the fused float32 quotient) as the 16-bit type, its bit pattern"""
    return pinned.to(torch.float32).to(dt).view(torch.int16)


def assert_rows(pinned, rows16, dt, what=""):
    assert rows16.dtype == dt and rows16.shape == pinned.shape, (what, rows16.dtype, rows16.shape)
    got, want = rows16.view(torch.int16), as16(pinned, dt)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[0].tolist()
        pytest.fail(f"{what}: first mismatch at {bad}: {rows16[tuple(bad)].item()} vs pinned {pinned[tuple(bad)].item()}")


def _pair(dt, normalized, **kw):
    from pikazoo_amd.wrappers import NormalizeObservation

    a, b = make_env(**kw), make_env(observation_dtype=dt, **kw)
    if normalized:
        a, b = NormalizeObservation(a), NormalizeObservation(b)
        assert a.fused and b.fused
    return a, b


# ---- 1. the same run in the pinned format and in the 16-bit one ------------------------------------------------------
CASES = [(1, {}), (63, dict(is_player2_computer=True)),
         (4096 + 8, dict(is_player1_computer=True, is_player2_computer=True, flight_tables="power_hit")),
         (km.SWITCH + 8, dict(is_player2_computer=True, flight_tables="none")),
         (4096 + 8, dict(is_player1_computer=True, flight_tables="both")),
         (km.SWITCH + 8, {})]


@pytest.mark.parametrize("fmt", ["int32", "packed"])
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("n,kw", CASES, ids=[f"n{n}-{'-'.join(k for k in kw) or 'human'}" for n, kw in CASES])
def test_float16_rows_are_the_pinned_rows_converted(n, kw, dtname, normalized, fmt):
    dt = DTYPES[dtname]
    a, b = _pair(dt, normalized, num_envs=n, seed=6, env_id_base=11, state_format=fmt, winning_score=3, **kw)
    ra, rb = a.unwrapped, b.unwrapped
    assert rb.obs_dtype == dt and rb._cfg.normalize_obs == FORMAT[(dt, normalized)]
    oa, ob = a.reset()[0], b.reset()[0]
    for ag in ("player_1", "player_2"):
        assert_rows(oa[ag], ob[ag], dt, f"reset {ag}")
    for t in range(40):
        acts = ra.random_actions(5, t)
        xa, xb = (a.step(acts), b.step(acts)) if t % 3 else (a.step_random(5, t0=t), b.step_random(5, t0=t))
        if t % 7 == 0 or t == 39:
            for ag in ("player_1", "player_2"):
                assert_rows(xa[0][ag], xb[0][ag], dt, f"frame {t} {ag}")
                assert torch.equal(xa[1][ag], xb[1][ag])
            assert torch.equal(xa[2]["player_1"], xb[2]["player_1"]) and torch.equal(ra.state, rb.state), t
    fa, fb = ra.observe(), rb.observe()
    for ag in ("player_1", "player_2"):
        assert_rows(fa[ag], fb[ag], dt, f"observe() {ag}")
    k = 19 if n % 8 == 0 else 1
    ta, tb = a.rollout_random(4, k), b.rollout_random(4, k)
    assert tb["obs"]["player_1"].shape == (k, n, OBS)
    for ag in ("player_1", "player_2"):
        assert_rows(ta["obs"][ag], tb["obs"][ag], dt, f"rollout_random {ag}")
        assert torch.equal(ta["rewards"][ag], tb["rewards"][ag])
    assert torch.equal(ta["terminations"], tb["terminations"]) and torch.equal(ra.state, rb.state)
    tape = ta["actions"].clone()
    ta, tb = a.step_many(tape), b.step_many(tape)
    for ag in ("player_1", "player_2"):
        assert_rows(ta["obs"][ag], tb["obs"][ag], dt, f"step_many {ag}")
        assert torch.equal(ta["rewards"][ag], tb["rewards"][ag])
    assert torch.equal(ta["terminations"], tb["terminations"]) and torch.equal(ra.state, rb.state)
    # the single-frame views follow the last frame
    assert torch.equal(rb.observe()["player_1"].view(torch.int16), tb["obs"]["player_1"][-1].view(torch.int16))
    assert torch.equal(b.step(ra.random_actions(5, 99))[0]["player_2"].view(torch.int16),
                       as16(a.step(ra.random_actions(5, 99))[0]["player_2"], dt))


# ---- 2. every instantiation the 16-bit formats reach ----------------------------------------------------------------
def _float16_instantiations():
    """ENTRIES x {N_BELOW, N_ABOVE} x packed x MIXES x TABLE_MODES, dispatched on 2-byte rows that are never PLAIN: the
    first configuration of every instantiation reached"""
    seen = {}
    for above, (entry, k), packed, (ai1, ai2), tables in itertools.product(
            (False, True), km.ENTRIES, (False, True), km.MIXES, km.TABLE_MODES):
        if tables != "none" and not (ai1 or ai2):
            continue
        n = km.N_ABOVE if above else km.N_BELOW
        cfg = config_fields(p1_computer=ai1, p2_computer=ai2, packed_state=packed, normalize_obs=3)
        name = km.dispatch(entry, k, n, cfg, False, tables)
        seen.setdefault(name, (entry, k, n, packed, ai1, ai2, tables))
    return seen


INSTANTIATIONS = _float16_instantiations()


def test_the_float16_formats_reach_only_named_instantiations():
    assert len(INSTANTIATIONS) == 75
    assert set(INSTANTIATIONS) <= km.KERNELS


@pytest.fixture(scope="module")
def tables_of():
    from pikazoo_amd.env import flight_tables

    dev = torch.device("cuda:0")
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = {"both": lambda: flight_tables(dev)[0], "power_hit": lambda: flight_tables(dev, landing=False)[0],
                          "none": lambda: None}[mode]()
        return made[mode]

    return get


@pytest.mark.parametrize("kernel", sorted(INSTANTIATIONS))
def test_every_float16_instantiation_against_the_pinned_formats(kernel, tables_of):
    from pikazoo_amd import _native

    lib = _native.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    entry, k, n, packed, ai1, ai2, table_mode = INSTANTIATIONS[kernel]
    k = min(k, 20)  # (the instantiation depends on k > 1 only)
    stride = n + km.STRIDE_PAD
    frames = k if entry in ("pz_rollout_random", "pz_step_many") else 1
    seed = zlib.crc32(kernel.encode())
    rng = np.random.default_rng(seed)
    planted = _random_valid_states(n, rng)
    over = rng.random(n) < 0.125  # an eighth of the games over: reset in place before their first frame
    winner = np.where(rng.random(n) < 0.5, 38, 39)
    planted[winner[over], np.flatnonzero(over)] = 3
    planted[41][over] = planted[42][over] = 1
    planted = torch.from_numpy(planted).to(dev)
    tables = tables_of(table_mode)
    tb = None if tables is None else C.byref(tables)
    base, aseed, t0 = 1 << 20, seed ^ 0x5EED, 1000
    tape = torch.empty((k, 2, n), dtype=torch.int32, device=dev)
    for f in range(k):
        assert lib.pz_random_actions(tape[f, 0].data_ptr(), tape[f, 1].data_ptr(), n, base, aseed, t0 + f, 18,
                                     stream) == 0
    state = torch.empty((44, stride), dtype=torch.int32, device=dev)
    packed_buf = torch.empty(36 * stride, dtype=torch.uint8, device=dev)

    def run(fmt):
        cfg = _native.PzConfig()
        cfg.winning_score, cfg.serve_mode, cfg.p1_computer, cfg.p2_computer = 3, 2, int(ai1), int(ai2)
        cfg.auto_reset, cfg.seed, cfg.env_id_base, cfg.x_line, cfg.y_line = 1, seed, base, 216, 176
        cfg.normalize_obs, cfg.packed_state = fmt, int(packed)
        state.fill_(-99)
        state[:, :n] = planted
        ptr = state.data_ptr()
        if packed:
            misfits = torch.zeros(1, dtype=torch.int64, device=dev)
            assert lib.pz_pack_state(state.data_ptr(), n, stride, packed_buf.data_ptr(), stride, misfits.data_ptr(),
                                     stream) == 0
            ptr = packed_buf.data_ptr()
        odt = torch.int32 if fmt < 2 else torch.int16
        obs = [torch.full((frames, n, OBS), -7, dtype=odt, device=dev) for _ in range(2)]
        rew = [torch.zeros((frames, n), dtype=torch.int32, device=dev) for _ in range(2)]
        term = torch.zeros((frames, n), dtype=torch.uint8, device=dev)
        act = torch.zeros((k, 2, n), dtype=torch.int32, device=dev)
        o = (obs[0].data_ptr(), obs[1].data_ptr(), rew[0].data_ptr(), rew[1].data_ptr(), term.data_ptr())
        torch.cuda.synchronize()
        watch = fmt >= 3  # (the dispatched kernel is checked on the 16-bit runs)
        with (profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) if watch else contextlib.nullcontext()) as prof:
            if entry == "pz_step":
                err = lib.pz_step(ptr, n, stride, C.byref(cfg), tape[0, 0].data_ptr(), tape[0, 1].data_ptr(), *o, None,
                                  tb, stream)
            elif entry == "pz_step_random":
                err = lib.pz_step_random(ptr, n, stride, C.byref(cfg), aseed, t0, k, *o, None, None, tb, stream)
            elif entry == "pz_rollout_random":
                err = lib.pz_rollout_random(ptr, n, stride, C.byref(cfg), aseed, t0, k, act.data_ptr(), *o, None, None,
                                            tb, stream)
            else:
                err = lib.pz_step_many(ptr, n, stride, C.byref(cfg), tape.data_ptr(), k, *o, None, None, tb, stream)
            assert err == 0, (kernel, fmt, err)
            torch.cuda.synchronize()
        names = [e.name.replace("void ", "").split("(")[0].replace("pz::", "") for e in prof.events()
                 if e.device_type == torch.autograd.DeviceType.CUDA and "pz::" in e.name] if watch else []
        if packed:
            flagged = torch.zeros(1, dtype=torch.int64, device=dev)
            assert lib.pz_unpack_state(packed_buf.data_ptr(), n, stride, state.data_ptr(), stride, flagged.data_ptr(),
                                       stream) == 0
        torch.cuda.synchronize()
        return dict(obs=obs, rew=rew, term=term, act=act, state=state[:, :n].clone(), kernels=names)

    for normalized in (False, True):
        pinned = run(1 if normalized else 0)
        view = (lambda x: x.view(torch.float32)) if normalized else (lambda x: x)
        for dt in (torch.float16, torch.bfloat16):
            fmt = FORMAT[(dt, normalized)]
            got = run(fmt)
            assert got["kernels"] == [kernel], (fmt, got["kernels"])
            for i in range(2):
                assert_rows(view(pinned["obs"][i]), got["obs"][i].view(dt), dt, f"{kernel} format {fmt} agent {i}")
                assert torch.equal(pinned["rew"][i], got["rew"][i])
            assert torch.equal(pinned["term"], got["term"]) and torch.equal(pinned["act"], got["act"])
            assert torch.equal(pinned["state"], got["state"]), (kernel, fmt)


# ---- 3. against the reference's own trajectories --------------------------------------------------------------------
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("name", ["normalize_observation", "full_wrapper_stack"])
def test_reference_fixtures_in_float16(name, dtname):
    from conftest import load_golden

    dt = DTYPES[dtname]
    d = load_golden(name)
    meta = d["meta"]
    env = make_env(meta, observation_dtype=dt)
    raw = env.unwrapped
    assert raw._cfg.normalize_obs == FORMAT[(dt, True)] and not raw._unfused
    want = torch.from_numpy(d["obs"].astype(np.float32))  # [T, 2, L, 35]: the reference's quotient as float32
    obs, _ = env.reset()
    w0 = torch.from_numpy(d["obs_reset"].astype(np.float32))
    for i, ag in enumerate(raw.possible_agents):
        assert_rows(w0[:, i], obs[ag].cpu(), dt, f"{name} reset {ag}")
    acts = torch.as_tensor(d["actions"].astype(np.int32), device=raw.device)
    T = meta["steps"]
    got = torch.empty((T, 2, meta["lanes"], OBS), dtype=dt, device=raw.device)
    for t in range(T):
        obs = env.step({"player_1": acts[t, 0], "player_2": acts[t, 1]})[0]
        got[t, 0].copy_(obs["player_1"])
        got[t, 1].copy_(obs["player_2"])
    assert_rows(want, got.cpu(), dt, name)


# ---- 4. every column's whole value range, the out-of-domain states included ----------------------------------------
@pytest.mark.parametrize("name", ["planted_random_states_human", "planted_random_states_both_computer",
                                  "planted_random_states_p2_computer_random_serve", "planted_fast_balls_human",
                                  "planted_fast_balls_both_computer"])
def test_observe_over_the_planted_state_space(name):
    from conftest import load_golden
    from pikazoo_amd import _native

    lib = _native.load()
    d = load_golden(name)
    states = np.concatenate([d["planted"].astype(np.int32)] + [s.astype(np.int32) for s in d["states"]], axis=1)
    m = states.shape[1]
    dev = torch.device("cuda:0")
    st = torch.from_numpy(np.ascontiguousarray(states)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def observe(fmt):
        dt = torch.int32 if fmt < 2 else torch.int16
        rows = m if fmt < 2 else (m + 1) // 2 * 2
        o = [torch.zeros((rows, OBS), dtype=dt, device=dev) for _ in range(2)]
        assert lib.pz_observe(st.data_ptr(), m, m, fmt, 0, o[0].data_ptr(), o[1].data_ptr(), stream) == 0
        return [x[:m] for x in o]

    for normalized in (False, True):
        pinned = observe(1 if normalized else 0)
        if normalized:
            pinned = [x.view(torch.float32) for x in pinned]
        for dt in (torch.float16, torch.bfloat16):
            got = observe(FORMAT[(dt, normalized)])
            for i in range(2):
                assert_rows(pinned[i], got[i].view(dt), dt, f"{name} {dt} normalized={normalized} agent {i}")


# ---- 5. the API rules ------------------------------------------------------------------------------------------------
def test_float16_api_rules():
    from pikazoo_amd.wrappers import NormalizeObservation, RewardByBallPosition

    table = (0.0, -0.01, 0.0, 0.01, 0.0, 0.01, 0.0, -0.01)
    raw16 = make_env(num_envs=64, observation_dtype="float16")
    assert raw16.observation_space("player_1").dtype == np.float16
    assert np.array_equal(raw16.observation_space("player_1").high, make_env(num_envs=8).observation_space("player_1").high)
    norm = NormalizeObservation(raw16)
    assert norm.fused is True and raw16.obs_dtype == torch.float16
    sp = norm.observation_space("player_1")
    assert sp.dtype == np.float16 and float(sp.low.min()) == 0.0 and float(sp.high.max()) == 1.0
    assert norm.reset()[0]["player_1"].dtype == torch.float16
    bf = make_env(num_envs=64, observation_dtype=torch.bfloat16)
    assert bf.observation_space("player_1").dtype == np.float32  # numpy has no bfloat16
    assert NormalizeObservation(bf).observation_space("player_1").dtype == np.float32
    # stacks in which an observation-reading wrapper would run outside the kernel, on rounded values
    for dt in ("float16", "bfloat16"):
        with pytest.raises(ValueError, match="NormalizeObservation"):
            NormalizeObservation(NormalizeObservation(make_env(num_envs=8, observation_dtype=dt)))
        with pytest.raises(ValueError, match="RewardByBallPosition"):
            RewardByBallPosition(NormalizeObservation(make_env(num_envs=8, observation_dtype=dt)), table)
        with pytest.raises(ValueError):
            NormalizeObservation(RewardByBallPosition(RewardByBallPosition(make_env(num_envs=8, observation_dtype=dt),
                                                                           table), table))
    # the same stacks on integer rows are unchanged
    assert NormalizeObservation(NormalizeObservation(make_env(num_envs=8))).fused is False
    assert RewardByBallPosition(NormalizeObservation(make_env(num_envs=8, observation_dtype=torch.int16)), table)
    # scalar_api: numpy rows
    with pytest.raises(ValueError, match="bfloat16"):
        make_env(num_envs=1, scalar_api=True, observation_dtype=torch.bfloat16)
    one = make_env(num_envs=1, scalar_api=True, observation_dtype=torch.float16)
    o = one.reset()[0]["player_1"]
    assert isinstance(o, np.ndarray) and o.dtype == np.float16 and o.shape == (35,)
    ref = make_env(num_envs=1, scalar_api=True)
    assert np.array_equal(o, ref.reset()[0]["player_1"].astype(np.float32).astype(np.float16))


def test_checkpoint_moves_between_float16_and_float32_rows():
    from pikazoo_amd.wrappers import NormalizeObservation

    kw = dict(num_envs=256, seed=3, is_player2_computer=True, winning_score=2)
    src = NormalizeObservation(make_env(observation_dtype=torch.bfloat16, **kw))
    src.reset()
    for t in range(30):
        src.step(src.unwrapped.random_actions(2, t))
    dst = NormalizeObservation(make_env(**kw))
    dst.reset()
    dst.unwrapped.load_state_dict(src.unwrapped.state_dict())
    for t in range(30, 80):
        acts = src.unwrapped.random_actions(2, t)
        xs, xd = src.step(acts), dst.step(acts)
        for ag in ("player_1", "player_2"):
            assert_rows(xd[0][ag], xs[0][ag], torch.bfloat16, f"frame {t} {ag}")
            assert torch.equal(xs[1][ag], xd[1][ag])
        assert torch.equal(xs[2]["player_1"], xd[2]["player_1"])
    assert torch.equal(src.unwrapped.state, dst.unwrapped.state)
