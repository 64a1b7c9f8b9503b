"""GPU tests of the egocentric rows: ``pz_ego_rows`` through the C ABI between sentinel guards on every case of
tests/ego_judge.py -- 7 formats x 11 row counts x 18 layouts of pitches, base offsets and in-place calls, and a [3, 65, 35]
slab -- equal to the judge bit for bit with every sentinel and every element of pitch padding intact; the overlap code with
nothing written; ``pz_ego_actions`` in the four action types; the binding into a slot of a rollout buffer and under a captured
graph; ``wrappers.EgocentricObservation`` on real envs of both state formats against a twin env with the same seed and
actions; and both examples with and without ``egocentric``.

PAST ONE GRID STRIDE.  The kernels cap their grid at 2 048 workgroups of 256 and stride; every case above is done in one trip
of their loops (tests/test_ego_host.py proves it on a model of the walks), so the advance of the column, the (row, column) walk
with its carry and the stride ran in none of them.  ``LARGE_CASES`` (7 formats x 9 layouts at about 2.5 strides, in-place
element-by-element calls among them: out of place an element done twice is stored twice with the same value and passes),
the large actions count, a ``[8, 40 001, 35]`` trajectory slab through the binding and one captured replay of each run them."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ego_judge as EJ

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
DEV = torch.device("cuda:0")
TORCH_WORDS = {2: torch.int16, 4: torch.int32}
TORCH_ROWS = {0: torch.int32, 1: torch.float32, 2: torch.int16, 3: torch.float16, 4: torch.bfloat16, 5: torch.float16, 6: torch.bfloat16}


@pytest.fixture(scope="module")
def ego():
    from pikazoo_amd import ego

    ego.load()
    return ego


def upload(words):
    """unsigned numpy words as a device tensor of the same bits"""
    signed = words.view(np.int16 if words.dtype.itemsize == 2 else np.int32)
    return torch.from_numpy(signed.copy()).to(DEV)


def download(t):
    a = t.cpu().numpy()
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def stored(t):
    """a row tensor as the judge's storage array (bfloat16: its bits as uint16)"""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(EJ.FORMATS))
def test_rows_equal_the_judge_between_the_guards(ego, fmt):
    lib = ego.load()
    cases = [c for c in EJ.row_cases() if c["fmt"] == fmt]
    assert len(cases) == len(EJ.ROWS) * len(EJ.LAYOUTS) + 1
    pending = []
    for case in cases:
        src, dst, _ = EJ.case_buffers(case)
        size = src.dtype.itemsize
        d_src = upload(src)
        d_dst = d_src if dst is None else upload(dst)
        assert d_src.data_ptr() % 256 == 0 and d_dst.data_ptr() % 256 == 0
        p_in = d_src.data_ptr() + (EJ.GUARD + case["in_offset"]) * size
        p_out = d_dst.data_ptr() + (EJ.GUARD + case["out_offset"]) * size
        assert not case["inplace"] or p_in == p_out
        rc = lib.pz_ego_rows(p_in, p_out, fmt, case["rows"], case["in_pitch"], case["out_pitch"], None)
        assert rc == 0, (case, rc)
        pending.append((case, src, d_src, d_dst))
    torch.cuda.synchronize()
    for case, src, d_src, d_dst in pending:
        want = EJ.expected_buffer(case)
        got = download(d_dst)
        assert np.array_equal(got, want), (case, np.nonzero(got != want)[0][:8])
        if not case["inplace"]:
            assert np.array_equal(download(d_src), src), case        # the input is read only


@pytest.mark.parametrize("fmt", [0, 5])
def test_overlapping_ranges_are_refused_with_nothing_written(ego, fmt):
    lib = ego.load()
    size = 4 if fmt == 0 else 2
    words = EJ.bits(EJ.encode(EJ.content(16, 0), fmt)).reshape(-1)
    buf = upload(words)
    base = buf.data_ptr()
    row = 35 * size
    for p_in, p_out, rows, ip, op in ((base, base + row, 4, 35, 35), (base + row, base, 4, 35, 35), (base, base + size, 3, 40, 40),
                                      (base, base, 3, 35, 36), (base, base, 3, 36, 35), (base, base + 3 * row + 34 * size, 4, 35, 35),
                                      (base + 2 * row - size, base, 2, 35, 70)):
        assert lib.pz_ego_rows(p_in, p_out, fmt, rows, ip, op, None) == -5, (p_in - base, p_out - base, rows, ip, op)
    assert lib.pz_ego_actions(base, base + 4, 0, 2, None) == -5 and lib.pz_ego_actions(base + 8, base, 1, 2, None) == -5
    torch.cuda.synchronize()
    assert np.array_equal(download(buf), words)
    # ranges that only touch are apart: 4 rows behind 4 rows
    assert lib.pz_ego_rows(base, base + 4 * row, fmt, 4, 35, 35, None) == 0
    torch.cuda.synchronize()
    want = words.copy()
    want[4 * 35:8 * 35] = EJ.bits(EJ.mirror(EJ.encode(EJ.content(16, 0), fmt)[:4], fmt)).reshape(-1)
    assert np.array_equal(download(buf), want)


@pytest.mark.parametrize("dtype", EJ.ACTION_DTYPES)
def test_actions_go_through_pi_and_other_values_pass(ego, dtype):
    lib = ego.load()
    fmt = {np.int32: 0, np.int64: 1, np.uint8: 2, np.int16: 3}[dtype]
    for n in EJ.ACTION_COUNTS:
        for inplace in (False, True):
            a = EJ.action_case(dtype, n)
            guard = np.full(16, 77, dtype)
            src = torch.from_numpy(np.concatenate([guard, a, guard])).to(DEV)
            dst = src if inplace else torch.from_numpy(np.concatenate([guard, np.full(n, 99, dtype), guard])).to(DEV)
            size = a.dtype.itemsize
            assert lib.pz_ego_actions(src.data_ptr() + 16 * size, dst.data_ptr() + 16 * size, fmt, n, None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(dst.cpu().numpy(), np.concatenate([guard, EJ.mirror_actions(a), guard])), (dtype, n, inplace)
    values = torch.from_numpy(EJ.action_values(dtype)).to(DEV)
    assert ego.mirror_actions(values).cpu().numpy().tolist()[:18] == list(EJ.PI)
    assert torch.equal(ego.mirror_actions(ego.mirror_actions(values)), values)
    assert ego.mirror_actions(values, out=values) is values and values.cpu().numpy().tolist()[18:] == EJ.action_values(dtype).tolist()[18:]


# ---- past one grid stride --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(EJ.FORMATS))
def test_large_rows_equal_the_judge_between_the_guards(ego, fmt):
    """LARGE_CASES as above, one case on the device at a time: every thread of the launch takes two trips and some a third"""
    lib = ego.load()
    cases = [c for c in EJ.LARGE_CASES if c["fmt"] == fmt]
    assert len(cases) == len(EJ.LARGE_FLAT) + len(EJ.LARGE_PITCHED)
    for case in cases:
        buffers = EJ.case_buffers(case)
        src, dst, _ = buffers
        size = src.dtype.itemsize
        d_src = upload(src)
        d_dst = d_src if dst is None else upload(dst)
        assert d_src.data_ptr() % 256 == 0 and d_dst.data_ptr() % 256 == 0
        p_in = d_src.data_ptr() + (EJ.GUARD + case["in_offset"]) * size
        p_out = d_dst.data_ptr() + (EJ.GUARD + case["out_offset"]) * size
        assert not case["inplace"] or p_in == p_out
        rc = lib.pz_ego_rows(p_in, p_out, fmt, case["rows"], case["in_pitch"], case["out_pitch"], None)
        assert rc == 0, (case, rc)
        torch.cuda.synchronize()
        want = EJ.expected_buffer(case, buffers=buffers)
        got = download(d_dst)
        assert np.array_equal(got, want), (case, np.nonzero(got != want)[0][:8], int((got != want).sum()))
        if not case["inplace"]:
            assert np.array_equal(download(d_src), src), case        # the input is read only
        del d_src, d_dst


@pytest.mark.parametrize("dtype", EJ.ACTION_DTYPES)
def test_large_actions_go_through_pi_on_every_trip(ego, dtype):
    lib = ego.load()
    fmt = {np.int32: 0, np.int64: 1, np.uint8: 2, np.int16: 3}[dtype]
    n = EJ.LARGE_ACTION_COUNT
    a = EJ.action_case(dtype, n)
    guard = np.full(16, 77, dtype)
    want = np.concatenate([guard, EJ.mirror_actions(a), guard])
    for inplace in (False, True):
        src = torch.from_numpy(np.concatenate([guard, a, guard])).to(DEV)
        dst = src if inplace else torch.from_numpy(np.concatenate([guard, np.full(n, 99, dtype), guard])).to(DEV)
        size = a.dtype.itemsize
        assert lib.pz_ego_actions(src.data_ptr() + 16 * size, dst.data_ptr() + 16 * size, fmt, n, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), (dtype, inplace, np.nonzero(got != want)[0][:8])
        assert inplace or np.array_equal(src.cpu().numpy()[16:-16], a)


def as_rows(host, fmt):
    t = torch.from_numpy((host.view(np.int16) if host.dtype == np.uint16 else host).copy()).to(DEV)   # (a copy: the shared rows are read-only)
    return t.view(torch.bfloat16) if fmt in (4, 6) else t


def test_mirror_of_a_trajectory_slab_past_one_stride(ego):
    """"one launch serves a step's [n, 35] and a trajectory's [k, n, 35]" -- here with k * n = 320 008 bfloat16
    rows, 1.4 million 16-byte pieces, about 2.7 strides of the flat path: in place, and into a slot of a larger buffer"""
    fmt, k, n = 6, 8, 40001
    host, want = (x.reshape(k, n, EJ.DIM) for x in EJ.large_rows(fmt, k * n, 3))
    slab = as_rows(host, fmt)
    buf = torch.zeros((3, k, n, EJ.DIM), dtype=torch.bfloat16, device=DEV)
    assert ego.mirror(slab, True, out=buf[1]).data_ptr() == buf[1].data_ptr()
    torch.cuda.synchronize()
    assert np.array_equal(stored(buf[1]), want) and not buf[0].any() and not buf[2].any()
    assert np.array_equal(stored(slab), host)
    assert ego.mirror(slab, True, out=slab) is slab
    torch.cuda.synchronize()
    assert np.array_equal(stored(slab), want)


def test_large_launches_under_a_captured_graph(ego):
    """one replay of the large aligned flat case and of the large actions count; every captured tensor lives until after it"""
    fmt, n = 1, EJ.LARGE_ROWS[4]
    host, want = EJ.large_rows(fmt, n, 1)
    rows = as_rows(np.zeros_like(host), fmt)
    out = torch.zeros_like(rows)
    a = EJ.action_case(np.int64, EJ.LARGE_ACTION_COUNT)
    actions = torch.zeros(len(a), dtype=torch.int64, device=DEV)
    mapped = torch.zeros_like(actions)
    ego.mirror(rows, out=out)
    ego.mirror_actions(actions, out=mapped)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ego.mirror(rows, out=out)
        ego.mirror_actions(actions, out=mapped)
    rows.copy_(as_rows(host, fmt))
    actions.copy_(torch.from_numpy(a).to(DEV))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(EJ.bits(stored(out)), EJ.bits(want)) and np.array_equal(EJ.bits(stored(rows)), EJ.bits(host))
    assert np.array_equal(mapped.cpu().numpy(), EJ.mirror_actions(a)) and np.array_equal(actions.cpu().numpy(), a)
    del graph                                   # (the graph first: rows, out, actions and mapped outlive it)


# ---- the binding -----------------------------------------------------------------------------------------------------------------
def rows_on_device(fmt, shape, seed):
    count = int(np.prod(shape[:-1]))
    host = EJ.encode(EJ.content(count, seed), fmt).reshape(shape)
    t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(DEV)
    return host, (t.view(torch.bfloat16) if fmt in (4, 6) else t)


@pytest.mark.parametrize("fmt", list(EJ.FORMATS))
def test_mirror_into_a_slot_of_a_rollout_buffer(ego, fmt):
    k, n = 3, 65
    normalized = None if fmt in (0, 1, 2) else fmt in EJ.NORMALISED
    host, rows = rows_on_device(fmt, (n, 35), 2)
    buf = torch.zeros((k, n, 35), dtype=TORCH_ROWS[fmt], device=DEV)
    assert ego.mirror(rows, normalized, out=buf[1]) .data_ptr() == buf[1].data_ptr()
    want = EJ.mirror(host, fmt)
    assert np.array_equal(EJ.bits(stored(buf[1])), EJ.bits(want)) and not buf[0].any() and not buf[2].any()
    fresh = ego.mirror(rows, normalized)
    assert fresh.is_contiguous() and np.array_equal(EJ.bits(stored(fresh)), EJ.bits(want)) and np.array_equal(EJ.bits(stored(rows)), EJ.bits(host))
    # a whole slab, in place; a slice of rows from row 1; the front of a wider tensor
    slab_host, slab = rows_on_device(fmt, (k, n, 35), 3)
    assert ego.mirror(slab, normalized, out=slab) is slab
    assert np.array_equal(EJ.bits(stored(slab)), EJ.bits(EJ.mirror(slab_host, fmt)))
    part = ego.mirror(rows[1:], normalized)
    assert np.array_equal(EJ.bits(stored(part)), EJ.bits(want[1:]))
    wide = torch.zeros((n, 48), dtype=TORCH_ROWS[fmt], device=DEV)
    ego.mirror(rows, normalized, out=wide[:, :35])
    assert np.array_equal(EJ.bits(stored(wide[:, :35].contiguous())), EJ.bits(want)) and not wide[:, 35:].any()
    assert tuple(ego.mirror(rows[:0], normalized).shape) == (0, 35)
    with pytest.raises(ValueError, match="overlaps"):
        ego.mirror(slab[0], normalized, out=slab.view(-1)[35:35 * (n + 1)].view(n, 35))


def test_mirror_under_a_captured_graph(ego):
    fmt, n = 6, 257
    host, rows = rows_on_device(fmt, (n, 35), 0)
    buf = torch.zeros((2, n, 35), dtype=torch.bfloat16, device=DEV)
    actions = torch.zeros(n, dtype=torch.int64, device=DEV)
    mapped = torch.zeros_like(actions)
    ego.mirror(rows, True, out=buf[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ego.mirror(rows, True, out=buf[1])
        ego.mirror_actions(actions, out=mapped)
    for replay in range(3):
        host, fresh = rows_on_device(fmt, (n, 35), 5 + replay)
        rows.copy_(fresh)
        a = EJ.action_case(np.int64, n) if replay else np.arange(n, dtype=np.int64) % 18
        actions.copy_(torch.from_numpy(np.roll(a, replay)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(stored(buf[1]), EJ.mirror(host, fmt)), replay
        assert np.array_equal(mapped.cpu().numpy(), EJ.mirror_actions(np.roll(a, replay))), replay
    assert not buf[0].any()


# ---- the wrapper on real envs ---------------------------------------------------------------------------------------------------
def make_pair(below=(), above=(), agents=("player_2",), **env_kw):
    """(the wrapped env, its twin without EgocentricObservation): same seed, same stack"""
    from pikazoo_amd import pikazoo_v0, wrappers

    def stack(with_ego):
        env = pikazoo_v0.env(device=DEV, seed=5, winning_score=1, **env_kw)
        for name in below:
            env = getattr(wrappers, name)(env)
        if with_ego:
            env = wrappers.EgocentricObservation(env, agents=agents)
        for name in above:
            env = getattr(wrappers, name)(env)
        return env

    return stack(True), stack(False)


def check_obs(got, want, fmt, mirrored, what):
    for a in ("player_1", "player_2"):
        rows = stored(want[a])
        expect = EJ.mirror(rows, fmt) if a in mirrored else rows
        assert got[a].dtype == want[a].dtype and np.array_equal(EJ.bits(stored(got[a])), EJ.bits(expect)), (what, a)


PAIRS = {
    "int32 state, 18 actions": dict(num_envs=33),
    "packed state, 18 actions": dict(num_envs=33, state_format="packed"),
    "SimplifyAction": dict(num_envs=33, below=("SimplifyAction",)),
    "NormalizeObservation below": dict(num_envs=33, below=("SimplifyAction", "NormalizeObservation")),
    "NormalizeObservation above": dict(num_envs=33, state_format="packed", above=("NormalizeObservation",)),
    "bfloat16 rows": dict(num_envs=33, observation_dtype=torch.bfloat16),
    "bfloat16 rows, normalised above": dict(num_envs=34, observation_dtype=torch.bfloat16, below=("SimplifyAction",), above=("NormalizeObservation",)),
    "float16 rows, normalised below": dict(num_envs=33, observation_dtype=torch.float16, state_format="packed", below=("NormalizeObservation",)),
    "int16 rows, int16 actions": dict(num_envs=33, observation_dtype=torch.int16, action_dtype=torch.int16),
    "frame_skip 2": dict(num_envs=32, frame_skip=2),
    "output_ring 2": dict(num_envs=33, output_ring=2, below=("NormalizeObservation",)),
    "both agents": dict(num_envs=33, agents=("player_1", "player_2"), action_dtype=torch.uint8),
    "no auto_reset": dict(num_envs=33, auto_reset=False, steps=12),
}


@pytest.mark.parametrize("name", list(PAIRS))
def test_the_wrapper_against_a_twin_env(ego, name):
    kw = dict(PAIRS[name])
    steps, action_dtype = kw.pop("steps", 90), kw.pop("action_dtype", torch.int64)
    env, twin = make_pair(**kw)
    n, mirrored = kw["num_envs"], kw.get("agents", ("player_2",))
    ring = kw.get("output_ring", 1)
    fmt = lambda: int(twin.unwrapped._cfg.normalize_obs)  # noqa: E731
    A = env.action_space("player_2").n
    assert A == twin.action_space("player_2").n == (13 if "SimplifyAction" in kw.get("below", ()) else 18)
    obs, _ = env.reset()
    want, _ = twin.reset()
    assert int(env.unwrapped._cfg.normalize_obs) == fmt()
    check_obs(obs, want, fmt(), mirrored, "reset")
    for a in ("player_1", "player_2"):
        assert obs[a].data_ptr() != env.unwrapped._obs_view(0 if a == "player_1" else 1).data_ptr() or a not in mirrored
    gen = torch.Generator().manual_seed(3)
    ended, previous = 0, None
    for t in range(steps):
        acts = {a: torch.randint(A, (n,), generator=gen).to(action_dtype).to(DEV) for a in ("player_1", "player_2")}
        theirs = {a: (ego.mirror_actions(v) if (A == 18 and a in mirrored) else v.clone()) for a, v in acts.items()}
        kept = {a: v.clone() for a, v in acts.items()}
        obs, rew, term, trunc, _ = env.step(acts)
        want, want_rew, want_term, _, _ = twin.step(theirs)
        check_obs(obs, want, fmt(), mirrored, t)
        for a in ("player_1", "player_2"):
            assert torch.equal(rew[a], want_rew[a]) and torch.equal(term[a], want_term[a]) and not trunc[a].any(), (t, a)
            assert torch.equal(acts[a], kept[a]), (t, a)                      # the caller's actions are not written
        if ring == 2 and previous is not None:                                 # the previous step's rows are intact
            for a in ("player_1", "player_2"):
                assert np.array_equal(EJ.bits(stored(previous[0][a])), previous[1][a]), (t, a)
        previous = (obs, {a: EJ.bits(stored(obs[a])).copy() for a in obs})
        ended += int(term["player_1"].sum())
        if t == steps // 2 and kw.get("auto_reset", True):                                    # reset(mask=): only some games, every row right
            mask = torch.arange(n, device=DEV) % 3 == 0
            obs, _ = env.reset(mask=mask)
            want, _ = twin.reset(mask=mask)
            check_obs(obs, want, fmt(), mirrored, "masked reset")
            previous = None
    assert torch.equal(env.unwrapped.state, twin.unwrapped.state)
    if kw.get("auto_reset", True):
        assert ended >= 5, ended                                               # (across episode ends)


def test_the_wrapper_step_under_a_captured_graph(ego):
    env, twin = make_pair(num_envs=64, below=("NormalizeObservation",), validate_actions=False)
    obs, _ = env.reset()
    twin.reset()
    acts = {a: torch.zeros(64, dtype=torch.int64, device=DEV) for a in ("player_1", "player_2")}
    obs, *_ = env.step(acts)
    twin.step({a: v.clone() for a, v in acts.items()})
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, rew, term, _, _ = env.step(acts)
    gen = torch.Generator().manual_seed(1)
    for replay in range(3):
        for a in acts:
            acts[a].copy_(torch.randint(18, (64,), generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        want, want_rew, want_term, _, _ = twin.step({"player_1": acts["player_1"].clone(), "player_2": ego.mirror_actions(acts["player_2"])})
        check_obs(obs, want, 1, ("player_2",), replay)
        assert torch.equal(rew["player_1"], want_rew["player_1"]) and torch.equal(term["player_2"], want_term["player_2"])


def test_observation_space_and_refusals(ego):
    from pikazoo_amd import pikazoo_v0, wrappers

    def raw(**kw):
        return pikazoo_v0.env(num_envs=4, device=DEV, **kw)

    for dtype, np_dtype in ((torch.int32, np.int32), (torch.int16, np.int16), (torch.float16, np.float16), (torch.bfloat16, np.float32)):
        inner = raw(observation_dtype=dtype)
        env = wrappers.EgocentricObservation(inner)
        box, plain = env.observation_space("player_2"), inner.observation_space("player_2")
        assert box is env.observation_space("player_2") and box.dtype == np_dtype and box.shape == (35,)
        assert box.low[26] == 0 and box.high[26] == 412 and plain.low[26] == 20 and plain.high[26] == 432
        others = [j for j in range(35) if j != 26]
        assert np.array_equal(box.low[others], plain.low[others]) and np.array_equal(box.high[others], plain.high[others])
        assert env.observation_space("player_1") is plain and env.action_space("player_2").n == 18
        # every bound is the mirror of a bound
        low, high = EJ.mirror(plain.low.astype(np.int32)[None], 0)[0], EJ.mirror(plain.high.astype(np.int32)[None], 0)[0]
        assert np.array_equal(np.minimum(low, high), box.low.astype(np.int32)) and np.array_equal(np.maximum(low, high), box.high.astype(np.int32))
    env = wrappers.EgocentricObservation(wrappers.NormalizeObservation(raw()), agents="player_2")
    assert env.observation_space("player_2") is env.env.observation_space("player_2") and env.observation_space("player_2").high.max() == 1
    assert isinstance(env, wrappers.BaseParallelWrapper) and "EgocentricObservation" in wrappers.__all__ and env.mirrored == ("player_2",)
    assert wrappers.EgocentricObservation(raw(), agents=["player_2", "player_1"]).mirrored == ("player_1", "player_2")
    with pytest.raises(ValueError, match="scalar_api"):
        wrappers.EgocentricObservation(pikazoo_v0.env(device=DEV, scalar_api=True))
    with pytest.raises(ValueError, match="PixelObservation"):
        from pikazoo_amd.render import synthetic_sprites

        wrappers.EgocentricObservation(wrappers.PixelObservation(raw(render_mode="rgb_array", sprites=synthetic_sprites(7, DEV))))
    for agents in (("player_3",), ("player_1", "nobody"), (), "player"):
        with pytest.raises(ValueError, match="agents"):
            wrappers.EgocentricObservation(raw(), agents=agents)
    # step_many stays reachable through unwrapped, and ego.mirror serves its slab
    env = wrappers.EgocentricObservation(raw())
    env.reset()
    traj = env.unwrapped.step_many(torch.zeros((3, 2, 4), dtype=torch.int32, device=DEV))
    slab = traj["obs"]["player_2"]
    assert tuple(slab.shape) == (3, 4, 35)
    assert np.array_equal(stored(ego.mirror(slab)), EJ.mirror(stored(slab), 0))


# ---- the examples ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("example", ["ppo_league", "ppo_selfplay"])
def test_the_examples_with_and_without_egocentric(ego, example):
    sys.path.insert(0, str(REPO / "examples"))
    module = __import__(example)
    kw = dict(num_envs=256, iters=2, steps=8, log=lambda line: None)
    if example == "ppo_league":
        kw["snapshot_every"] = 1
    plain = module.main(**kw)
    off = module.main(egocentric=False, **kw)
    on = module.main(egocentric=True, **kw)
    assert plain == off and len(on) == len(off) == 16
    assert all(np.isfinite(on)) and all(np.isfinite(off)) and on != off
