"""GPU tests (``-m gpu``) of the k-step trajectory launches of a frame-skip env: ``pz_step_many_held`` /
``pz_rollout_random_held`` (the ``held_traj_kernel`` family) and ``raw_env.step_many_held`` / ``rollout_random_held``, on
the structural cases of tests/held_rollout_cases.py (the runtime configurations of every instantiation, from planted
states: tests/test_gpu_held_configs.py, through ``Launch`` / ``check_case`` here).

The judge is ``HeldOracle`` (tests/frame_skip_judge.py): the CPU oracle driven as the loop that defines frame skip,
pinned to the unmodified reference by tests/golden/frame_skip_k4.npz.  Every launch is compared with it slab by slab and
bit for bit -- integers, normalized float32 rows, 16-bit row patterns, float32 reward sums against the judge's numpy
float32 sums; no GPU result is ever the expected value.  ``hold == 1`` cases are the plain trajectory semantics (the judge
at one frame per step is the oracle's own step), ``k == 1`` cases one held step.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from frame_skip_judge import HeldOracle
from held_configs import hold_kernels
from held_rollout_cases import CASES, N_ABOVE, STACKS, TABLE, held_traj_kernels, judge_counts, make_judge, policy
from kernel_configs import ACTION_FORMATS

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
WORDS, OBS, PAD, SLICE = 44, 35, 64, 512
SENT = -7  # what the output buffers hold before a launch


def cpu(t):
    return t.detach().cpu().numpy()


def rows_as(ref_obs, fmt):
    """The judge's rows -- int32, or the float32 NormalizeObservation quotient -- as the bit patterns a buffer of format
    `fmt` holds (2-byte rows widened to int32; float formats rounded to nearest even: a plain cast)"""
    if fmt == 1:
        return ref_obs.view(np.int32)
    if fmt in (0, 2):
        return ref_obs
    dt = torch.float16 if fmt in (3, 5) else torch.bfloat16
    return torch.from_numpy(np.ascontiguousarray(ref_obs)).to(torch.float32).to(dt).view(torch.int16).numpy().astype(np.int32)


def kernel_name(raw):
    return raw.replace("void ", "").split("(")[0].replace("pz::", "")


def tables_of(mode, dev):
    from pikazoo_amd.env import flight_tables

    return {"both": lambda: flight_tables(dev)[0], "power_hit": lambda: flight_tables(dev, landing=False)[0],
            "none": lambda: None}[mode]()


ACTION_DTYPES = {"i32": torch.int32, "i64": torch.int64, "u8": torch.uint8, "i16": torch.int16}


class Launch:
    """One launch of `c` (a held_rollout_cases.Case or a held_configs.HeldConfig) through the C ABI from `start`
    ([44][n] int32, the judge's state) into sentinel-filled buffers.  ``pz_step_held`` (entry "held"): k launches in a
    row, launch t on row t of the tape in the caller's element type, into output slot t."""

    def __init__(self, c, oracle, start, stats0, tape=None):
        from pikazoo_amd import _native

        self.c, self.lib, dev = c, _native.load(), torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        n, k, fmt = c.n, c.k, c.obs_format
        self.n, self.stride = n, n + c.stride_pad
        stride = self.stride
        self.cfg = _native.PzConfig.from_buffer_copy(oracle.make_config(**c.oracle_kwargs()))
        self.cfg.packed_state, self.cfg.normalize_obs, self.cfg.action_format = int(c.packed), fmt, ACTION_FORMATS[c.action_format]
        self.faults = torch.zeros(1, dtype=torch.int64, device=dev)
        self.cfg.action_faults = self.faults.data_ptr()
        self.tables = tables_of(c.tables, dev)
        self.flat_state = torch.full((WORDS * stride + PAD,), -99, dtype=torch.int32, device=dev)
        self.state = self.flat_state[:WORDS * stride].view(WORDS, stride)
        self.state[:, :n] = torch.from_numpy(start).to(dev)
        self.packed = None
        if c.packed:
            self.packed = torch.full((36 * stride + PAD,), 0xA5, dtype=torch.uint8, device=dev)
            misfits = torch.zeros(1, dtype=torch.int64, device=dev)
            assert self.lib.pz_pack_state(self.state.data_ptr(), n, stride, self.packed.data_ptr(), stride,
                                          misfits.data_ptr(), self.stream) == 0
            torch.cuda.synchronize()
            assert int(misfits.item()) == 0
        self.with_stats = c.stats_ptr  # (a statistics mode without a pointer: nothing may be written through it)
        self.stats = torch.zeros(20 * stride, dtype=torch.uint8, device=dev)
        self.ret = self.stats[:16 * stride].view(torch.float64).view(2, stride)
        self.lengths = self.stats[16 * stride:].view(torch.int32)
        if stats0 is not None:
            self.ret[:, :n] = torch.from_numpy(stats0[:16 * n].view(np.float64).reshape(2, n).copy()).to(dev)
            self.lengths[:n] = torch.from_numpy(stats0[16 * n:].view(np.int32).copy()).to(dev)
        odt = torch.int16 if fmt >= 2 else torch.int32
        self.obs = [torch.full(((k * n + PAD) * OBS,), SENT, dtype=odt, device=dev) for _ in range(2)]
        self.rew = [torch.full((k * n + PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(2)]
        self.term = torch.full((k * n + PAD,), 9, dtype=torch.uint8, device=dev)
        self.act = torch.full((k * 2 * n + PAD,), SENT, dtype=torch.int32, device=dev)
        self.done = torch.zeros(1, dtype=torch.int64, device=dev)
        self.tape = None if tape is None else torch.from_numpy(np.ascontiguousarray(tape, np.int32)).to(dev)
        if c.entry == "held":
            self.tape = self.tape.to(ACTION_DTYPES[c.action_format]).contiguous()
        else:
            assert c.action_format == "i32"  # the tape of a trajectory launch is int32 alone
        torch.cuda.synchronize()

    def run(self):
        c, lib = self.c, self.lib
        sp = self.stats.data_ptr() if self.with_stats else None
        tb = None if self.tables is None else C.byref(self.tables)
        state_ptr = self.packed.data_ptr() if c.packed else self.state.data_ptr()
        n = self.n

        def slot(t):  # the outputs of pz_step_held's launch t
            return (self.obs[0][t * n * OBS:].data_ptr(), self.obs[1][t * n * OBS:].data_ptr(), self.rew[0][t * n:].data_ptr(),
                    self.rew[1][t * n:].data_ptr(), self.term[t * n:].data_ptr(), sp, self.done.data_ptr(), tb, self.stream)

        outs = slot(0)
        launches = c.k if c.entry == "held" else 1
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            if c.entry == "held":
                for t in range(c.k):
                    err = lib.pz_step_held(state_ptr, n, self.stride, C.byref(self.cfg), self.tape[t, 0].data_ptr(),
                                           self.tape[t, 1].data_ptr(), c.hold, *slot(t))
                    assert err == 0, (c.id, t, err)
            elif c.entry == "many":
                err = lib.pz_step_many_held(state_ptr, self.n, self.stride, C.byref(self.cfg), self.tape.data_ptr(), c.k,
                                            c.hold, *outs)
            else:
                err = lib.pz_rollout_random_held(state_ptr, self.n, self.stride, C.byref(self.cfg), c.action_seed, c.t0, c.k,
                                                 c.hold, self.act.data_ptr(), *outs)
            assert err == 0, (c.id, err)
            torch.cuda.synchronize()
        device_events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        assert device_events, "torch.profiler recorded no device kernel: the dispatched-kernel check cannot run"
        assert [kernel_name(e.name) for e in device_events if "pz::" in e.name] == [c.kernel] * launches, \
            (c.id, sorted({e.name for e in device_events}))
        assert c.kernel in (hold_kernels() if c.entry == "held" else held_traj_kernels())

    def check_nothing_written_outside(self):
        c, n, stride, k = self.c, self.n, self.stride, self.c.k
        if c.packed:
            p = self.packed
            assert all(bool((part == 0xA5).all()) for part in (p[16 * n:16 * stride], p[16 * stride + 16 * n:32 * stride],
                                                             p[32 * stride + 4 * n:])), "packed state past lane n"
            flagged = torch.zeros(1, dtype=torch.int64, device=p.device)
            self.flat_state.fill_(-99)
            assert self.lib.pz_unpack_state(p.data_ptr(), n, stride, self.state.data_ptr(), stride, flagged.data_ptr(),
                                            self.stream) == 0
            torch.cuda.synchronize()
            assert int(flagged.item()) == 0
        assert bool((self.state[:, n:] == -99).all()) and bool((self.flat_state[WORDS * stride:] == -99).all()), \
            "state past lane n"
        for o in self.obs:
            assert bool((o[k * n * OBS:] == SENT).all()), "observation rows past slab k"
        for r in self.rew:
            assert bool((r[k * n:] == SENT).all()), "rewards past slab k"
        assert bool((self.term[k * n:] == 9).all()), "terminations past slab k"
        written = k * 2 * n if c.entry == "rollout" else 0
        assert bool((self.act[written:] == SENT).all()), "actions past slab k (or written by the tape launch)"
        if self.with_stats:
            assert bool((self.ret[:, n:] == 0).all()) and bool((self.lengths[n:] == 0).all()), "statistics past lane n"
        else:
            assert bool((self.stats == 0).all()), "statistics written without a statistics pointer"


def check_case(c, oracle):
    """Launch `c`, then judge it: every slab's rows, rewards and `terminated`, the actions pz_rollout_random_held writes,
    the final state, the statistics, episodes_done (all exact, on every lane), nothing outside lane n / slab k, and --
    hold > 1, k >= 16 -- the judge's own counters say that the case bit.  Returns the judge's counts (judge_counts).

    On top of the bit-for-bit comparison, float32 rewards under auto_reset are held against the float64 sum of the
    judge's per-frame float32 rewards r_1 .. r_hold, within ``hold * 2**-24 * sum(|r_j|)``.  Derivation: the device sums
    in frame order from +0.0f, s_j = fl(s_{j-1} + r_j).  The first add is exact.  Every later one is off by at most half
    an ulp of its result, 2**-24 times a partial sum that is itself bounded by T = sum(|r_j|) plus the error so far:
    e_j <= e_{j-1} (1 + 2**-24) + 2**-24 T, so e_hold <= T ((1 + 2**-24)**(hold - 1) - 1) < hold * 2**-24 * T for every
    hold below 2**12.  A frame counted twice, dropped, or summed into the wrong slab misses it by a whole reward."""
    n, k, fmt = c.n, c.k, c.obs_format
    # the judge runs the whole batch (the exact episodes_done, every lane's rewards / flags / actions / final state); the
    # observation rows are compared on every lane below the size switch, on three slices of 512 lanes at and above it
    spans = [(0, n)] if n < N_ABOVE else [(0, SLICE), (n // 2 - 300, n // 2 - 300 + SLICE), (n - SLICE, n)]
    judge = make_judge(oracle, c)
    start = judge.state.copy()
    stats0 = None if judge.env.stats is None else judge.env.stats.copy()
    tape = None
    if c.entry in ("many", "held"):
        tape = np.stack([np.stack(policy(oracle, c, t)) for t in range(k)])  # [k][2][n]
    run = Launch(c, oracle, start, stats0, tape)
    run.run()
    run.check_nothing_written_outside()
    assert int(run.faults.item()) == 0

    h_obs = [[cpu(o[:k * n * OBS].view(k, n, OBS)[:, lo:hi]).astype(np.int32) for lo, hi in spans] for o in run.obs]
    h_rew = [cpu(r[:k * n].view(k, n)) for r in run.rew]
    h_term = cpu(run.term[:k * n].view(k, n))
    h_act = cpu(run.act[:k * 2 * n].view(k, 2, n)) if c.entry == "rollout" else None
    terms, ended = [], 0
    frozen = (judge.state[oracle.E_GAME_ENDED] != 0) & (not c.auto_reset)
    judge64 = judge.float_rewards and bool(c.auto_reset)
    sum64, abs64 = np.zeros((2, n)), np.zeros((2, n))

    def on_frame(j, env, _):  # the float64 judge of a slab's reward: the frame rewards, exactly
        if j == 0:
            sum64[:], abs64[:] = 0.0, 0.0
        for p in range(2):
            sum64[p] += env.rew[p].astype(np.float64)
            abs64[p] += np.abs(env.rew[p].astype(np.float64))

    if judge64:
        judge.on_frame = on_frame
    for t in range(k):
        a1, a2 = policy(oracle, c, t)
        if h_act is not None:
            assert np.array_equal(h_act[t, 0], a1) and np.array_equal(h_act[t, 1], a2), (c.id, t, "actions")
        robs, rrew, rterm = judge.step(a1, a2)
        for p in range(2):
            for i, (lo, hi) in enumerate(spans):
                assert np.array_equal(h_obs[p][i][t], rows_as(robs[p][lo:hi], fmt)), \
                    (c.id, lo, t, f"observations of player {p + 1}")
            assert rrew[p].dtype == (np.float32 if judge.float_rewards else np.int32)
            assert np.array_equal(h_rew[p][t], rrew[p].view(np.int32)), (c.id, t, f"rewards of player {p + 1}")
            if judge64:
                err = np.abs(h_rew[p][t].view(np.float32).astype(np.float64) - sum64[p])
                bound = c.hold * 2.0 ** -24 * abs64[p]
                assert bool((err <= bound).all()), \
                    (c.id, t, f"rewards of player {p + 1} vs float64: {err.max()} (bound {bound[err.argmax()]})")
        assert np.array_equal(h_term[t], rterm), (c.id, t, "terminations")
        ended += int(((rterm != 0) & ~frozen).sum())
        frozen = (rterm != 0) & (not c.auto_reset)
        terms.append(rterm.copy())
    got = cpu(run.state[:, :n])
    if not np.array_equal(got, judge.state):
        f, l = np.argwhere(got != judge.state)[0]
        pytest.fail(f"{c.id}: lane {l} word {oracle.FIELD_NAMES[f]}: hip {got[f, l]} != judge {judge.state[f, l]}")
    if run.with_stats:
        assert np.array_equal(cpu(run.ret[:, :n]), judge.episode_returns), (c.id, "episode returns")
        assert np.array_equal(cpu(run.lengths[:n]), judge.episode_lengths), (c.id, "episode lengths")
    inside, last, revived, twice = judge_counts(judge, np.stack(terms))
    # one ending per game and policy step: the judge's two counters are all of them
    assert int(run.done.item()) == ended == inside + last, (c.id, "episodes_done")
    if c.bites:
        assert inside > 0, "no game ended inside a repeat"
        assert last > 0, "no game ended on a repeat's last frame"
        if c.auto_reset:
            assert revived > 0, "no game was terminated in one slab and running in the next"
    if c.ends_twice:
        assert twice > 0, "no game ended twice inside the launch"
    return inside, last, revived, twice


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_held_trajectory_launch_vs_the_judge(case, oracle):
    check_case(case, oracle)


def test_the_cases_launch_every_instantiation_and_cover_every_axis():
    assert {c.kernel for c in CASES} == held_traj_kernels()
    assert {c.hold for c in CASES} == {1, 2, 3, 4, 8} and {c.k for c in CASES} == {1, 5, 16, 32, 70, 130}
    assert {c.obs_format for c in CASES} == set(range(7)) and {c.tables for c in CASES} == {"both", "power_hit", "none"}
    assert {c.players for c in CASES} == {"hh", "hc", "ch", "cc"} and {c.auto_reset for c in CASES} == {True, False}
    assert {c.stack for c in CASES} == set(STACKS) and any(c.n >= N_ABOVE for c in CASES)
    assert any(c.n % 64 and c.stride_pad for c in CASES) and any(c.ends_twice for c in CASES)


# ------------------------------------------------------------------------------------------------
# the reference itself, in one launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["int32", "packed"])
@pytest.mark.parametrize("tables", ["both", "power_hit", "none"])
def test_the_reference_stepped_with_held_actions_in_one_launch(oracle, tables, packed):
    """tests/golden/frame_skip_k4.npz -- the unmodified reference, 400 policy steps of 6 games held for 4 frames -- as ONE
    pz_step_many_held(k = 400, hold = 4) on 8 lanes (n % 4 == 0; games are independent and ids global: lanes 6 - 7 are
    two further games fed action 0).  k = 400 crosses six tape-chunk refills."""
    from conftest import GOLDEN
    from held_rollout_cases import Case

    d = dict(np.load(GOLDEN / "frame_skip_k4.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    kw, lanes, k = meta["env_kwargs"], meta["lanes"], meta["steps"]
    assert (lanes, k, meta["frame_skip"], kw["winning_score"], kw["is_player2_computer"]) == (6, 400, 4, 2, True)
    c = Case(entry="many", hold=4, k=k, players="hc", tables=tables, packed=packed, n=8, winning_score=2,
             seed=meta["seed"], env_id_base=meta["env_id_base"])
    init = oracle.OracleEnv(8, oracle.make_config(**c.oracle_kwargs()))
    init.reset()
    assert np.array_equal(init.state[:, :lanes], d["state0"])
    tape = np.zeros((k, 2, 8), np.int32)
    tape[:, :, :lanes] = d["actions"].astype(np.int32)
    run = Launch(c, oracle, init.state, None, tape)
    run.run()
    run.check_nothing_written_outside()
    for p in range(2):
        assert np.array_equal(cpu(run.obs[p][:k * 8 * OBS].view(k, 8, OBS)[:, :lanes]), d["obs"][:, p])
        assert np.array_equal(cpu(run.rew[p][:k * 8].view(k, 8)[:, :lanes]), d["rew"][:, p])
    assert np.array_equal(cpu(run.term[:k * 8].view(k, 8)[:, :lanes]), d["term"])
    final = d["states"][k - 1].astype(np.int32)
    final[43] = d["rng_counter"][k - 1]
    assert np.array_equal(cpu(run.state[:, :lanes]), final)
    assert meta["ended_inside"] > 0 and meta["ended_last"] > 0


# ------------------------------------------------------------------------------------------------
# the Python methods
# ------------------------------------------------------------------------------------------------
def make_env(oracle, n, skip, players="hc", tables="both", fmt="int32", stack=False, ws=1, seed=11, auto_reset=True, **kw):
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd import wrappers as W

    p1, p2 = {"hh": (False, False), "hc": (False, True), "ch": (True, False), "cc": (True, True)}[players]
    env = pikazoo_v0.env(num_envs=n, device="cuda:0", seed=seed, winning_score=ws, is_player1_computer=p1,
                         is_player2_computer=p2, flight_tables=tables, state_format=fmt, auto_reset=auto_reset,
                         frame_skip=skip, **kw)
    okw = dict(winning_score=ws, is_player1_computer=p1, is_player2_computer=p2, auto_reset=auto_reset, seed=seed)
    if stack:
        env = W.NormalizeObservation(W.RecordEpisodeStatistics(W.RewardByBallPosition(W.SimplifyAction(env), TABLE)))
        okw.update(simplify_action=True, additional_reward=TABLE, episode_stats=2, normalize_obs=True)
        assert not env.unwrapped._unfused
    return env, HeldOracle(oracle, n, skip, oracle.make_config(**okw))


def judge_trajectory(oracle, raw, ref, out, actions, stats=True):
    """`out` (a result dict of k slabs) against the judge stepped on `actions` ([k][2][n] numpy)"""
    for t in range(actions.shape[0]):
        robs, rrew, rterm = ref.step(actions[t, 0], actions[t, 1])
        for i, a in enumerate((A1, A2)):
            assert out["obs"][a].dtype == raw.obs_dtype and out["rewards"][a].dtype == raw.reward_dtype
            assert np.array_equal(cpu(out["obs"][a][t]).view(np.int32), robs[i].view(np.int32)), (t, a)
            assert np.array_equal(cpu(out["rewards"][a][t]).view(np.int32), rrew[i].view(np.int32)), (t, a)
        assert np.array_equal(cpu(out["terminations"][t]).astype(np.uint8), rterm), t
    assert np.array_equal(cpu(out["actions"]), actions)
    assert np.array_equal(cpu(raw.read_state()), ref.state)
    if stats and raw.episode_returns is not None:
        assert np.array_equal(cpu(raw.episode_returns), ref.episode_returns)
        assert np.array_equal(cpu(raw.episode_lengths), ref.episode_lengths)


@pytest.mark.parametrize("stack", [False, True], ids=["bare", "stack"])
@pytest.mark.parametrize("fmt", ["int32", "packed"])
@pytest.mark.parametrize("skip", [1, 2, 4])
def test_the_python_methods_match_the_judge(oracle, skip, fmt, stack):
    """rollout_random_held and step_many_held in turn on one env (`out=` reused), steps_done counting policy steps, t0
    defaulting to it; then a plain step() continues the same trajectory."""
    n, k = 256, 24
    env, ref = make_env(oracle, n, skip, fmt=fmt, stack=stack)
    raw = env.unwrapped
    env.reset(), ref.reset()
    n_act = raw.n_actions
    out_r = out_m = None
    for rnd in range(3):
        t0 = raw.steps_done
        out_r = raw.rollout_random_held(5, k, out=out_r)
        assert raw.steps_done == t0 + k
        acts = np.stack([np.stack(oracle.random_actions(n, 0, 5, t0 + t, n_act)) for t in range(k)])
        judge_trajectory(oracle, raw, ref, out_r, acts)
        tape = np.stack([np.stack(oracle.random_actions(n, 0, 77, rnd * k + t, n_act)) for t in range(k)])
        again = raw.step_many_held(torch.as_tensor(tape, device="cuda:0"), out=out_m)
        assert out_m is None or again is out_m
        out_m = again
        assert raw.steps_done == t0 + 2 * k
        judge_trajectory(oracle, raw, ref, out_m, tape)
    a1, a2 = oracle.random_actions(n, 0, 9, 0, n_act)
    obs, rew, term, _, _ = env.step({A1: torch.as_tensor(a1, device="cuda:0"), A2: torch.as_tensor(a2, device="cuda:0")})
    robs, rrew, rterm = ref.step(a1, a2)
    assert np.array_equal(cpu(obs[A2]).view(np.int32), robs[1].view(np.int32))
    assert np.array_equal(cpu(rew[A1]).view(np.int32), rrew[0].view(np.int32))
    assert np.array_equal(cpu(raw.read_state()), ref.state)
    assert ref.ended_last > 0 and (skip == 1 or ref.ended_inside > 0)
    raw.check_actions()


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.int16])
def test_every_tape_dtype_and_an_out_of_range_element(oracle, dtype):
    n, k = 64, 8
    env, ref = make_env(oracle, n, 4, "hh", "none")
    env.reset(), ref.reset()
    tape = np.stack([np.stack(oracle.random_actions(n, 0, 3, t, 18)) for t in range(k)])
    out = env.step_many_held(torch.as_tensor(tape, device="cuda:0").to(dtype))
    judge_trajectory(oracle, env, ref, out, tape)
    env.check_actions()
    # lazy validation: counted by the launch, raised by a later poll; strict: raised by the call itself
    bad = torch.as_tensor(tape, device="cuda:0").to(dtype)
    bad[k - 1, 1, n - 1] = {torch.int64: 2 ** 32 + 3, torch.uint8: 200, torch.int16: -2}[dtype]
    env.step_many_held(bad)
    with pytest.raises(IndexError):
        env.check_actions()
    strict, _ = make_env(oracle, n, 4, "hh", "none", validate_every=1)
    strict.reset()
    with pytest.raises(IndexError):
        strict.step_many_held(bad)
    strict.step_many_held(torch.as_tensor(tape, device="cuda:0"))  # the counter was reset with the error


def test_refusals_and_argument_errors():
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd import wrappers as W

    env = pikazoo_v0.env(num_envs=8, device="cuda:0", frame_skip=2)
    env.reset()
    # the three existing methods keep refusing a frame-skip env
    with pytest.raises(ValueError, match="frame_skip=2"):
        env.step_random(1)
    with pytest.raises(ValueError, match="frame_skip=2"):
        env.rollout_random(1, 4)
    with pytest.raises(ValueError, match="frame_skip=2"):
        env.step_many(torch.zeros((4, 2, 8), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError, match="shape"):
        env.step_many_held(torch.zeros((4, 8), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(TypeError):
        env.step_many_held(torch.zeros((4, 2, 8), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError, match="k must be"):
        env.rollout_random_held(1, 0)
    odd = pikazoo_v0.env(num_envs=6, device="cuda:0", frame_skip=2)
    odd.reset()
    with pytest.raises(ValueError, match="multiple of 4"):
        odd.rollout_random_held(1, 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        odd.step_many_held(torch.zeros((4, 2, 6), dtype=torch.int32, device="cuda:0"))
    odd.rollout_random_held(1, 1)  # a single slab needs no alignment
    # a stack with a wrapper outside the kernel is refused as the siblings refuse it
    unfused = W.SimplifyAction(W.SimplifyAction(pikazoo_v0.env(num_envs=8, device="cuda:0", frame_skip=2)))
    unfused.reset()
    for call in (lambda: unfused.unwrapped.rollout_random_held(1, 4),
                 lambda: unfused.unwrapped.step_many_held(torch.zeros((4, 2, 8), dtype=torch.int32, device="cuda:0"))):
        with pytest.raises(RuntimeError, match="outside the kernel"):
            call()


def test_a_checkpoint_after_a_held_trajectory_continues_identically(oracle):
    n, k = 256, 16
    env, ref = make_env(oracle, n, 4, stack=True)
    env.reset(), ref.reset()
    env.unwrapped.rollout_random_held(5, k)
    sd = env.unwrapped.state_dict()
    assert sd["steps_done"] == k and sd["config"]["frame_skip"] == 4
    same, _ = make_env(oracle, n, 4, fmt="packed", stack=True)
    same.reset()
    same.unwrapped.load_state_dict(sd)
    assert same.unwrapped.steps_done == k
    o1, o2 = env.unwrapped.rollout_random_held(5, k), same.unwrapped.rollout_random_held(5, k)
    acts = np.stack([np.stack(oracle.random_actions(n, 0, 5, t, 13)) for t in range(2 * k)])
    for t in range(k):
        ref.step(acts[t, 0], acts[t, 1])
    judge_trajectory(oracle, same.unwrapped, ref, o2, acts[k:])
    for key in ("actions", "terminations"):
        assert torch.equal(o1[key], o2[key])
    for a in (A1, A2):
        assert torch.equal(o1["obs"][a], o2["obs"][a]) and torch.equal(o1["rewards"][a], o2["rewards"][a])
    assert torch.equal(env.unwrapped.read_state(), same.unwrapped.read_state())


def test_hipgraph_replay_equals_eager(oracle):
    n, k = 256, 16
    tape = torch.as_tensor(np.stack([np.stack(oracle.random_actions(n, 0, 3, t, 18)) for t in range(k)]), device="cuda:0")
    results = {}
    for mode in ("eager", "graph"):
        env, ref = make_env(oracle, n, 4, validate_actions=False)
        env.reset(), ref.reset()
        out = env.step_many_held(tape)  # (allocates the outputs; a capture records launches only, it runs nothing)
        if mode == "graph":
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                env.step_many_held(tape, out=out)
                roll = env.rollout_random_held(5, k, t0=k)
            g.replay()
            torch.cuda.synchronize()
        else:
            env.step_many_held(tape, out=out)
            roll = env.rollout_random_held(5, k, t0=k)
        results[mode] = (out["obs"][A1].clone(), out["rewards"][A2].clone(), roll["obs"][A2].clone(),
                         roll["actions"].clone(), roll["terminations"].clone(), env.read_state().clone())
        if mode == "eager":  # and eager is the judge's
            for t in range(2 * k):
                ref.step(*(cpu(tape[t % k])))
            rolled = np.stack([np.stack(oracle.random_actions(n, 0, 5, k + t, 18)) for t in range(k)])
            assert np.array_equal(results[mode][3].cpu().numpy(), rolled)
            for t in range(k):
                robs, _, rterm = ref.step(rolled[t, 0], rolled[t, 1])
                assert np.array_equal(cpu(roll["obs"][A2][t]), robs[1]) and np.array_equal(
                    cpu(roll["terminations"][t]).astype(np.uint8), rterm)
            assert np.array_equal(cpu(env.read_state()), ref.state)
    for e, g in zip(results["eager"], results["graph"]):
        assert torch.equal(e, g)
