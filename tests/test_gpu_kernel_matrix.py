"""Every step-kernel instantiation of the product library, launched and checked against the oracle.

One test per row of tests/kernel_matrix.py (its id: the instantiation's name, and the table mode where the kernel runs
under both).  Each row goes straight through the C ABI -- the config, the tables pointer and the statistics pointer are
exactly the row's -- from random valid states with a winning score of 3 (scores of 0-2 planted, an eighth of the games
planted over): scoring, the terminal frame and the in-place auto-reset all happen inside the launch.  Compared with
the oracle: every frame's observations (int16 rows widened), rewards and terminations, the actions pz_rollout_random
writes, the final state (unpacked for the packed format) and the episode statistics; and nothing past lane n of the
state or of any output is written.  Below the switch every lane; at/above it the first, a middle and the last 512 lanes.
The launch runs under torch.profiler, and the one `pz::` kernel it records must be the row's instantiation.  The
fused rows' float outputs are also judged in float64 (check_config).

check_config() is that check for any kernel_configs.Config; tests/test_gpu_kernel_configs.py runs it on the other
runtime configurations of every instantiation.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from kernel_configs import ACTION_FORMATS, NORMAL_STATE_REWARD, NORMALIZED, SHAPING, plant_states
from kernel_matrix import ROWS, STRIDE_PAD
from test_gpu_parity import cpu

pytestmark = pytest.mark.gpu

SLICE = 512
KMAX = max(r.k for r in ROWS)
WORDS, OBS = 44, 35
SENT = -7  # what the output buffers hold before a launch


def _slots(c):
    """(launches, output frames per launch): the single-frame entry points run a few launches, each into its own slot"""
    if c.entry in ("pz_rollout_random", "pz_step_many"):
        return 1, c.k
    return (3 if c.k == 1 else 2), 1


class _Buffers:
    """Device buffers of one batch size, reused across the rows: the 70-frame tape at 393 224 games is 7.7 GB of
    observations.  Every buffer holds STRIDE_PAD lanes (or rows) more than a launch may write."""

    def __init__(self, n, dev):
        stride, frames = n + STRIDE_PAD, max(KMAX, 3)
        self.state = torch.empty(WORDS * stride, dtype=torch.int32, device=dev)  # [WORDS][launch stride], then spare
        self.packed = torch.empty(36 * stride, dtype=torch.uint8, device=dev)
        self.stats = torch.empty(20 * stride, dtype=torch.uint8, device=dev)
        self.obs = [torch.empty(frames * n * OBS + STRIDE_PAD * OBS, dtype=torch.int32, device=dev) for _ in range(2)]
        self.rew = [torch.empty(frames * n + STRIDE_PAD, dtype=torch.int32, device=dev) for _ in range(2)]
        self.term = torch.empty(frames * n + STRIDE_PAD, dtype=torch.uint8, device=dev)
        self.act = torch.empty(frames * 2 * n + STRIDE_PAD, dtype=torch.int32, device=dev)
        self.tape = torch.empty((frames, 2, n), dtype=torch.int32, device=dev)


@pytest.fixture(scope="module")
def buffers():
    made = {}

    def get(n):
        if n not in made:
            made.clear()
            torch.cuda.empty_cache()
            made[n] = _Buffers(n, torch.device("cuda:0"))
        return made[n]

    yield get
    made.clear()
    torch.cuda.empty_cache()


def _kernel_name(raw):
    """kernel_digest's form: no `void `, no `pz::`, no argument list"""
    return raw.replace("void ", "").split("(")[0].replace("pz::", "")


def _rows_as(ref_obs, fmt):
    """The bit-exact judge of one frame's rows: the oracle's rows -- int32, or the float32 NormalizeObservation quotient
    of the normalized formats -- in format `fmt`, as the values / bit patterns the buffer holds (2-byte rows widened)"""
    if fmt == 1:
        return ref_obs.view(np.int32)
    if fmt in (0, 2):
        return ref_obs
    dt = torch.float16 if fmt in (3, 5) else torch.bfloat16
    return torch.from_numpy(np.ascontiguousarray(ref_obs)).to(torch.float32).to(dt).view(torch.int16).numpy().astype(
        np.int32)


def _wrapper_stack(c):
    """The fused wrappers of `c` as the reference would stack them (innermost first), for oracle.wrappers_oracle"""
    table, x_line, y_line = SHAPING[c.shaping] or (None, 216, 176)
    stack = [("SimplifyAction", {})] if c.simplify_action else []
    if c.stats_mode == 1:
        stack.append(("RecordEpisodeStatistics", {}))
    if c.normal_state_mode == 1:
        stack.append(("RewardInNormalState", {"reward": NORMAL_STATE_REWARD}))
    if table is not None:
        stack.append(("RewardByBallPosition", dict(additional_reward=table, x_line=x_line, y_line=y_line)))
    if c.normal_state_mode == 2:
        stack.append(("RewardInNormalState", {"reward": NORMAL_STATE_REWARD}))
    if c.stats_mode == 2:
        stack.append(("RecordEpisodeStatistics", {}))
    if c.obs_format in NORMALIZED:
        stack.append(("NormalizeObservation", {}))
    return stack


def check_config(c, oracle, buffers):
    """Launch configuration `c` (a kernel_configs.Config; a matrix row: Row.config()) through the C ABI and compare it
    with the oracle.  The launch starts from random valid states with an eighth of the games planted over (a winner at
    the winning score) and, but on the matrix rows, scores drawn below the winning score with a quarter of the games
    one point from the end.  Checked: the dispatched kernel by name (torch.profiler); nothing past lane n of the state,
    the outputs or the statistics written; every frame's rows, rewards and terminations, pz_rollout_random's actions,
    the final state and the statistics bit for bit against the oracle (every lane below the switch, three slices of
    512 above it).  With auto_reset on, the float outputs of a fused configuration are also judged in float64 against
    oracle/wrappers_oracle.WrappedOracle: normalized rows bit for bit (the float32 rounding of the float64 quotient,
    rounded again to nearest even for the 2-byte formats), rewards within 1e-6, episode returns within 2e-6.  A
    configuration with reward shaping must have put some post-step ball exactly on one of its lines."""
    from oracle.wrappers_oracle import WrappedOracle
    from pikazoo_amd import _native
    from pikazoo_amd.env import flight_tables

    lib = _native.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, stride, k, fmt = c.n, c.stride, c.k, c.obs_format
    launches, frames = _slots(c)
    slots = launches * frames
    b = buffers(n)
    base, aseed, t0, ws = c.env_id_base, c.seed ^ 0x5EED, c.t0, c.winning_score
    n_act = 13 if c.simplify_action else 18

    # random valid states, scores below the winning score, an eighth of the games over: reset in place before their first
    # frame, or frozen without auto_reset (kernel_configs.plant_states, shared with the frame-skip configurations)
    planted, over = plant_states(c)
    frozen = over & (c.auto_reset == 0)
    okw = c.oracle_kwargs()
    cfg = _native.PzConfig.from_buffer_copy(oracle.make_config(env_id_base=base, **okw))
    cfg.packed_state = int(c.packed)
    cfg.normalize_obs = fmt
    cfg.action_format = ACTION_FORMATS[c.action_format]
    tables = {"both": lambda: flight_tables(dev)[0], "power_hit": lambda: flight_tables(dev, landing=False)[0],
              "none": lambda: None}[c.tables]()
    tb = None if tables is None else C.byref(tables)

    # the starting state, the outputs' sentinels, the actions of the launches that read them
    b.state.fill_(-99)
    state = b.state[:WORDS * stride].view(WORDS, stride)
    state[:, :n] = torch.from_numpy(planted).to(dev)
    if c.packed:
        b.packed.fill_(0xA5)
        misfits = torch.zeros(1, dtype=torch.int64, device=dev)
        assert lib.pz_pack_state(state.data_ptr(), n, stride, b.packed.data_ptr(), stride, misfits.data_ptr(),
                                 stream) == 0
        torch.cuda.synchronize()
        assert int(misfits.item()) == 0
    state_ptr = b.packed.data_ptr() if c.packed else state.data_ptr()
    b.stats.zero_()
    sp = b.stats.data_ptr() if c.stats_ptr else None
    odt = torch.int16 if fmt >= 2 else torch.int32
    obs = [o.view(odt)[:(slots * n + STRIDE_PAD) * OBS] for o in b.obs]
    for o in obs:
        o.fill_(SENT)
    for r in b.rew:
        r.fill_(SENT)
    b.term.fill_(9)
    b.act.fill_(SENT)
    acts = []
    if c.entry in ("pz_step", "pz_step_many"):
        for f in range(slots):
            assert lib.pz_random_actions(b.tape[f, 0].data_ptr(), b.tape[f, 1].data_ptr(), n, base, aseed, t0 + f,
                                         n_act, stream) == 0
        adt = {"i32": torch.int32, "i64": torch.int64, "u8": torch.uint8, "i16": torch.int16}[c.action_format]
        acts = [(b.tape[f, 0].to(adt), b.tape[f, 1].to(adt)) for f in range(slots)] if c.entry == "pz_step" else []
    torch.cuda.synchronize()

    def out(buf, slot, width=1):
        return buf[slot * n * width:(slot + 1) * n * width].data_ptr()

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(launches):
            o = (out(obs[0], i, OBS), out(obs[1], i, OBS), out(b.rew[0], i), out(b.rew[1], i), out(b.term, i))
            if c.entry == "pz_step":
                err = lib.pz_step(state_ptr, n, stride, C.byref(cfg), acts[i][0].data_ptr(), acts[i][1].data_ptr(),
                                  *o, sp, tb, stream)
            elif c.entry == "pz_step_random":
                err = lib.pz_step_random(state_ptr, n, stride, C.byref(cfg), aseed, t0 + i * k, k, *o, sp, None, tb,
                                         stream)
            elif c.entry == "pz_rollout_random":
                err = lib.pz_rollout_random(state_ptr, n, stride, C.byref(cfg), aseed, t0, k, b.act.data_ptr(), *o, sp,
                                            None, tb, stream)
            else:
                err = lib.pz_step_many(state_ptr, n, stride, C.byref(cfg), b.tape.data_ptr(), k, *o, sp, None, tb,
                                       stream)
            assert err == 0, (c.name, err)
        torch.cuda.synchronize()
    device_events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert device_events, "torch.profiler recorded no device kernel: the dispatched-kernel check cannot run"
    dispatched = [_kernel_name(e.name) for e in device_events if "pz::" in e.name]
    assert dispatched == [c.kernel] * launches, (c.name, sorted({e.name for e in device_events}))

    # nothing past lane n (past the last written row) of the state or of an output
    if c.packed:
        p = b.packed
        assert all(bool((part == 0xA5).all()) for part in (p[16 * n:16 * stride], p[16 * stride + 16 * n:32 * stride],
                                                         p[32 * stride + 4 * n:])), "packed state past lane n"
        flagged = torch.zeros(1, dtype=torch.int64, device=dev)
        b.state.fill_(-99)
        assert lib.pz_unpack_state(b.packed.data_ptr(), n, stride, state.data_ptr(), stride, flagged.data_ptr(),
                                   stream) == 0
        torch.cuda.synchronize()
        assert int(flagged.item()) == 0
    assert bool((state[:, n:] == -99).all()) and bool((b.state[WORDS * stride:] == -99).all()), "state past lane n"
    for o in obs:
        assert bool((o[slots * n * OBS:] == SENT).all()), "observation rows past the last frame's lane n"
    for r in b.rew:
        assert bool((r[slots * n:] == SENT).all()), "rewards past the last frame's lane n"
    assert bool((b.term[slots * n:] == 9).all()), "terminations past the last frame's lane n"
    written_act = k * 2 * n if c.entry == "pz_rollout_random" else 0
    assert bool((b.act[written_act:] == SENT).all()), "actions past the last frame's lane n"
    ret = b.stats[:16 * stride].view(torch.float64).view(2, stride)
    lengths = b.stats[16 * stride:].view(torch.int32)
    if c.stats_ptr:
        assert bool((ret[:, n:] == 0).all()) and bool((lengths[n:] == 0).all()), "statistics past lane n"
    else:
        assert bool((b.stats == 0).all()), "statistics written without a statistics pointer"

    # the oracle on every lane below the switch, on three slices of 512 above it
    table, x_line, y_line = SHAPING[c.shaping] or (None, None, None)
    float_rewards = table is not None or c.normal_state_mode != 0
    judge64 = c.auto_reset and (float_rewards or fmt in NORMALIZED or c.stats_ptr)
    on_line = nsr_after_cancel = False
    spans = [(0, n)] if not c.above else [(0, SLICE), (n // 2 - 300, n // 2 - 300 + SLICE), (n - SLICE, n)]
    for lo, hi in spans:
        m = hi - lo
        ref = oracle.OracleEnv(m, oracle.make_config(env_id_base=base + lo, **okw), nthreads=8)
        ref.state[:] = planted[:, lo:hi]
        wo = None
        if judge64:
            wo = WrappedOracle(m, _wrapper_stack(c), winning_score=ws, serve=c.serve, is_player1_computer=c.p1,
                               is_player2_computer=c.p2, seed=c.seed, env_id_base=base + lo)
            wo.plant(planted[:, lo:hi])
        live = ~frozen[lo:hi]
        h_obs = [cpu(o[:slots * n * OBS].view(slots, n, OBS)[:, lo:hi]).astype(np.int32) for o in obs]
        h_rew = [cpu(r[:slots * n].view(slots, n)[:, lo:hi]) for r in b.rew]
        h_term = cpu(b.term[:slots * n].view(slots, n)[:, lo:hi])
        h_act = cpu(b.act[:k * 2 * n].view(k, 2, n)[:, :, lo:hi]) if c.entry == "pz_rollout_random" else None
        tape = cpu(b.tape[:slots, :, lo:hi])
        for s in range(slots):
            if c.entry == "pz_step_random":
                ref.rollout_random(aseed, t0 + s * k, k)
                for j in range(k if wo else 0):
                    wout = wo.step(*oracle.random_actions(m, base + lo, aseed, t0 + s * k + j, n_act))
            elif c.entry == "pz_rollout_random":
                a1, a2 = oracle.random_actions(m, base + lo, aseed, t0 + s, n_act)
                assert np.array_equal(h_act[s, 0], a1) and np.array_equal(h_act[s, 1], a2), (c.name, lo, s, "actions")
                ref.step(a1, a2)
                wout = wo.step(a1, a2) if wo else None
            else:
                ref.step(tape[s, 0], tape[s, 1])
                wout = wo.step(tape[s, 0], tape[s, 1]) if wo else None
            ctx = (c.name, lo, s)
            for p in range(2):
                assert np.array_equal(h_obs[p][s], _rows_as(ref.obs[p], fmt)), (*ctx, f"observations of player {p + 1}")
                assert np.array_equal(h_rew[p][s], ref.rew[p].view(np.int32)), (*ctx, f"rewards of player {p + 1}")
            assert np.array_equal(h_term[s], ref.term), (*ctx, "terminations")
            if table is not None:  # the post-step ball the zone was taken from
                bx, by = ref.state[oracle.B_X], ref.state[oracle.B_Y]
                on_line |= bool((live & ((bx == x_line) | (by == y_line))).any())
                if c.shaping == "cancel" and c.normal_state_mode == 2:  # a point cancelled to 0, then replaced
                    nsr = np.float32(NORMAL_STATE_REWARD)
                    nsr_after_cancel |= bool((live & (by == 252) & (h_rew[0][s].view(np.float32) == nsr) &
                                              (h_rew[1][s].view(np.float32) == nsr)).any())
            if wo:  # the float64 judge
                w_obs, w_rew, w_term, _ = wout
                assert np.array_equal(h_term[s], w_term), (*ctx, "terminations (float64 judge)")
                for p in range(2):
                    if fmt in NORMALIZED:
                        assert np.array_equal(h_obs[p][s], _rows_as(w_obs[p].astype(np.float32), fmt)), \
                            (*ctx, f"normalized rows of player {p + 1} vs float64")
                    if float_rewards:
                        err = np.abs(h_rew[p][s].view(np.float32).astype(np.float64) - w_rew[p]).max()
                        assert err <= 1e-6, (*ctx, f"rewards of player {p + 1} vs float64: {err}")
        got = cpu(state[:, lo:hi])
        if not np.array_equal(got, ref.state):
            f, l = np.argwhere(got != ref.state)[0]
            pytest.fail(f"{c.name}: lane {lo + l} word {oracle.FIELD_NAMES[f]}: hip {got[f, l]} != oracle "
                        f"{ref.state[f, l]}")
        if c.stats_ptr:
            assert np.array_equal(cpu(ret[:, lo:hi]), ref.episode_returns), (c.name, lo, "episode returns")
            assert np.array_equal(cpu(lengths[lo:hi]), ref.episode_lengths), (c.name, lo, "episode lengths")
            if wo:
                err = np.abs(cpu(ret[:, lo:hi]) - wo.episode_returns).max()
                assert err <= 2e-6, (c.name, lo, f"episode returns vs float64: {err}")
                assert np.array_equal(cpu(lengths[lo:hi]), wo.episode_lengths), (c.name, lo, "lengths (float64 judge)")
    assert bool(cpu(b.term[:slots * n]).any()), "no game ended inside the launch"
    if table is not None:
        assert on_line, f"{c.name}: no post-step ball on x_line {x_line} or y_line {y_line}"
    if c.shaping == "cancel" and c.normal_state_mode == 2:
        assert nsr_after_cancel, f"{c.name}: no point cancelled by the table and replaced by RewardInNormalState"


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_kernel_matrix_row_vs_oracle(row, oracle, buffers):
    check_config(row.config(), oracle, buffers)
