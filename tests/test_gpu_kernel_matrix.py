"""Every step-kernel instantiation of the product library, launched and checked against the oracle.

One test per row of tests/kernel_matrix.py (its id: the instantiation's name, and the table mode where the kernel runs
under both).  Each row goes straight through the C ABI -- the config, the tables pointer and the statistics pointer are
exactly the row's -- from random valid states with a winning score of 3 (scores of 0-2 planted, an eighth of the games
planted over): scoring, the terminal frame and the in-place auto-reset all happen inside the launch.  Compared with
the oracle: every frame's observations (int16 rows widened), rewards and terminations, the actions pz_rollout_random
writes, the final state (unpacked for the packed format) and the episode statistics; and nothing past lane n of the
state or of any output is written.  Below the switch every lane; at/above it the first, a middle and the last 512 lanes.
The launch runs under torch.profiler, and the one `pz::` kernel it records must be the row's instantiation.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from kernel_matrix import ROWS, STRIDE_PAD
from test_gpu_packed import _random_valid_states
from test_gpu_parity import cpu

pytestmark = pytest.mark.gpu

TABLE = (0.0, -0.01, 0.25, 0.01, -0.5, 0.01, 0.0, -0.01)  # RewardByBallPosition of the fused rows
SLICE = 512
KMAX = max(r.k for r in ROWS)
WORDS, OBS = 44, 35
SENT = -7  # what the output buffers hold before a launch


def _slots(row):
    """(launches, output frames per launch): the single-frame entry points run a few launches, each into its own slot"""
    if row.entry in ("pz_rollout_random", "pz_step_many"):
        return 1, row.k
    return (3 if row.k == 1 else 2), 1


class _Buffers:
    """Device buffers of one batch size, reused across the rows: the 70-frame tape at 393 224 games is 7.7 GB of
    observations.  Every buffer holds STRIDE_PAD lanes (or rows) more than a launch may write."""

    def __init__(self, n, dev):
        stride, frames = n + STRIDE_PAD, max(KMAX, 3)
        self.state = torch.empty((WORDS, stride), dtype=torch.int32, device=dev)
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


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_kernel_matrix_row_vs_oracle(row, oracle, buffers):
    from pikazoo_amd import _native
    from pikazoo_amd.env import flight_tables

    lib = _native.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, stride, k = row.n, row.stride, row.k
    launches, frames = _slots(row)
    slots = launches * frames
    b = buffers(n)
    seed = zlib.crc32(row.id.encode())
    rng = np.random.default_rng(seed)
    base, aseed, t0 = 1 << 20, seed ^ 0x5EED, 1000
    fused = not row.plain
    n_act = 13 if fused else 18

    planted = _random_valid_states(n, rng)
    # an eighth of the games over (a winner at the winning score; game_ended implies round_ended): reset in place
    # before their first frame
    over = rng.random(n) < 0.125
    winner = np.where(rng.random(n) < 0.5, 38, 39)
    planted[winner[over], np.flatnonzero(over)] = 3
    planted[41][over] = planted[42][over] = 1
    okw = dict(winning_score=3, serve="random" if fused else "winner", is_player1_computer=row.p1,
               is_player2_computer=row.p2, seed=seed, simplify_action=fused, additional_reward=TABLE if fused else None,
               normalize_obs=fused and not row.obs16 and row.p1 == row.p2, episode_stats=1 if fused else 0)
    cfg = _native.PzConfig.from_buffer_copy(oracle.make_config(env_id_base=base, **okw))
    cfg.packed_state = int(row.packed)
    if row.obs16:
        cfg.normalize_obs = 2
    tables = {"both": lambda: flight_tables(dev)[0], "power_hit": lambda: flight_tables(dev, landing=False)[0],
              "none": lambda: None}[row.tables]()
    tb = None if tables is None else C.byref(tables)

    # the starting state, the outputs' sentinels, the actions of the launches that read them
    b.state.fill_(-99)
    b.state[:, :n] = torch.from_numpy(planted).to(dev)
    if row.packed:
        b.packed.fill_(0xA5)
        misfits = torch.zeros(1, dtype=torch.int64, device=dev)
        assert lib.pz_pack_state(b.state.data_ptr(), n, stride, b.packed.data_ptr(), stride, misfits.data_ptr(),
                                 stream) == 0
        torch.cuda.synchronize()
        assert int(misfits.item()) == 0
    state_ptr = b.packed.data_ptr() if row.packed else b.state.data_ptr()
    b.stats.zero_()
    sp = b.stats.data_ptr() if fused else None
    odt = torch.int16 if row.obs16 else torch.int32
    obs = [o.view(odt)[:(slots * n + STRIDE_PAD) * OBS] for o in b.obs]
    for o in obs:
        o.fill_(SENT)
    for r in b.rew:
        r.fill_(SENT)
    b.term.fill_(9)
    b.act.fill_(SENT)
    if row.entry in ("pz_step", "pz_step_many"):
        for f in range(slots):
            assert lib.pz_random_actions(b.tape[f, 0].data_ptr(), b.tape[f, 1].data_ptr(), n, base, aseed, t0 + f,
                                         n_act, stream) == 0
    torch.cuda.synchronize()

    def out(buf, slot, width=1):
        return buf[slot * n * width:(slot + 1) * n * width].data_ptr()

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(launches):
            o = (out(obs[0], i, OBS), out(obs[1], i, OBS), out(b.rew[0], i), out(b.rew[1], i), out(b.term, i))
            if row.entry == "pz_step":
                err = lib.pz_step(state_ptr, n, stride, C.byref(cfg), b.tape[i, 0].data_ptr(), b.tape[i, 1].data_ptr(),
                                  *o, sp, tb, stream)
            elif row.entry == "pz_step_random":
                err = lib.pz_step_random(state_ptr, n, stride, C.byref(cfg), aseed, t0 + i * k, k, *o, sp, None, tb,
                                         stream)
            elif row.entry == "pz_rollout_random":
                err = lib.pz_rollout_random(state_ptr, n, stride, C.byref(cfg), aseed, t0, k, b.act.data_ptr(), *o, sp,
                                            None, tb, stream)
            else:
                err = lib.pz_step_many(state_ptr, n, stride, C.byref(cfg), b.tape.data_ptr(), k, *o, sp, None, tb,
                                       stream)
            assert err == 0, (row.id, err)
        torch.cuda.synchronize()
    device_events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert device_events, "torch.profiler recorded no device kernel: the dispatched-kernel check cannot run"
    dispatched = [_kernel_name(e.name) for e in device_events if "pz::" in e.name]
    assert dispatched == [row.kernel] * launches, (row.id, sorted({e.name for e in device_events}))

    # nothing past lane n (past the last written row) of the state or of an output
    if row.packed:
        p = b.packed
        assert all(bool((part == 0xA5).all()) for part in (p[16 * n:16 * stride], p[16 * stride + 16 * n:32 * stride],
                                                         p[32 * stride + 4 * n:])), "packed state past lane n"
        flagged = torch.zeros(1, dtype=torch.int64, device=dev)
        b.state.fill_(-99)
        assert lib.pz_unpack_state(b.packed.data_ptr(), n, stride, b.state.data_ptr(), stride, flagged.data_ptr(),
                                   stream) == 0
        torch.cuda.synchronize()
        assert int(flagged.item()) == 0
    assert bool((b.state[:, n:] == -99).all()), "state past lane n"
    for o in obs:
        assert bool((o[slots * n * OBS:] == SENT).all()), "observation rows past the last frame's lane n"
    for r in b.rew:
        assert bool((r[slots * n:] == SENT).all()), "rewards past the last frame's lane n"
    assert bool((b.term[slots * n:] == 9).all()), "terminations past the last frame's lane n"
    written_act = k * 2 * n if row.entry == "pz_rollout_random" else 0
    assert bool((b.act[written_act:] == SENT).all()), "actions past the last frame's lane n"
    ret = b.stats[:16 * stride].view(torch.float64).view(2, stride)
    lengths = b.stats[16 * stride:].view(torch.int32)
    assert bool((ret[:, n:] == 0).all()) and bool((lengths[n:] == 0).all()), "statistics past lane n"

    # the oracle on every lane below the switch, on three slices of 512 above it
    spans = [(0, n)] if not row.above else [(0, SLICE), (n // 2 - 300, n // 2 - 300 + SLICE), (n - SLICE, n)]
    for lo, hi in spans:
        m = hi - lo
        ref = oracle.OracleEnv(m, oracle.make_config(env_id_base=base + lo, **okw), nthreads=8)
        ref.state[:] = planted[:, lo:hi]
        h_obs = [cpu(o[:slots * n * OBS].view(slots, n, OBS)[:, lo:hi]).astype(np.int32) for o in obs]
        h_rew = [cpu(r[:slots * n].view(slots, n)[:, lo:hi]) for r in b.rew]
        h_term = cpu(b.term[:slots * n].view(slots, n)[:, lo:hi])
        h_act = cpu(b.act[:k * 2 * n].view(k, 2, n)[:, :, lo:hi]) if row.entry == "pz_rollout_random" else None
        tape = cpu(b.tape[:slots, :, lo:hi])
        for s in range(slots):
            if row.entry == "pz_step_random":
                ref.rollout_random(aseed, t0 + s * k, k)
            elif row.entry == "pz_rollout_random":
                a1, a2 = oracle.random_actions(m, base + lo, aseed, t0 + s, n_act)
                assert np.array_equal(h_act[s, 0], a1) and np.array_equal(h_act[s, 1], a2), (row.id, lo, s, "actions")
                ref.step(a1, a2)
            else:
                ref.step(tape[s, 0], tape[s, 1])
            ctx = (row.id, lo, s)
            for p in range(2):
                want = ref.obs[p] if row.obs16 else ref.obs[p].view(np.int32)
                assert np.array_equal(h_obs[p][s], want), (*ctx, f"observations of player {p + 1}")
                assert np.array_equal(h_rew[p][s], ref.rew[p].view(np.int32)), (*ctx, f"rewards of player {p + 1}")
            assert np.array_equal(h_term[s], ref.term), (*ctx, "terminations")
        got = cpu(b.state[:, lo:hi])
        if not np.array_equal(got, ref.state):
            f, l = np.argwhere(got != ref.state)[0]
            pytest.fail(f"{row.id}: lane {lo + l} word {oracle.FIELD_NAMES[f]}: hip {got[f, l]} != oracle "
                        f"{ref.state[f, l]}")
        if fused:
            assert np.array_equal(cpu(ret[:, lo:hi]), ref.episode_returns), (row.id, lo, "episode returns")
            assert np.array_equal(cpu(lengths[lo:hi]), ref.episode_lengths), (row.id, lo, "episode lengths")
    assert bool(cpu(b.term[:slots * n]).any()), "no game ended inside the launch"
