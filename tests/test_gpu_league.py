"""GPU tests (``-m gpu``) of the league library (include/pikazoo_league.h: ``pz_league_tally``, ``pz_league_draw``) and of
``pikazoo_amd.league``.

The judge is tests/league_judge.py: the header's draw and tally in numpy / Python integers (tests/test_league_host.py holds it
to a scalar formulation and to eleven mutants on exactly the cases used here).  Both launches are integer arithmetic, so every
comparison is for EQUALITY: member vectors word for word, tables and error counts cell for cell.  No GPU result is ever an
expected value.  Every C-ABI launch writes into sentinel-filled buffers with words in front of the first element and behind
the last one, which must keep the sentinel; member vectors hold a planted value that every game which is not drawn must keep.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import league_judge as LJ
import pool_judge as PJ
from test_gpu_policy import SENT, TAIL, cpu, stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRONT = 3   # sentinel elements in front of every output buffer
TORCH = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64, "int16": torch.int16}
A1, A2 = "player_1", "player_2"


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import league

    return league.load()


def guarded(values, dtype):
    """a device buffer holding `values` between FRONT and TAIL sentinel elements: (tensor, address of element 0)"""
    values = np.asarray(values).astype(dtype).reshape(-1)
    sent = np.array(SENT).astype(dtype)                # (uint8: 249)
    host = np.concatenate([np.full(FRONT, sent, dtype), values, np.full(TAIL, sent, dtype)])
    t = torch.from_numpy(host).to(DEV)
    return t, t.data_ptr() + FRONT * t.element_size()


def read_guarded(t, count):
    flat = cpu(t)
    sent = np.array(SENT).astype(flat.dtype)
    assert (flat[:FRONT] == sent).all() and (flat[FRONT + count:] == sent).all(), "a buffer was written outside its elements"
    return flat[FRONT:FRONT + count]


def on_device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- the draw -----------------------------------------------------------------------------------------------------------------
def run_draw(lib, case):
    """pz_league_draw of a judge case through the C ABI: (members as int64, errors)"""
    n, P, dtype = case["n"], case["P"], case["dtype"]
    weights = LJ.make_weights(case["weights"], P)
    mask = LJ.make_mask(case["mask"], n)
    by_value, device_part = LJ.split_counter(case["counter"], case["C"])
    d_weights, d_mask = on_device(weights), on_device(mask)
    d_counter = on_device(np.array([device_part], np.int64)) if device_part is not None else None
    members = guarded(np.full(n, LJ.PLANTED), dtype)
    errors = guarded([0], "int32")
    code = lib.pz_league_draw(ptr(d_weights), P, case["seed"], by_value, ptr(d_counter), case["first_game"], ptr(d_mask), members[1],
                              LJ.MEMBER_DTYPES.index(dtype), n, errors[1], stream())
    assert code == 0, (code, case)
    torch.cuda.synchronize()
    return read_guarded(members[0], n).astype(np.int64), int(read_guarded(errors[0], 1)[0])


@pytest.mark.parametrize("n", LJ.CASE_N)
def test_draw_equals_the_judge_word_for_word(lib, n):
    """P in {1, 2, 3, 16} x every weight kind (small, with zeros, one and all at 2^32 - 1) x every mask, the three formats,
    first_game beyond 2^32, the counter by value, on the device and both; then a negative weight, 2^32 and all-zero weights:
    errors == 1 and every member untouched"""
    for P in LJ.CASE_P:
        for case in LJ.draw_cases(n, P):
            weights, mask = LJ.make_weights(case["weights"], P), LJ.make_mask(case["mask"], n)
            want, want_errors = LJ.draw(weights, n, case["seed"], case["C"], case["first_game"], mask)
            got, errors = run_draw(lib, case)
            assert errors == want_errors, case
            assert np.array_equal(got, want), (case, np.flatnonzero(got != want)[:8])
            if case["weights"] in LJ.BAD_WEIGHT_KINDS:
                assert errors == 1 and (got == LJ.PLANTED).all(), case


def test_draw_errors_is_never_cleared_and_a_shard_draws_the_batchs_tail(lib):
    n, P = 4099, 3
    case = dict(LJ.draw_cases(n, P)[0], mask="absent", dtype="int32", first_game=(1 << 32) - 1000)
    weights = on_device(LJ.make_weights(case["weights"], P))
    errors = guarded([1], "int32")                                             # an earlier failure stays visible
    whole, tail = guarded(np.full(n, LJ.PLANTED), "int32"), guarded(np.full(n - 1000, LJ.PLANTED), "int32")
    assert lib.pz_league_draw(weights.data_ptr(), P, case["seed"], 4, None, case["first_game"], None, whole[1], 1, n, errors[1], stream()) == 0
    assert lib.pz_league_draw(weights.data_ptr(), P, case["seed"], 4, None, case["first_game"] + 1000, None, tail[1], 1, n - 1000, errors[1], stream()) == 0
    torch.cuda.synchronize()
    want, _ = LJ.draw(LJ.make_weights(case["weights"], P), n, case["seed"], 4, case["first_game"])
    assert np.array_equal(read_guarded(whole[0], n), want) and np.array_equal(read_guarded(tail[0], n - 1000), want[1000:])
    assert read_guarded(errors[0], 1)[0] == 1


# ---- the tally ----------------------------------------------------------------------------------------------------------------
def run_tally(lib, case, x, table=None, errors=None):
    """pz_league_tally of a judge case through the C ABI, into the given guarded buffers or fresh ones holding the case's
    preloaded table and errors: (table int64 [P, P, 4], errors, the two guarded buffers)"""
    n, P = case["n"], case["P"]
    table = guarded(x["table"], "int64") if table is None else table
    errors = guarded([x["errors"]], "int64") if errors is None else errors
    d = {k: on_device(x[k]) for k in ("terminated", "buf1", "buf2", "members_p1", "members_p2")}
    code = lib.pz_league_tally(ptr(d["terminated"]), ptr(d["buf1"]), ptr(d["buf2"]), LJ.SCORE_DTYPES.index(case["score_dtype"]), case["stride"],
                               ptr(d["members_p1"]), ptr(d["members_p2"]), LJ.MEMBER_DTYPES.index(case["member_dtype"]), n, P, table[1], errors[1],
                               stream())
    assert code == 0, (code, case)
    torch.cuda.synchronize()
    return read_guarded(table[0], P * P * LJ.CELL).reshape(P, P, LJ.CELL), int(read_guarded(errors[0], 1)[0]), table, errors


@pytest.mark.parametrize("n", LJ.CASE_N)
def test_tally_equals_the_judge(lib, n):
    """P in {1, 2, 3, 16} x every termination pattern x strides 1, 8, 3 x both score formats; members_p1 NULL and given, the
    three member formats, invalid members on both sides (counted in errors only), games that did not end holding random scores
    and invalid members, into a table preloaded near 2^40 and a preloaded errors word"""
    for P in LJ.CASE_P:
        for case in LJ.tally_cases(n, P):
            x = LJ.tally_inputs(case)
            want, want_errors = LJ.tally(x["terminated"], x["buf1"], x["buf2"], case["stride"], x["members_p1"], x["members_p2"], P, x["table"], x["errors"])
            got, errors, _, _ = run_tally(lib, case, x)
            assert errors == want_errors, (case, errors, want_errors)
            assert np.array_equal(got, want), (case, np.argwhere(got != want)[:8])                  # (preloaded near 2^40: 64-bit adds)


def test_a_second_tally_adds_to_the_first(lib):
    case = LJ.tally_cases(4099, 16)[9]
    assert case["terminated"] == "all"
    x = LJ.tally_inputs(case)
    args = (x["terminated"], x["buf1"], x["buf2"], case["stride"], x["members_p1"], x["members_p2"], 16)
    once = LJ.tally(*args, x["table"], x["errors"])
    twice = LJ.tally(*args, *once)
    got1, err1, table, errors = run_tally(lib, case, x)
    got2, err2, _, _ = run_tally(lib, case, x, table, errors)
    assert np.array_equal(got1, once[0]) and err1 == once[1] and np.array_equal(got2, twice[0]) and err2 == twice[1]
    assert twice[0][..., 0].sum() - once[0][..., 0].sum() + twice[1] - once[1] == 4099


# ---- the binding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_format", ["int32", "packed"])
def test_tally_on_a_real_env_until_games_end(state_format):
    """``env.scores`` of either state format, read right after ``env.step``: the judge's table from the same views"""
    from pikazoo_amd import league, pikazoo_v0

    n, P = 300, 4
    env = pikazoo_v0.env(num_envs=n, device=DEV, seed=5, winning_score=1, state_format=state_format, validate_actions=False)
    env.reset()
    assert env.scores.dtype == (torch.int32 if state_format == "int32" else torch.int16)
    assert env.scores.stride(0) == (1 if state_format == "int32" else 8)
    members = torch.from_numpy(np.random.default_rng(0).integers(0, P, n)).to(DEV)
    table = torch.zeros((P, P, 4), dtype=torch.int64, device=DEV)
    errors = torch.zeros(1, dtype=torch.int64, device=DEV)
    want, ended = np.zeros((P, P, 4), np.int64), 0
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(400):
        actions = {a: torch.randint(0, 18, (n,), device=DEV, generator=gen) for a in env.agents}
        _, _, terminations, _, _ = env.step(actions)
        term = terminations[A1]
        assert league.tally(term, env.scores, members, P, table=table, errors=errors) is table
        scores = cpu(env.scores)
        want, bad = LJ.tally(cpu(term), scores[:, 0], scores[:, 1], 1, None, cpu(members), P, want)
        ended += int(cpu(term).sum())
        assert bad == 0
        if ended >= 200:
            break
    assert ended >= 200, "no game ended: the test saw nothing"
    assert np.array_equal(cpu(table), want) and int(errors.item()) == 0
    assert want[0, :, 0].sum() == ended and (want[1:] == 0).all() and (want[0, :, 2] + want[0, :, 3] == want[0, :, 0]).all()   # winning_score = 1
    # a fresh table when none is given, uint8 flags and members, members_p1 given
    m8 = members.to(torch.uint8)
    fresh = league.tally(term.to(torch.uint8), env.scores, m8, P, members_p1=m8)
    scores = cpu(env.scores)
    assert np.array_equal(cpu(fresh), LJ.tally(cpu(term), scores[:, 0], scores[:, 1], 1, cpu(m8), cpu(m8), P)[0])


def test_draw_binding_allocates_reuses_and_masks():
    from pikazoo_amd import league

    n = 4099
    w = np.array([5, 0, 1, 9], np.int64)
    weights = on_device(w)
    for dtype in (torch.int64, torch.int32, torch.uint8):
        got = league.draw(weights, n, seed=11, counter=3, first_game=(1 << 32) + 7, dtype=dtype)
        assert got.dtype == dtype and np.array_equal(cpu(got).astype(np.int64), LJ.draw(w, n, 11, 3, (1 << 32) + 7)[0])
    out = torch.full((n,), LJ.PLANTED, dtype=torch.int64, device=DEV)
    counter = torch.tensor([40], dtype=torch.int64, device=DEV)
    mask = torch.arange(n, device=DEV) % 3 == 0
    errors = torch.zeros(1, dtype=torch.int32, device=DEV)
    at = out.data_ptr()
    assert league.draw(weights, n, seed=-2, counter=counter, mask=mask, out=out, errors=errors) is out and out.data_ptr() == at
    want, _ = LJ.draw(w, n, -2, 40, 0, cpu(mask))
    assert np.array_equal(cpu(out), want) and (want[1::3] == LJ.PLANTED).all()
    counter += 1                                                              # the device counter is read when the launch runs
    league.draw(weights, n, seed=-2, counter=counter, out=out, errors=errors)
    assert np.array_equal(cpu(out), LJ.draw(w, n, -2, 41)[0]) and int(errors.item()) == 0
    league.draw(on_device(np.array([0, 0], np.int64)), n, seed=0, out=out, errors=errors)
    assert int(errors.item()) == 1 and np.array_equal(cpu(out), LJ.draw(w, n, -2, 41)[0])
    assert tuple(league.draw(weights, 0, seed=0).shape) == (0,)
    masked = league.draw(weights, n, seed=1, mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    assert not masked.any()                                                    # an allocated vector under a mask starts as zeros


def test_matchmaker_under_a_captured_graph():
    """record + rematch captured once and replayed three times: the device counter advances, every replay's draw is the
    judge's for its counter under the weights the table gave, the table is the judge's sum, and push() zeroes a row and a
    column"""
    from pikazoo_amd import league, net, pool

    n, cap = 1000, 4
    model = net.ActorCritic().to(DEV)
    snapshots = pool.Snapshots(model, cap)
    mm = league.Matchmaker(snapshots, n, seed=77, first_game=1 << 33)
    assert mm.push() == 1 and mm.push() == 2 and len(snapshots) == 3
    rng = np.random.default_rng(3)
    term = torch.zeros(n, dtype=torch.bool, device=DEV)
    scores = torch.zeros((n, 2), dtype=torch.int32, device=DEV)

    def step():
        mm.record(term, scores)
        return mm.rematch(mask=term)

    def feed():
        t, s = rng.random(n) < 0.3, rng.integers(0, 16, (n, 2)).astype(np.int32)
        term.copy_(torch.from_numpy(t))
        scores.copy_(torch.from_numpy(s))
        return t, s

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up: libraries, plans, allocator
        t, s = feed()
        plan = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    members = np.zeros(n, np.int64)
    table = np.zeros((cap, cap, 4), np.int64)

    def judge(t, s, counter):
        nonlocal members, table
        table, bad = LJ.tally(t, s[:, 0], s[:, 1], 1, None, members, cap, table)
        assert bad == 0
        # the weights are plain torch on the table (the caller's policy choice, held to its restatement within 1 as on the
        # CPU); the draw is judged on the weights it was given
        weights = cpu(mm.weights())
        assert np.abs(weights - LJ.pfsp_weights(table, 3)).max() <= 1 and weights[3] == 0
        kept = members.copy()
        members, errors = LJ.draw(weights, n, 77, counter, 1 << 33, t, prior=members)
        assert errors == 0 and members.max() < 3 and (members[~t] == kept[~t]).all()

    judge(t, s, 0)
    assert np.array_equal(cpu(mm.members), members) and np.array_equal(cpu(mm.table), table) and cpu(mm.counter).tolist() == [1]
    graph = torch.cuda.CUDAGraph()
    t, s = feed()
    with torch.cuda.graph(graph):
        captured = step()
    assert captured is plan                                                    # one Plan per pool size, overwritten in place
    for replay in range(3):
        if replay:
            t, s = feed()
        before = cpu(mm.counter)[0]
        graph.replay()
        torch.cuda.synchronize()
        # (the capture itself ran nothing: the first replay is the first execution of its launches)
        judge(t, s, int(before))
        assert cpu(mm.counter)[0] == before + 1 == 2 + replay
        assert np.array_equal(cpu(mm.members), members), replay
        assert np.array_equal(cpu(mm.table), table), replay
        order, first, bad = PJ.plan(members, 3)
        assert np.array_equal(cpu(plan.order), order) and np.array_equal(cpu(plan.first), first) and int(plan.errors.item()) == bad == 0
    assert mm.check() is mm and table[0, :3, 0].sum() > 0 and (table[1:] == 0).all()
    rates = cpu(mm.win_rates())
    assert np.allclose(rates[:3], table[0, :3, 1] / table[0, :3, 0]) and np.isnan(rates[3])
    assert mm.push() == 3 and mm.push() == 1                                  # the ring overwrites member 1
    table[1] = 0
    table[:, 1] = 0
    table[3] = 0
    table[:, 3] = 0
    assert np.array_equal(cpu(mm.table), table) and table[0, 1].sum() == 0 and table[0, 2, 0] > 0


def test_the_league_example_runs_with_pfsp_and_as_before_without():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "examples"))
    import ppo_league

    lines = []
    losses = ppo_league.main(num_envs=256, iters=2, steps=8, snapshot_every=1, log=lines.append, pfsp=True)
    assert len(losses) == 2 * 2 * 4 and np.isfinite(losses).all() and len(lines) == 2
    assert "pool 2" in lines[0] and "pool 3" in lines[1] and all("win rate" in line for line in lines)
    # the default route: what it returned before the flag existed, twice the same
    plain = []
    a = ppo_league.main(num_envs=256, iters=2, steps=8, snapshot_every=1, log=plain.append)
    b = ppo_league.main(num_envs=256, iters=2, steps=8, snapshot_every=1, log=lambda line: None, pfsp=False)
    assert a == b and len(a) == 16 and np.isfinite(a).all() and len(plain) == 2 and not any("win rate" in line for line in plain)
    assert "pool 2" in plain[0] and "pool 3" in plain[1]
