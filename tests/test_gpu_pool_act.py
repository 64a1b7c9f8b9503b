"""GPU tests (``-m gpu``) of the pool-act launch (include/pikazoo_pool_act.h: ``pz_mlp_act_pool``) and of
``pikazoo_amd.pool_act``.

Two references, kept apart.  (1) The header's promise: on every row of a valid member the bits of pz_mlp_forward_pool (float32)
followed by pz_sample_actions on the same inputs -- actions, log-prob, entropy, value and head compared bit for bit.  (2) The
float64 judge of tests/pool_act_judge.py, which knows nothing of the older kernels (its ``verdict``; tests/test_pool_act_host.py
holds it to seven mutants on exactly the cases used here).  Every C-ABI launch writes into sentinel-filled outputs with elements
in front of the first one and behind the last one (and in the head's pad columns), all of which must keep the sentinel, as must
every output of a row whose member is invalid and every buffer behind a pointer that was not given; the pad columns of the
observations and the memory around the parameters hold NaN patterns.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import net_judge as N
import policy_judge as J
import pool_act_judge as PA
import pool_judge as PJ
from test_gpu_net import device_obs, device_params
from test_gpu_policy import SENT, TAIL, TORCH_ACTION, cpu, stream
from test_gpu_pool import a_model, member_array, run_plan

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
REPO = Path(__file__).resolve().parent.parent
FRONT = 8  # elements in front of every output vector (8: an int64 vector stays aligned)
CASES = PA.cases()
KEYS = ("head", "actions", "log_probs", "entropy", "values")


@pytest.fixture(scope="module")
def libs():
    from pikazoo_amd import act, policy, pool, pool_act

    return pool_act.load(), pool.load(), policy.load(), act.load()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


class Device:
    """the device buffers of one case, shared by the launches that are compared"""

    def __init__(self, libs, case, obs=None, params=None, members=None):
        self.case = case
        if obs is None:
            obs, params = PA.case_inputs(case)
            members = PA.case_members(case)
        self.obs, self.params, self.members = obs, params, members
        self.sides, self.n = len(obs), obs[0].shape[0]
        self.obs_pitch, self.head_pitch = case["K"] + case["obs_extra"], case["O"] + case["head_extra"]
        self.xs = [device_obs(x, case["obs_dtype"], self.obs_pitch, case["offset"]) for x in obs]
        self.sets = [device_params(p, case["offset"]) for p in params]
        self.plans = []
        for m in members:
            if m is None:
                self.plans.append(None)
                continue
            order, first, errors, tensors = run_plan(libs[1], m, case["P"])
            want = PJ.plan(m, case["P"])
            assert np.array_equal(order, want[0]) and np.array_equal(first, want[1]) and errors == want[2]
            self.plans.append(tensors)
        self.written = [PA.effective(case, members, s)[1] for s in range(self.sides)]

    def args(self):
        """the arguments the pool's forward and the fused launch share: obs_p1 .. first_p2"""
        c, second = self.case, self.sides == 2
        plan_ptrs = []
        for s in range(2):
            p = self.plans[s] if s < self.sides else None
            plan_ptrs += [p[0][1], p[1][1]] if p is not None else [None, None]
        return (self.xs[0][1], self.xs[1][1] if second else None, N.OBS_DTYPES.index(c["obs_dtype"]), self.n, c["K"], self.obs_pitch, c["H"],
                c["O"], N.ACTIVATIONS.index(c["activation"]), member_array(self.sets), c["P"], *plan_ptrs)


def vectors(sides, n, dtype):
    return [torch.full((FRONT + n + TAIL,), SENT, dtype=dtype, device="cuda:0") for _ in range(sides)]


def pointers(ts, on, itemsize=4, front=FRONT):
    return [(ts[s].data_ptr() + front * itemsize if s < len(ts) and on[s] else None) for s in (0, 1)]


def read_vectors(ts, n, on, written, what):
    """the n elements of every vector; the guards, the rows that must not be written and a vector that was not asked for all
    hold the sentinel"""
    out = []
    for s, t in enumerate(ts):
        flat = cpu(t)
        assert (flat[:FRONT] == SENT).all() and (flat[FRONT + n:] == SENT).all(), f"{what}: written outside its rows"
        assert on[s] or (flat == SENT).all(), f"{what} of side {s}: written though it was not asked for"
        rows = flat[FRONT:FRONT + n]
        assert (rows[~written[s]] == SENT).all(), f"{what} of side {s}: a row of an invalid member was written"
        out.append(rows if on[s] else None)
    return out


def read_heads(heads, n, O, pitch, offset, on, written):
    out = []
    for s, h in enumerate(heads):
        flat = cpu(h)
        rows = flat[offset:offset + n * pitch].reshape(n, pitch)
        assert (flat[:offset] == SENT).all() and (flat[offset + n * pitch:] == SENT).all(), "the head outside its rows"
        assert (rows[:, O:] == SENT).all(), "a pad column of the head was written"
        assert on[s] or (flat == SENT).all(), f"the head of side {s}: written though it was not asked for"
        assert (rows[~written[s]] == SENT).all(), f"the head of side {s}: a row of an invalid member was written"
        out.append(np.ascontiguousarray(rows[:, :O]).view(np.float32) if on[s] else None)
    return out


def draw_args(draw):
    seed, first_game, step, step_dev = draw
    dev = torch.tensor([step_dev], dtype=torch.int64, device="cuda:0") if step_dev is not None else None
    return dev, (seed, first_game, step, dev.data_ptr() if dev is not None else None)


def run_fused(libs, d, stats=None, head=None, draw=None, expect=0):
    """pz_mlp_act_pool: per side a dict (written, head or None, actions int64, log_probs, entropy, values or None) as numpy"""
    c, n, sides = d.case, d.n, d.sides
    O, A = c["O"], c["A"]
    stats = tuple(c["stats"] if stats is None else stats)
    head = tuple([True] * sides if head is None else head)
    values = tuple(on and O > A for on in stats)
    asize = 8 if c["action_dtype"] == "int64" else 4
    act, logp, ent, val = (vectors(sides, n, t) for t in (TORCH_ACTION[c["action_dtype"]], torch.int32, torch.int32, torch.int32))
    heads = [torch.full((c["offset"] + n * d.head_pitch + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(sides)]
    dev, dargs = draw_args(PA.DRAWS[c["draw"]] if draw is None else draw)
    err = libs[0].pz_mlp_act_pool(*d.args(), A, *dargs, J.ACTION_DTYPES.index(c["action_dtype"]), *pointers(act, [True] * sides, asize),
                                  *pointers(logp, stats), *pointers(ent, stats), *pointers(val, values), *pointers(heads, head, front=c["offset"]),
                                  d.head_pitch, stream())
    assert err == expect
    torch.cuda.synchronize()
    a = [cpu(t)[FRONT:FRONT + n] for t in act]
    written = [x != SENT for x in a]
    for s in range(sides):
        assert np.array_equal(written[s], d.written[s]), f"side {s}: the rows of valid members are written, those of invalid ones are not"
    a = read_vectors(act, n, [True] * sides, written, "actions")
    lp, en, va = (read_vectors(ts, n, on, written, what) for ts, on, what in ((logp, stats, "log_probs"), (ent, stats, "entropy"), (val, values, "values")))
    hs = read_heads(heads, n, O, d.head_pitch, c["offset"], head, written)
    f32 = lambda x: None if x is None else np.ascontiguousarray(x).view(np.float32)  # noqa: E731
    return [dict(written=written[s], head=hs[s], actions=a[s].astype(np.int64), log_probs=f32(lp[s]), entropy=f32(en[s]), values=f32(va[s]))
            for s in range(sides)]


def run_two_launches(libs, d, draw=None):
    """pz_mlp_forward_pool (float32, at the head's pitch) and pz_sample_actions on its logits: the same dicts (a row of an
    invalid member holds what the second launch made of the sentinel: it is compared nowhere)"""
    c, n, sides = d.case, d.n, d.sides
    O, A = c["O"], c["A"]
    asize = 8 if c["action_dtype"] == "int64" else 4
    on = [True] * sides
    heads = [torch.full((c["offset"] + n * d.head_pitch + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(sides)]
    hp = pointers(heads, on, front=c["offset"])
    assert libs[1].pz_mlp_forward_pool(*d.args(), *hp, 0, d.head_pitch, stream()) == 0
    act, logp, ent = (vectors(sides, n, t) for t in (TORCH_ACTION[c["action_dtype"]], torch.int32, torch.int32))
    dev, dargs = draw_args(PA.DRAWS[c["draw"]] if draw is None else draw)
    assert libs[2].pz_sample_actions(*hp, 0, A, n, d.head_pitch, *dargs, J.ACTION_DTYPES.index(c["action_dtype"]), *pointers(act, on, asize),
                                     *pointers(logp, on), *pointers(ent, on), stream()) == 0
    torch.cuda.synchronize()
    everything = [np.ones(n, bool)] * sides
    hs = read_heads(heads, n, O, d.head_pitch, c["offset"], on, d.written)
    a, lp, en = (read_vectors(ts, n, on, everything, what) for ts, what in ((act, "actions"), (logp, "log_probs"), (ent, "entropy")))
    return [dict(written=d.written[s], head=hs[s], actions=a[s].astype(np.int64), log_probs=lp[s].view(np.float32), entropy=en[s].view(np.float32),
                 values=np.ascontiguousarray(hs[s][:, A]) if O > A else None) for s in range(sides)]


def same_bits(got, want, what, keys=KEYS):
    """on the rows that are written, every output that `got` holds has the bits of `want`'s"""
    compared = 0
    for s, (g, w) in enumerate(zip(got, want)):
        rows = g["written"]
        assert np.array_equal(rows, w["written"]), (what, "side", s)
        for key in keys:
            if g[key] is None:
                continue
            assert w[key] is not None, (what, key)
            differ = int((bits(g[key])[rows] != bits(w[key])[rows]).sum())
            assert differ == 0, (what, "side", s, key, differ, "elements differ")
            compared += 1
    assert compared


_runs = {}


def case_run(libs, index):
    """(the device buffers, the fused launch with the case's statistics and both heads) of a case, launched once"""
    if index not in _runs:
        _runs.clear()                                  # (one case's buffers at a time)
        d = Device(libs, CASES[index])
        _runs[index] = (d, run_fused(libs, d))
    return _runs[index]


# ---- 1. the bits of the two launches, 2. the float64 judge ------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)))
def test_cases_return_the_bits_of_the_two_launches(libs, index):
    """every case of pool_act_judge.cases(): on the rows of valid members the bits of pz_mlp_forward_pool followed by
    pz_sample_actions, the head included; rows of invalid members keep the sentinel in every output (checked by the reader)"""
    case = CASES[index]
    if "max_cus" in case:  # (a case sized so that a workgroup walks several groups under the grid cap of such a device)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print(f"case {index}: {cus} compute units, n = {case['n']}")
        assert cus <= case["max_cus"], "this case's n is sized for a smaller grid cap: it no longer reaches the path it is here for"
    d, got = case_run(libs, index)
    same_bits(got, run_two_launches(libs, d), f"case {index}")
    for s in range(d.sides):
        assert (got[s]["values"] is None) == (case["O"] == case["A"] or not case["stats"][s])


@pytest.mark.parametrize("index", range(len(CASES)))
def test_cases_against_the_float64_judge(libs, index):
    """... and the same launch against the float64 judge, independently of the older kernels"""
    d, got = case_run(libs, index)
    amb, fails = PA.verdict(d.case, got, d.obs, d.params, d.members, what=f"case {index}")
    assert not fails, fails


# ---- 3. the optional outputs ---------------------------------------------------------------------------------------------------------
def case_index(**want):
    return next(i for i, c in enumerate(CASES) if all(c[k] == v for k, v in want.items()))


STATS_CASES = (case_index(n=257, P=16, kinds=("round_robin", "reverse_sorted")), case_index(n=4099, P=16, kinds=(None, "invalid_entries")),
               case_index(K=72, H=128, O=33, activation="relu"), case_index(n=40000))


@pytest.mark.parametrize("index", STATS_CASES)
def test_statistics_off_leave_the_actions_and_write_nothing_else(libs, index):
    """with the statistics off for agent 2 (the league's call), for agent 1, and for both, every action is the bit it is with
    them on, the other agent's outputs keep their bits, and nothing behind the absent pointers is written (the reader)"""
    d = Device(libs, CASES[index])
    full = run_fused(libs, d, stats=(True, True))
    for stats in ((True, False), (False, True), (False, False)):
        got = run_fused(libs, d, stats=stats, head=(False, False))
        same_bits(got, full, f"case {index} stats {stats}", keys=("actions", "log_probs", "entropy", "values"))
        for s in (0, 1):
            assert all((got[s][key] is None) != stats[s] for key in ("log_probs", "entropy")) and got[s]["head"] is None
            assert (got[s]["values"] is not None) == (stats[s] and d.case["O"] > d.case["A"])
    # each of the three on its own, per agent
    A, O, n = d.case["A"], d.case["O"], d.n
    act, logp, ent, val = (vectors(2, n, t) for t in (TORCH_ACTION[d.case["action_dtype"]], torch.int32, torch.int32, torch.int32))
    dev, dargs = draw_args(PA.DRAWS[d.case["draw"]])
    asize = 8 if d.case["action_dtype"] == "int64" else 4
    assert libs[0].pz_mlp_act_pool(*d.args(), A, *dargs, J.ACTION_DTYPES.index(d.case["action_dtype"]), *pointers(act, (True, True), asize),
                                   *pointers(logp, (True, False)), *pointers(ent, (False, True)), *pointers(val, (False, O > A)), None, None, O,
                                   stream()) == 0
    torch.cuda.synchronize()
    a = read_vectors(act, n, (True, True), d.written, "actions")
    lp, en, va = (read_vectors(ts, n, on, d.written, what) for ts, on, what in ((logp, (True, False), "log_probs"), (ent, (False, True), "entropy"),
                                                                                (val, (False, O > A), "values")))
    for s in (0, 1):
        w = d.written[s]
        assert np.array_equal(a[s].astype(np.int64)[w], full[s]["actions"][w])
    assert np.array_equal(lp[0][d.written[0]], bits(full[0]["log_probs"]).view(np.int32)[d.written[0]])
    assert np.array_equal(en[1][d.written[1]], bits(full[1]["entropy"]).view(np.int32)[d.written[1]])
    if O > A:
        assert np.array_equal(va[1][d.written[1]], bits(full[1]["values"]).view(np.int32)[d.written[1]])


@pytest.mark.parametrize("index", STATS_CASES[:3])
def test_the_head_changes_no_other_output(libs, index):
    """the head is pz_mlp_forward_pool's (held in test 1); with it off, or given for one agent alone, every other output keeps
    its bits and the absent head is not written"""
    d, full = case_run(libs, index)
    for head in ((False, False), (True, False), (False, True)):
        got = run_fused(libs, d, head=head)
        same_bits(got, full, f"case {index} head {head}")
        assert [g["head"] is not None for g in got] == list(head)


# ---- 4. one member without plans is pz_mlp_act ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,activation", [((35, 64, 19, 18), "tanh"), ((72, 128, 33, 32), "relu"), ((8, 32, 2, 2), "tanh")])
def test_one_member_and_no_plans_equal_pz_mlp_act(libs, size, activation):
    K, H, O, A = size
    case = dict(CASES[0], K=K, H=H, O=O, A=A, activation=activation, n=4099, P=1, kinds=(None, None), draw=1, head_extra=2, offset=1, seed=90)
    d = Device(libs, case)
    got = run_fused(libs, d)
    n, sides = d.n, 2
    act, logp, ent, val = (vectors(sides, n, t) for t in (torch.int64, torch.int32, torch.int32, torch.int32))
    heads = [torch.full((1 + n * d.head_pitch + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(sides)]
    dev, dargs = draw_args(PA.DRAWS[1])
    on, values = (True, True), (O > A, O > A)
    assert libs[3].pz_mlp_act(*d.args()[:9], *d.sets[0][1], *d.sets[0][1], A, *dargs, 1, *pointers(act, on, 8), *pointers(logp, on), *pointers(ent, on),
                              *pointers(val, values), *pointers(heads, on, front=1), d.head_pitch, stream()) == 0
    torch.cuda.synchronize()
    a, lp, en, va = (read_vectors(ts, n, o, d.written, w) for ts, o, w in ((act, on, "actions"), (logp, on, "log_probs"), (ent, on, "entropy"), (val, values, "values")))
    hs = read_heads(heads, n, O, d.head_pitch, 1, on, d.written)
    f32 = lambda x: None if x is None else np.ascontiguousarray(x).view(np.float32)  # noqa: E731
    want = [dict(written=d.written[s], head=hs[s], actions=a[s].astype(np.int64), log_probs=f32(lp[s]), entropy=f32(en[s]), values=f32(va[s]))
            for s in range(sides)]
    same_bits(got, want, f"{size} {activation}")
    # ... and a plan of one member changes nothing
    planned = Device(libs, dict(case, kinds=("round_robin", None)), d.obs, d.params, [np.zeros(n, np.int32), None])
    same_bits(run_fused(libs, planned), want, f"{size} {activation} with a plan")


# ---- 5. shard, 6. n = 0 --------------------------------------------------------------------------------------------------------------
def test_a_shard_returns_the_bits_of_the_whole_batch_s_tail(libs):
    """rows [g0, n) with first_game + g0 and a plan over those rows: a row's bits depend neither on the batch nor on the plan"""
    case = dict(CASES[0], n=1000, P=3, kinds=("round_robin", "invalid_entries"), draw=1, seed=91)
    g0 = 333
    d = Device(libs, case)
    whole = run_fused(libs, d)
    seed, first, step, dev = PA.DRAWS[1]
    part = Device(libs, dict(case, n=case["n"] - g0), [x[g0:] for x in d.obs], d.params, [m[g0:] for m in d.members])
    shard = run_fused(libs, part, draw=(seed, first + g0, step, dev))
    same_bits(shard, [{k: (v[g0:] if v is not None else None) for k, v in side.items()} for side in whole], "shard")
    rows = whole[0]["written"][:case["n"] - g0] & shard[0]["written"]
    assert not np.array_equal(shard[0]["actions"][rows], whole[0]["actions"][:case["n"] - g0][rows])


def test_zero_rows_launch_nothing(libs):
    case = dict(CASES[0], n=0, P=3, kinds=("round_robin", None))
    obs = [N.make_obs(0, 35, "float32", s) for s in (0, 1)]
    params = [N.make_params(35, 64, 19, p) for p in range(3)]
    d = Device(libs, case, obs, params, [np.zeros(0, np.int32), None])
    run_fused(libs, d)  # (every sentinel intact: checked by the reader)


# ---- 7. the binding -------------------------------------------------------------------------------------------------------------------
def two_calls(league, obs, sides, A, **kw):
    """Snapshots.act and policy.sample on its logits: the route the fused launch replaces"""
    from pikazoo_amd import policy

    head = league.act(obs, sides)
    picked = policy.sample({a: h[:, :A] for a, h in head.items()}, **kw)
    return head, picked


def assert_equals_two_calls(out, head, picked, agents, stats, A, rows=None):
    for a in agents:
        keep = slice(None) if rows is None or rows[a] is None else rows[a]
        assert torch.equal(out["actions"][a][keep], picked["actions"][a][keep]), a
        if a in stats:
            for key in ("log_probs", "entropy"):
                assert np.array_equal(bits(cpu(out[key][a][keep])), bits(cpu(picked[key][a][keep]))), (a, key)
            assert np.array_equal(bits(cpu(out["values"][a][keep])), bits(cpu(head[a][:, A][keep]))), a
        else:
            assert all(a not in out[key] for key in ("log_probs", "entropy", "values"))


def test_sample_its_out_argument_and_the_snapshots(libs):
    from pikazoo_amd import pool, pool_act

    n, K, A, P = 1000, 35, 18, 4
    models = [a_model(50 + p) for p in range(P)]
    member_params = [m.parameter_tensors() for m in models]
    obs = {a: torch.from_numpy(N.make_obs(n, K, "float32", seed)).to("cuda:0") for a, seed in ((A1, 60), (A2, 61))}
    values = PJ.member_vector("invalid_entries", n, P, seed=3)
    members = torch.from_numpy(PJ.invalid_for(values, "int64")).to("cuda:0")
    plan = pool.plan(members, P)
    valid = torch.from_numpy(PJ.valid_rows(cpu(members), P)).to("cuda:0")
    sides = {A1: None, A2: plan}
    head = pool.forward(obs, member_params, sides)
    from pikazoo_amd import policy

    picked = policy.sample({a: h[:, :A] for a, h in head.items()}, seed=11, step=9, first_game=5)
    out = pool_act.sample(obs, member_params, sides, A, seed=11, step=9, first_game=5, head=True)
    assert list(out) == ["actions", "log_probs", "entropy", "values", "head"] and all(list(v) == [A1, A2] for v in out.values())
    rows = {A1: None, A2: valid}
    assert_equals_two_calls(out, head, picked, (A1, A2), (A1, A2), A, rows)
    assert torch.equal(out["head"][A1], head[A1]) and torch.equal(out["head"][A2][valid], head[A2][valid])
    # out= reuse: the same tensors, the same bits, rows of invalid members left as they were
    ptrs = {k: {a: t.data_ptr() for a, t in v.items()} for k, v in out.items()}
    out["actions"][A2][~valid] = -3
    again = pool_act.sample(obs, member_params, sides, A, seed=11, step=9, first_game=5, head=True, out=out)
    assert again is out and ptrs == {k: {a: t.data_ptr() for a, t in v.items()} for k, v in out.items()}
    assert (out["actions"][A2][~valid] == -3).all()
    assert_equals_two_calls(out, head, picked, (A1, A2), (A1, A2), A, rows)
    # the league's call: the learner's statistics only, int32 actions, a device step; and one agent as a tensor
    lean = pool_act.sample(obs, member_params, sides, A, seed=11, step=torch.tensor([4], device="cuda:0") + 5, first_game=5,
                           action_dtype=torch.int32, stats={A1}, head={A2})
    assert list(lean) == ["actions", "log_probs", "entropy", "values", "head"] and list(lean["actions"]) == [A1, A2]
    assert all(list(lean[key]) == [A1] for key in ("log_probs", "entropy", "values")) and list(lean["head"]) == [A2]
    assert lean["actions"][A1].dtype == torch.int32
    assert_equals_two_calls({**lean, "actions": {a: t.to(torch.int64) for a, t in lean["actions"].items()}}, head, picked, (A1, A2), (A1,), A, rows)
    assert torch.equal(lean["head"][A2][valid], head[A2][valid])
    clean = torch.from_numpy(PJ.member_vector("round_robin", n, P)).to("cuda:0")
    pool.plan(clean, P, out=plan).check()
    one = pool_act.sample(obs[A2], member_params, plan, A, seed=11, step=9, first_game=5, stats=False)
    assert list(one) == ["actions"] and isinstance(one["actions"], torch.Tensor)
    head2 = pool.forward(obs, member_params, {A1: plan, A2: plan})
    picked2 = policy.sample({a: h[:, :A] for a, h in head2.items()}, seed=11, step=9, first_game=5)
    both = pool_act.sample(obs, member_params, {A1: plan, A2: plan}, A, seed=11, step=9, first_game=5)
    assert_equals_two_calls(both, head2, picked2, (A1, A2), (A1, A2), A)
    full = pool_act.sample(obs[A1], member_params, plan, A, seed=11, step=9, first_game=5)     # (a tensor is agent 1: word 0)
    assert torch.equal(full["actions"], both["actions"][A1]) and torch.equal(full["log_probs"], both["log_probs"][A1])
    assert len(set(cpu(both["actions"][A1]).tolist())) > 4
    for bad in (lambda: pool_act.sample(obs, member_params, sides, A, seed=1, out=lean),
                lambda: pool_act.sample(obs, member_params, sides, A, seed=1, step=torch.zeros(1, dtype=torch.int64)),
                lambda: pool_act.sample(obs, member_params, sides, A, seed=1, out={**out, "head": obs}, head=True),
                lambda: pool_act.sample(obs[A2][:500], member_params, plan, A, seed=1),
                lambda: pool_act.sample(obs, member_params[:3], sides, A, seed=1)):
        with pytest.raises(ValueError):
            bad()


def test_snapshots_act_sample_under_a_captured_graph(libs):
    """``Snapshots.act_sample`` and ``counter.add_(1)`` captured once; replays after a push(), after an optimizer step on member
    0 and after a re-plan into the same Plan equal ``Snapshots.act`` + ``policy.sample`` at the counter's step, bit for bit"""
    from pikazoo_amd import optim, pool

    n, K, A = 777, 35, 18
    model = a_model(70)
    with torch.no_grad():
        model.head.weight.mul_(20.0)  # (logits worth drawing from)
    league = pool.Snapshots(model, 3)
    for shift in (0.1, -0.2):
        league.push()
        with torch.no_grad():
            model.fc2.weight.add_(shift)
            model.head.bias.add_(shift)
    P = len(league)
    assert P == 3
    obs = {a: torch.from_numpy(N.make_obs(n, K, "float32", seed)).to("cuda:0") for a, seed in ((A1, 71), (A2, 72))}
    gen = torch.Generator(device="cuda:0").manual_seed(8)
    members = torch.randint(P, (n,), device="cuda:0", generator=gen)
    plan = pool.plan(members, P).check()
    sides = {A1: None, A2: plan}
    t0 = (1 << 33) + 40
    counter = torch.full((1,), t0, dtype=torch.int64, device="cuda:0")
    held = league.act_sample(obs, sides, seed=3, step=counter, first_game=77, stats={A1})
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = league.act_sample(obs, sides, seed=3, step=counter, first_game=77, stats={A1}, out=held)
            counter.add_(1)
    assert captured is held and list(held) == ["actions", "log_probs", "entropy", "values"]
    torch.cuda.synchronize()
    counter.fill_(t0)
    torch.cuda.synchronize()

    def replay_and_compare(step):
        graph.replay()
        torch.cuda.synchronize()
        head, picked = two_calls(league, obs, sides, A, seed=3, step=step, first_game=77)
        torch.cuda.synchronize()
        assert_equals_two_calls(held, head, picked, (A1, A2), (A1,), A)
        return {a: held["actions"][a].clone() for a in (A1, A2)}

    first = replay_and_compare(t0)
    second = replay_and_compare(t0 + 1)
    assert not torch.equal(first[A1], second[A1])
    assert league.push() == 1 and len(league) == 3                 # a push overwrites the oldest snapshot in place
    replay_and_compare(t0 + 2)
    optimizer = optim.Adam(model.parameters(), lr=1e-2)            # an optimizer step on member 0
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    optimizer.step()
    replay_and_compare(t0 + 3)
    members = torch.randint(P, (n,), device="cuda:0", generator=gen)  # opponents re-drawn into the same Plan
    assert pool.plan(members, P, out=plan) is plan
    replay_and_compare(t0 + 4)
    assert int(counter.item()) == t0 + 5


def test_env_step_takes_the_actions_as_they_are():
    from pikazoo_amd import net, pikazoo_v0, pool

    env = pikazoo_v0.env(num_envs=64, device="cuda:0", seed=5)
    obs, _ = env.reset()
    model = net.ActorCritic(in_features=obs[A1].shape[1]).to("cuda:0")
    league = pool.Snapshots(model, 3)
    league.push()
    plan = pool.plan(torch.arange(64, device="cuda:0") % 2, 2).check()
    out = None
    for t in range(3):
        out = league.act_sample(obs, {A1: None, A2: plan}, seed=5, step=t, stats={A1}, out=out)
        assert out["actions"][A1].dtype == torch.int64 and list(out["log_probs"]) == [A1]
        before = {a: out["actions"][a].data_ptr() for a in (A1, A2)}
        obs, rew, term, trunc, infos = env.step(out["actions"])
        assert {a: out["actions"][a].data_ptr() for a in (A1, A2)} == before
    env.unwrapped.check_actions()
    assert int(out["actions"][A1].max()) < 18 and int(out["actions"][A2].min()) >= 0


# ---- 8. the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pfsp", [False, True])
def test_the_league_example_returns_the_same_losses_with_the_fused_launch(pfsp):
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_league

    kw = dict(num_envs=256, iters=2, steps=8, snapshot_every=1, log=lambda *_: None, pfsp=pfsp)
    two = ppo_league.main(**kw)
    fused = ppo_league.main(fused_act=True, **kw)
    assert len(two) == 2 * 2 * 4 and all(np.isfinite(two)) and fused == two
