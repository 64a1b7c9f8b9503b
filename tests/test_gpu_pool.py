"""GPU tests (``-m gpu``) of the pool library (include/pikazoo_pool.h: ``pz_pool_plan``, ``pz_mlp_forward_pool``) and of
``pikazoo_amd.pool``.

The judge is tests/pool_judge.py: the header's plan in numpy integers, and ``net_judge.judge`` row by row under the row's own
member's parameters with its DERIVED tolerance (tests/test_pool_host.py holds the judge to a scalar formulation and to seven
mutants on exactly the cases used here).  No GPU result is ever an expected value.  Beside the judge, every valid row must
hold the BITS ``pz_mlp_forward`` writes for it with its member's parameters: that is the header's definition.  Every C-ABI
launch writes into sentinel-filled outputs with elements in front of the first row, behind the last one and in the pad
columns, all of which must keep the sentinel, as must the rows of invalid members and the words behind a plan's capacity;
the observations' pads and the memory around every parameter tensor hold NaN patterns, which must not reach any output.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import net_judge as N
import policy_judge as J
import pool_judge as PJ
from test_gpu_net import device_obs, device_params, run_forward
from test_gpu_policy import SENT, TAIL, cpu, stream

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
TORCH_MEMBER = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64}
FRONT = 3   # sentinel words in front of every plan buffer


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import pool

    return pool.load()


@pytest.fixture(scope="module")
def net_lib():
    from pikazoo_amd import net

    return net.load()


def guarded(words):
    """an int32 device buffer of `words` words between FRONT and TAIL sentinel words: (tensor, address of word 0)"""
    t = torch.full((FRONT + words + TAIL,), SENT, dtype=torch.int32, device="cuda:0")
    return t, t.data_ptr() + 4 * FRONT


def read_guarded(t, words):
    flat = cpu(t)
    assert (flat[:FRONT] == SENT).all() and (flat[FRONT + words:] == SENT).all(), "a plan buffer was written outside its words"
    return flat[FRONT:FRONT + words]


def run_plan(lib, members, P, expect=0):
    """pz_pool_plan on a typed member vector: (order, first, errors) as numpy, the device tensors (order, first) kept alive
    with their addresses; the words around every buffer, those behind the capacity included, must keep the sentinel"""
    n = len(members)
    cap = PJ.capacity(n, P)
    dev_members = torch.from_numpy(np.ascontiguousarray(members)).to("cuda:0") if n else None
    order, first, errors = guarded(cap), guarded(P + 1), guarded(1)
    err = lib.pz_pool_plan(dev_members.data_ptr() if n else None, PJ.MEMBER_DTYPES.index(str(members.dtype)), n, P, order[1], first[1], errors[1],
                           stream())
    assert err == expect
    torch.cuda.synchronize()
    return read_guarded(order[0], cap), read_guarded(first[0], P + 1), int(read_guarded(errors[0], 1)[0]), (order, first)


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PJ.PLAN_N)
def test_plan_equals_the_judge(lib, n):
    """every member vector x P in {1, 2, 3, 16}, the three formats: order and first word for word, errors the count"""
    for kind, P, dtype, members in PJ.plan_cases(n):
        want_order, want_first, want_errors = PJ.plan(members, P)
        order, first, errors, _ = run_plan(lib, members, P)
        assert np.array_equal(first, want_first), (kind, P, dtype, first, want_first)
        assert np.array_equal(order, want_order), (kind, P, dtype)
        assert errors == want_errors, (kind, P, dtype)


def test_plan_of_no_rows_and_a_second_plan_into_the_same_buffers(lib):
    order, first, errors, _ = run_plan(lib, np.zeros(0, np.int32), 3)
    assert (order == -1).all() and len(order) == 3 * PJ.G and (first == 0).all() and errors == 0
    # errors is SET by every plan, and a shorter run leaves no row of the previous one behind
    P, n = 3, 300
    a = PJ.invalid_for(PJ.member_vector("invalid_entries", n, P), "int64")
    b = PJ.typed(PJ.member_vector("all_one_member", n, P), "int64")
    order_t, first_t, errors_t = guarded(PJ.capacity(n, P)), guarded(P + 1), guarded(1)
    for members in (a, b, a):
        dev = torch.from_numpy(members).to("cuda:0")
        assert lib.pz_pool_plan(dev.data_ptr(), 2, n, P, order_t[1], first_t[1], errors_t[1], stream()) == 0
        torch.cuda.synchronize()
        want = PJ.plan(members, P)
        assert np.array_equal(read_guarded(order_t[0], PJ.capacity(n, P)), want[0]) and np.array_equal(read_guarded(first_t[0], P + 1), want[1])
        assert read_guarded(errors_t[0], 1)[0] == want[2]


# ---- the forward ------------------------------------------------------------------------------------------------------------
def member_array(sets):
    from pikazoo_amd import pool

    array = (pool.Member * 16)()
    for m, (_, ptrs) in enumerate(sets):
        array[m] = pool.Member(*ptrs)
    return array


def run_pool(lib, obs, obs_dtype, sets, plans, activation, out_dtype="float32", obs_pitch=None, out_pitch=None, offset=0, expect=0, shape=None):
    """pz_mlp_forward_pool on one or two agents' observations (`obs`: a list of [n, K] arrays; `sets`: the members' device
    parameter sets as device_params returns them; `plans`: per agent None or run_plan's device tensors): per side (the
    [n, O] outputs as float32 values, a mask of the rows that still hold the sentinel in every column); every buffer is
    checked for what must not have been written"""
    sides = len(obs)
    n, K = obs[0].shape
    H, O = shape
    obs_pitch, out_pitch = obs_pitch or K, out_pitch or O
    xs = [device_obs(x, obs_dtype, obs_pitch, offset) for x in obs]
    osize = 4 if out_dtype == "float32" else 2
    outs = [torch.full((offset + n * out_pitch + TAIL,), SENT, dtype=torch.int32 if osize == 4 else torch.int16, device="cuda:0") for _ in obs]
    optr = [o.data_ptr() + offset * osize for o in outs]
    second = sides == 2
    plan_ptrs = []
    for s in range(2):
        p = plans[s] if s < sides else None
        plan_ptrs += [p[0][1], p[1][1]] if p is not None else [None, None]
    err = lib.pz_mlp_forward_pool(xs[0][1], xs[1][1] if second else None, N.OBS_DTYPES.index(obs_dtype), n, K, obs_pitch, H, O,
                                  N.ACTIVATIONS.index(activation), member_array(sets), len(sets), *plan_ptrs, optr[0], optr[1] if second else None,
                                  N.OUT_DTYPES.index(out_dtype), out_pitch, stream())
    assert err == expect
    torch.cuda.synchronize()
    results = []
    for o in outs:
        flat = cpu(o)
        rows = flat[offset:offset + n * out_pitch].reshape(n, out_pitch)
        assert (flat[:offset] == SENT).all() and (flat[offset + n * out_pitch:] == SENT).all(), "an output outside its rows"
        assert (rows[:, O:] == SENT).all(), "a pad column of the output was written"
        bits = np.ascontiguousarray(rows[:, :O])
        untouched = (bits == SENT).all(axis=1)
        values = J.bits_to_float(bits.view(np.float32 if osize == 4 else (np.float16 if out_dtype == "float16" else np.uint16)), out_dtype)
        results.append((values, untouched))
    return results


def bits_of(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def case_setup(lib, case):
    obs, params = PJ.case_inputs(case)
    members = PJ.case_members(case)
    sets = [device_params(p, case["offset"]) for p in params]
    plans = []
    for m in members:
        if m is None:
            plans.append(None)
            continue
        order, first, errors, tensors = run_plan(lib, m, case["P"])
        want = PJ.plan(m, case["P"])
        assert np.array_equal(order, want[0]) and np.array_equal(first, want[1]) and errors == want[2]
        plans.append(tensors)
    return obs, params, members, sets, plans


@pytest.mark.parametrize("index", range(len(PJ.forward_cases())))
def test_forward_cases(lib, net_lib, index):
    """every case of pool_judge.forward_cases: each valid row within net_judge's tolerance of the float64 judge under its own
    member's parameters, bit-equal to pz_mlp_forward over the whole batch with that member's parameters, rows of invalid
    members untouched, and a second call returns the same bits"""
    case = PJ.forward_cases()[index]
    K, H, O, P, n = case["K"], case["H"], case["O"], case["P"], case["n"]
    if "max_cus" in case:  # (a case sized so that a workgroup walks several groups under the grid cap of such a device)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print(f"case {index}: {cus} compute units, n = {n}")
        assert cus <= case["max_cus"], "this case's n is sized for a smaller grid cap: it no longer reaches the path it is here for"
    obs, params, members, sets, plans = case_setup(lib, case)
    kw = dict(obs_pitch=K + case["obs_extra"], out_pitch=O + case["out_extra"], offset=case["offset"])
    have = run_pool(lib, obs, case["obs_dtype"], sets, plans, case["activation"], case["out_dtype"], shape=(H, O), **kw)
    again = run_pool(lib, obs, case["obs_dtype"], sets, plans, case["activation"], case["out_dtype"], shape=(H, O), **kw)
    effs = [PJ.effective_members(m, P) for m in members]
    used = sorted({0} | {int(p) for e in effs if e is not None for p in np.unique(e[e >= 0])})
    # pz_mlp_forward over the whole batch, once per member that occurs, both agents on that member's pointers
    whole = {p: run_forward(net_lib, obs, case["obs_dtype"], [params[p]], case["activation"], case["out_dtype"], shared=True, **kw) for p in used}
    for s in range(len(obs)):
        eff = np.zeros(n, np.int64) if effs[s] is None else effs[s]
        values, untouched = have[s]
        written = eff >= 0
        assert np.array_equal(untouched, ~written), f"side {s}: rows of invalid members must keep the sentinel, valid rows must be written"
        ref, tol = PJ.judge(obs[s], params, eff, case["activation"], case["out_dtype"])
        worst, rows = N.worst_share(values[written], ref[written], tol[written])
        print(f"case {index} side {s}: worst error / tolerance {worst:.4f}")
        assert worst <= 1, (index, s, worst, rows)
        expected_bits = np.zeros((n, O), np.uint32)
        for p in used:
            expected_bits[eff == p] = bits_of(whole[p][s])[eff == p]
        assert np.array_equal(bits_of(values)[written], expected_bits[written]), f"side {s}: not the bits of pz_mlp_forward"
        assert np.array_equal(bits_of(again[s][0])[written], bits_of(values)[written]) and np.array_equal(again[s][1], untouched)


def test_one_member_with_any_plan_is_pz_mlp_forward(lib, net_lib):
    K, H, O, n = 35, 64, 19, 257
    params = [N.make_params(K, H, O, 31)]
    obs = [N.make_obs(n, K, "float32", seed) for seed in (32, 33)]
    sets = [device_params(params[0])]
    want = run_forward(net_lib, obs, "float32", params, "tanh", shared=True)
    for plans in ([None, None], [run_plan(lib, np.zeros(n, np.uint8), 1)[3]] * 2, [None, run_plan(lib, np.zeros(n, np.int64), 1)[3]]):
        have = run_pool(lib, obs, "float32", sets, plans, "tanh", shape=(H, O))
        for s in (0, 1):
            assert np.array_equal(bits_of(have[s][0]), bits_of(want[s])) and not have[s][1].any()
            ref, tol = N.judge(obs[s], params[0], "tanh")
            assert N.worst_share(have[s][0], ref, tol)[0] <= 1


def test_rewritten_and_shared_parameters(lib):
    """a member whose parameters are rewritten between two launches is seen by the second one; two members pointing at the
    same tensors give what one member would"""
    K, H, O, n, P = 35, 64, 19, 300, 3
    params = [N.make_params(K, H, O, 40 + p) for p in range(P)]
    obs = [N.make_obs(n, K, "float32", 44)]
    members = PJ.typed(PJ.member_vector("round_robin", n, P), "int32")
    sets = [device_params(p) for p in params]
    plan = run_plan(lib, members, P)[3]
    first = run_pool(lib, obs, "float32", sets, [plan], "tanh", shape=(H, O))[0][0]
    ref, tol = PJ.judge(obs[0], params, PJ.effective_members(members, P), "tanh")
    assert N.worst_share(first, ref, tol)[0] <= 1
    fresh = N.make_params(K, H, O, 49)
    for t, p in zip(sets[1][0], fresh):                               # member 1's tensors, in place
        t[:p.size].copy_(torch.from_numpy(p.ravel()))
    second = run_pool(lib, obs, "float32", sets, [plan], "tanh", shape=(H, O))[0][0]
    ref2, tol2 = PJ.judge(obs[0], [params[0], fresh, params[2]], PJ.effective_members(members, P), "tanh")
    assert N.worst_share(second, ref2, tol2)[0] <= 1
    assert np.array_equal(bits_of(second)[members != 1], bits_of(first)[members != 1]) and N.worst_share(second, ref, tol)[0] > 1
    # members 0 and 2 on the same tensors: what the rows of member 2 would give as rows of member 0
    aliased = run_pool(lib, obs, "float32", [sets[0], sets[1], sets[0]], [plan], "tanh", shape=(H, O))[0][0]
    two = np.where(members == 2, 0, members).astype(np.int32)
    merged = run_pool(lib, obs, "float32", sets[:2], [run_plan(lib, two, 2)[3]], "tanh", shape=(H, O))[0][0]
    assert np.array_equal(bits_of(aliased), bits_of(merged))
    ref3, tol3 = PJ.judge(obs[0], [params[0], fresh], PJ.effective_members(two, 2), "tanh")
    assert N.worst_share(aliased, ref3, tol3)[0] <= 1


# ---- pikazoo_amd.pool --------------------------------------------------------------------------------------------------------
def a_model(seed, activation="tanh"):
    from pikazoo_amd import net

    torch.manual_seed(seed)
    model = net.ActorCritic(activation=activation).to("cuda:0")
    with torch.no_grad():
        for p in model.parameters():  # (biases away from 0, the head's weights away from the 0.01 gain)
            p.add_(torch.empty_like(p).uniform_(-0.2, 0.2))
    return model


def per_member(obs, member_params, members, activation="tanh"):
    """net.forward per member over the whole batch, selected by `members` (a device int64 tensor; None: member 0)"""
    from pikazoo_amd import net

    out = None
    for p, ps in enumerate(member_params):
        full = net.forward(obs, ps, activation)
        out = full.clone() if out is None else out
        if members is not None:
            out[members == p] = full[members == p]
    return out


def test_binding_plan_and_forward_with_out_reuse():
    from pikazoo_amd import pool

    n, K, P = 1000, 35, 4
    models = [a_model(50 + p) for p in range(P)]
    member_params = [m.parameter_tensors() for m in models]
    obs = {a: torch.from_numpy(N.make_obs(n, K, "float32", seed)).to("cuda:0") for a, seed in ((A1, 60), (A2, 61))}
    values = PJ.member_vector("invalid_entries", n, P, seed=3)
    members = torch.from_numpy(PJ.invalid_for(values, "int64")).to("cuda:0")
    plan = pool.plan(members, P)
    want = PJ.plan(cpu(members), P)
    assert np.array_equal(cpu(plan.order), want[0]) and np.array_equal(cpu(plan.first), want[1]) and int(plan.errors) == want[2] > 0
    assert plan.n == n and plan.num_members == P
    with pytest.raises(ValueError, match=f"{want[2]} of {n}"):
        plan.check()
    head = {a: torch.full((n, 19), float("inf"), device="cuda:0") for a in obs}
    got = pool.forward(obs, member_params, {A1: None, A2: plan}, out=head)
    assert all(got[a].data_ptr() == head[a].data_ptr() for a in obs)
    valid = torch.from_numpy(PJ.valid_rows(cpu(members), P)).to("cuda:0")
    assert torch.equal(head[A1], per_member(obs[A1], member_params, None))
    assert torch.equal(head[A2][valid], per_member(obs[A2], member_params, members)[valid]) and torch.isinf(head[A2][~valid]).all()
    host_params = [[cpu(p) for p in ps] for ps in member_params]
    ref, tol = PJ.judge(cpu(obs[A2]), host_params, PJ.effective_members(cpu(members), P), "tanh")
    assert N.worst_share(cpu(head[A2])[cpu(valid)], ref[cpu(valid)], tol[cpu(valid)])[0] <= 1
    # a clean draw, re-planned into the same Plan: no allocation, check() passes, one agent as a tensor
    clean = torch.from_numpy(PJ.member_vector("round_robin", n, P)).to("cuda:0")
    ptrs = (plan.order.data_ptr(), plan.first.data_ptr(), plan.errors.data_ptr())
    assert pool.plan(clean, P, out=plan) is plan and (plan.order.data_ptr(), plan.first.data_ptr(), plan.errors.data_ptr()) == ptrs
    plan.check()
    one = pool.forward(obs[A2], member_params, plan, out_dtype=torch.bfloat16)
    assert one.dtype == torch.bfloat16 and torch.equal(one, per_member(obs[A2], member_params, clean).to(torch.bfloat16))
    with pytest.raises(ValueError, match="overlaps"):
        pool.forward(obs[A2], member_params, plan, out=obs[A2][:, :19])
    with pytest.raises(ValueError, match="rows"):
        pool.forward(obs[A2][:500], member_params, plan)
    with pytest.raises(ValueError, match="members"):
        pool.forward(obs[A2], member_params[:3], plan)


def test_snapshots_under_a_captured_graph():
    """Snapshots against net.forward per member; the captured launch replayed after a push(), after an optimizer step on
    member 0, and after a re-plan into the same Plan"""
    from pikazoo_amd import optim, pool

    n, K = 777, 35
    model = a_model(70)
    league = pool.Snapshots(model, 3)
    assert len(league) == 1
    for shift in (0.1, -0.2):                                      # two snapshots, the learner moving between them
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
    head = league.act(obs, sides)

    def expected():
        params = league.member_params()
        return {A1: per_member(obs[A1], params, None), A2: per_member(obs[A2], params, members)}

    def judged():
        host = [[cpu(p) for p in ps] for ps in league.member_params()]
        for a, eff in ((A1, None), (A2, cpu(members))):
            ref, tol = PJ.judge(cpu(obs[a]), host, eff, "tanh")
            assert N.worst_share(cpu(head[a]), ref, tol)[0] <= 1, a

    want = expected()
    assert all(torch.equal(head[a], want[a]) for a in obs)
    judged()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        league.act(obs, sides, out=head)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        league.act(obs, sides, out=head)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(head[a], want[a]) for a in obs)
    before = {a: head[a].clone() for a in obs}
    # a push overwrites the oldest snapshot in place: the replay sees it
    assert league.push() == 1 and len(league) == 3
    graph.replay()
    torch.cuda.synchronize()
    want = expected()
    assert torch.equal(head[A2], want[A2]) and not torch.equal(head[A2], before[A2]) and torch.equal(head[A1], before[A1])
    judged()
    # an optimizer step on member 0
    optimizer = optim.Adam(model.parameters(), lr=1e-2)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    optimizer.step()
    graph.replay()
    torch.cuda.synchronize()
    want = expected()
    assert all(torch.equal(head[a], want[a]) for a in obs) and not torch.equal(head[A1], before[A1])
    judged()
    # opponents re-drawn into the same Plan between replays
    members = torch.randint(P, (n,), device="cuda:0", generator=gen)
    assert pool.plan(members, P, out=plan) is plan
    before = head[A2].clone()
    graph.replay()
    torch.cuda.synchronize()
    want = expected()
    assert all(torch.equal(head[a], want[a]) for a in obs) and not torch.equal(head[A2], before)
    judged()


def test_the_league_example_runs():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "examples"))
    import ppo_league

    lines = []
    losses = ppo_league.main(num_envs=256, iters=2, steps=8, snapshot_every=1, log=lines.append)
    assert len(losses) == 2 * 2 * 4 and np.isfinite(losses).all() and len(lines) == 2
    assert "pool 2" in lines[0] and "pool 3" in lines[1]
