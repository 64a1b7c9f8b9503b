"""GPU tests of the policy-net backward (include/pikazoo_netgrad.h) against tests/netgrad_judge.py: the header's definition
in float64 with a derived per-element tolerance (held to torch float64 autograd, a float32 restatement and seven mutants by
tests/test_netgrad_host.py).  Gradient outputs are sentinel-filled with guard elements in front and behind, the pads of obs and
grad_head and the surroundings of the parameters are NaN, the workspace is NaN with a sentinel tail that must survive.  Every
test prints its worst error / tolerance."""
import sys
from pathlib import Path

import numpy as np
import pytest

import net_judge as N
import netgrad_judge as G
from test_netgrad_host import GPU_BATCHES, GPU_LAYERS, GPU_SEED, LARGE_LAYERS, large_cases, large_n

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
DEV = "cuda"
GUARD, SENTINEL = 8, -12345.0
TORCH = {"int32": torch.int32, "int16": torch.int16, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def ng():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    from pikazoo_amd import netgrad

    netgrad.load()
    return netgrad


def rows_tensor(values, dtype, pitch, offset):
    """[n, width] `values` of numpy format `dtype` as a view at row stride `pitch`, `offset` elements into a NaN-filled (for
    integers: a large-negative-filled) buffer"""
    n, width = values.shape
    t = torch.from_numpy(np.ascontiguousarray(values.astype(np.float32) if dtype == "bfloat16" else values)).to(DEV).to(TORCH[dtype])
    poison = float("nan") if TORCH[dtype].is_floating_point else -30000
    buf = torch.full((offset + n * pitch + 3,), poison, dtype=TORCH[dtype], device=DEV)
    view = buf[offset:offset + n * pitch].view(n, pitch)[:, :width]
    view.copy_(t)
    return view


def param_tensor(p):
    buf = torch.full((p.size + 2,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[1:1 + p.size].view(p.shape)
    view.copy_(torch.from_numpy(p))
    return view


def guarded(shape):
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + size].view(shape)


def per_side(params, sides):
    """one parameter set for all sides, or a list of one set per side -> a list of one set per side"""
    return list(params) if isinstance(params[0], (list, tuple)) else [params] * len(sides)


def call(ng, sides, params, activation, shared, obs_dtype="float32", grad_dtype="float32", pitches=(3, 2), offset=1, ws_fill=float("nan")):
    """pz_mlp_backward through the C ABI on guarded buffers: [six numpy gradients] per output group.  `params` is one set (both
    agents then pass the SAME six pointers) or a list of one set per agent (each in device tensors of its own)."""
    lib = ng.load()
    n, K = sides[0][0].shape
    O = sides[0][1].shape[1]
    sets = per_side(params, sides)
    assert not shared or sets[0] is sets[-1]
    H = sets[0][0].shape[0]
    xs = [rows_tensor(x, obs_dtype, K + pitches[0], offset) for x, _ in sides]
    gs = [rows_tensor(g, grad_dtype, O + pitches[1], offset) for _, g in sides]
    P = [param_tensor(p) for p in sets[0]]
    P2 = P if sets[-1] is sets[0] else [param_tensor(p) for p in sets[-1]]
    groups = 1 if shared or len(sides) == 1 else 2
    outs = [[guarded(p.shape) for p in sets[0]] for _ in range(groups)]
    need = lib.pz_mlp_backward_workspace_bytes(n, K, H, O)
    assert need == ng.workspace_bytes(n, K, H, O, DEV) and need > 0 and need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), ws_fill, dtype=torch.float32, device=DEV)
    ws[need // 4:] = SENTINEL
    two = len(sides) == 2
    ptr = lambda t: t.data_ptr()  # noqa: E731
    code = lib.pz_mlp_backward(
        ptr(xs[0]), ptr(xs[1]) if two else None, N.OBS_DTYPES.index(obs_dtype), n, K, K + pitches[0], H, O, N.ACTIVATIONS.index(activation),
        *[ptr(p) for p in P], *([ptr(p) for p in P2] if two else [None] * 6), ptr(gs[0]), ptr(gs[1]) if two else None,
        G.GRAD_DTYPES.index(grad_dtype), O + pitches[1], *[ptr(v) for _, v in outs[0]],
        *([ptr(v) for _, v in outs[1]] if groups == 2 else [None] * 6), ptr(ws), None)
    torch.cuda.synchronize()
    assert code == 0
    assert (ws[need // 4:] == SENTINEL).all(), "the workspace's tail was written"
    result = []
    for group in outs:
        for buf, view in group:
            assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a guard element was written"
        result.append([view.cpu().numpy().copy() for _, view in group])
    return result


def judged(result, sides_list, params, activation, what):
    """each output group against the judge on its own rows and its own parameter set"""
    worst = 0.0
    for got, sides, own in zip(result, sides_list, per_side(params, sides_list)):
        refs, tols, ambiguous = G.judge(sides, own, activation)
        assert ambiguous == 0
        share, beyond = G.worst_share(got, refs, tols)
        assert not beyond, (what, share, beyond)
        worst = max(worst, share)
    print(f"{what}: worst error / tolerance {worst:.4f}")
    return worst


@pytest.mark.parametrize("n", GPU_BATCHES)
def test_batch_sizes_two_agents_with_separate_nets(ng, n):
    """each agent on a net of its own, judged against its own parameters: a launch that read agent 1's weights for agent 2
    fails every case"""
    for activation in N.ACTIVATIONS:
        sides, sets = G.make_case(n, 35, 64, 19, activation, GPU_SEED, agents=2, nets=2)
        out = call(ng, sides, sets, activation, shared=False)
        judged(out, [[sides[0]], [sides[1]]], sets, activation, f"n = {n} {activation}")
        if n == 33:  # the judge tells the two nets apart: agent 2's result is far from the judge under agent 1's parameters
            refs, tols, _ = G.judge([sides[1]], sets[0], activation)
            assert G.worst_share(out[1], refs, tols)[0] > 100


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", GPU_LAYERS)
def test_layer_sizes_one_agent_and_a_shared_net(ng, K, H, O, activation):
    sides, params = G.make_case(129, K, H, O, activation, GPU_SEED, agents=2)
    one = call(ng, sides[:1], params, activation, shared=False)
    judged(one, [[sides[0]]], params, activation, f"{K}-{H}-{O} {activation} one agent")
    both = call(ng, sides, params, activation, shared=True)
    judged(both, [sides], params, activation, f"{K}-{H}-{O} {activation} shared")


@pytest.mark.parametrize("grad_dtype", G.GRAD_DTYPES)
@pytest.mark.parametrize("obs_dtype", N.OBS_DTYPES)
def test_formats(ng, obs_dtype, grad_dtype):
    sides, params = G.make_case(65, 35, 64, 19, "tanh", GPU_SEED, agents=2, obs_dtype=obs_dtype, grad_dtype=grad_dtype)
    out = call(ng, sides, params, "tanh", shared=False, obs_dtype=obs_dtype, grad_dtype=grad_dtype)
    judged(out, [[sides[0]], [sides[1]]], params, "tanh", f"{obs_dtype} x {grad_dtype}")


def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n,K,H,O,small", [(65, 35, 64, 19, False), (65, 36, 128, 33, False), (33, 9, 32, 5, False), (0, 35, 64, 19, True),
                                           (0, 35, 32, 19, True), (0, 35, 128, 19, True)])
def test_exact_integer_pin(ng, n, K, H, O, small):
    """every intermediate and every partial sum is an exact float32: the result EQUALS the int64 one, units at z == 0
    included.  The last cases take their n from the grid cap: every workgroup runs two passes and a part of a third."""
    if n == 0:
        cap = compute_units()
        n = 2 * cap * ng.rows_per_pass(H) + 65
        print(f"{cap} compute units: n = {n}")
    x, params, d3, want = G.integer_case(n, K, H, O, small=small)
    for dtype in ("int32", "float32"):
        got = call(ng, [(x.astype(dtype), d3.astype(np.float32))], params, "relu", shared=False, obs_dtype=dtype)[0]
        for name, g, w in zip(G.NAMES, got, want):
            assert np.array_equal(g.astype(np.int64), w), (name, dtype)
    print(f"integer case n = {n}: equal")


@pytest.mark.parametrize("shared", (False, True), ids=("two_nets", "shared_net"))
def test_exact_integer_pin_two_agents_past_the_first_pass(ng, shared):
    """H = 64 at the cap-sized n with both agents: on nets of their own each result EQUALS its own int64 one; on a shared net
    the result EQUALS the int64 sum over the rows of both sides (one integer case of 2 n rows, cut in halves: its own
    assertions keep every partial sum of the whole below 2^24)."""
    K, H, O = 35, 64, 19
    cap = compute_units()
    n = 2 * cap * ng.rows_per_pass(H) + 65
    print(f"{cap} compute units: n = {n} per agent")
    f = lambda x, d3: (x.astype(np.int32), d3.astype(np.float32))  # noqa: E731
    if shared:
        x, params, d3, want = G.integer_case(2 * n, K, H, O, small=True)
        got = call(ng, [f(x[:n], d3[:n]), f(x[n:], d3[n:])], params, "relu", shared=True, obs_dtype="int32")
        wants = [want]
    else:
        cases = [G.integer_case(n, K, H, O, seed=seed, small=True) for seed in (5, 6)]
        assert not np.array_equal(cases[0][1][0], cases[1][1][0])
        got = call(ng, [f(c[0], c[2]) for c in cases], [c[1] for c in cases], "relu", shared=False, obs_dtype="int32")
        wants = [c[3] for c in cases]
    assert len(got) == len(wants)
    for group, want in zip(got, wants):
        for name, g, w in zip(G.NAMES, group, want):
            assert np.array_equal(g.astype(np.int64), w), name
    print(f"integer case n = {n}, two agents, {'a shared net' if shared else 'two nets'}: equal")


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("hidden", sorted(LARGE_LAYERS))
def test_past_the_first_pass_under_the_documented_roundings(ng, hidden, activation):
    """n = CUs * R + R + 33: workgroup 0 takes a second, whole pass, workgroup 1 a partial one, the others none.  One agent,
    two nets and a shared net, judged with the header's own count of roundings -- (rows of a workgroup) + (workgroups - 1) +
    (1 for a shared net) -- in the sums over the rows, not with n: under n a lost pass can stay inside the tolerance
    (tests/test_netgrad_host.py shows both)."""
    cus = compute_units()
    n = large_n(hidden, cus)
    print(f"{cus} compute units: n = {n}")
    for what, sides, params, shared, groups in large_cases(hidden, activation, cus):
        m = G.documented_roundings(n, hidden, cus, shared)
        out = call(ng, sides, params, activation, shared=shared)
        assert len(out) == len(groups)
        worst = 0.0
        for got, (own, own_params) in zip(out, groups):
            refs, tols, ambiguous = G.judge(own, own_params, activation, roundings=m)
            assert ambiguous == 0
            share, beyond = G.worst_share(got, refs, tols)
            assert not beyond, (what, share, beyond)
            worst = max(worst, share)
        print(f"H = {hidden} {activation} n = {n} {what}, {m} roundings: worst error / tolerance {worst:.4f}")


def test_nan_containment(ng):
    """a NaN in grad_head[row, c] reaches db3[c], dW3[c, :] and every gradient of layers 1 and 2, nothing else; a NaN
    observation reaches what the header's definition says it reaches (see below: not db3, and under relu not the biases)"""
    for activation in N.ACTIVATIONS:
        sides, params = G.make_case(65, 35, 64, 19, activation, GPU_SEED)
        x, g = sides[0]
        g2 = g.copy()
        g2[40, 3] = np.nan
        got = call(ng, [(x, g2)], params, activation, shared=False)[0]
        refs, tols, _ = G.judge([(x, g2)], params, activation)
        assert all(np.isnan(t).all() for t in got[:4]) and np.isnan(got[4][3]).all() and np.isnan(got[5][3])
        keep = np.arange(19) != 3
        share, beyond = G.worst_share([got[4][keep], got[5][keep]], [refs[4][keep], refs[5][keep]], [tols[4][keep], tols[5][keep]])
        assert np.isfinite(got[4][keep]).all() and np.isfinite(got[5][keep]).all() and share <= 1
        x2 = x.copy()
        x2[7, 5] = np.nan
        got = call(ng, [(x2, g)], params, activation, shared=False)[0]
        # the definition decides what a NaN observation reaches: db3 = sum d3 never sees it; under tanh everything else is NaN;
        # under relu "a NaN z passes the gradient on" (factor 1), so d2 and d1 of that row stay finite: dW3, dW2 and column 5
        # of dW1 are NaN, the bias gradients are not.  The NaN pattern must be the judge's, element for element.
        refs, _, _ = G.judge([(x2, g)], params, activation)
        for name, t, r in zip(G.NAMES, got, refs):
            assert np.array_equal(np.isnan(t), np.isnan(r)), (activation, name)
        assert np.isnan(got[4]).all() and np.isnan(got[2]).all() and np.isnan(got[0][:, 5]).all() and np.isfinite(got[5]).all()
        if activation == "tanh":
            assert all(np.isnan(t).all() for t in got[:5])
        print(f"NaN containment {activation}: worst error / tolerance of the untouched rows {share:.4f}")


def test_bit_equality(ng):
    sides, sets = G.make_case(257, 35, 64, 19, "tanh", GPU_SEED, agents=2, nets=2)
    base = call(ng, sides, sets, "tanh", shared=False)
    again = call(ng, sides, sets, "tanh", shared=False, ws_fill=0.0)
    moved = call(ng, sides, sets, "tanh", shared=False, pitches=(13, 1), offset=3)
    alone = call(ng, sides[:1], sets[0], "tanh", shared=False)
    swapped = call(ng, sides[::-1], sets[::-1], "tanh", shared=False)  # (agent 2's net and rows in agent 1's place)
    for a, b in zip(base[0] + base[1], swapped[1] + swapped[0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for other in (again, moved):
        for a, b in zip(base[0] + base[1], other[0] + other[1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(base[0], alone[0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    print("bit equality: two calls, NaN and zero workspace, other pitches and offsets, with and without agent 2")


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
def test_backward_with_a_parameter_set_per_agent(ng, activation):
    """netgrad.backward(obs, {a: P1, b: P2}, ...): two distinct sets through the binding, each agent's gradients judged against
    its own set; and the same sets with shared=False on one sequence per agent"""
    sides, sets = G.make_case(65, 35, 64, 19, activation, GPU_SEED + 3, agents=2, nets=2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    obs = {k: dev(x) for k, (x, _) in zip("ab", sides)}
    gh = {k: dev(g) for k, (_, g) in zip("ab", sides)}
    P = {k: [dev(p) for p in ps] for k, ps in zip("ab", sets)}
    out = ng.backward(obs, P, gh, activation)
    assert list(out) == ["a", "b"] and all(len(v) == 6 for v in out.values())
    worst = judged([[t.cpu().numpy() for t in out[k]] for k in "ab"], [[sides[0]], [sides[1]]], sets, activation,
                   f"a parameter set per agent, {activation}")
    assert worst > 0
    with pytest.raises(ValueError):
        ng.backward(obs, P, gh, activation, shared=True)


def test_zero_rows_write_nothing(ng):
    lib = ng.load()
    params = N.make_params(35, 64, 19, 1)
    P = [param_tensor(p) for p in params]
    outs = [guarded(p.shape) for p in params]
    x = torch.zeros(4, 35, device=DEV)
    g = torch.zeros(4, 19, device=DEV)
    ws = torch.zeros(64, device=DEV)
    code = lib.pz_mlp_backward(x.data_ptr(), None, 2, 0, 35, 35, 64, 19, 0, *[p.data_ptr() for p in P], *[None] * 6, g.data_ptr(), None, 0, 19,
                               *[v.data_ptr() for _, v in outs], *[None] * 6, ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert code == 0 and all((buf == SENTINEL).all() for buf, _ in outs)
    grads = ng.backward(x[:0], P, g[:0])
    assert all(float(t.abs().max()) == 0 for t in grads)


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
def test_backward_and_evaluate_against_torch_autograd(ng, activation):
    from pikazoo_amd import net

    torch.manual_seed(0)
    model = net.ActorCritic(activation=activation).to(DEV)
    with torch.no_grad():
        for b in (model.fc1.bias, model.fc2.bias, model.head.bias):
            b.uniform_(-0.2, 0.2)
    n = 129
    params = [p.detach().cpu().numpy() for p in model.parameter_tensors()]
    seed = GPU_SEED
    while True:  # (a relu case without an ambiguous unit under THIS module's parameters)
        sides = [(N.make_obs(n, 35, "float32", seed + s), G.make_grad(n, 19, "float32", seed + 5 + s)) for s in range(2)]
        refs, tols, ambiguous = G.judge(sides, params, activation)
        if ambiguous == 0:
            break
        seed += 1000
    obs = {k: torch.from_numpy(x).to(DEV) for k, (x, _) in zip("ab", sides)}
    gh = {k: torch.from_numpy(g).to(DEV) for k, (_, g) in zip("ab", sides)}
    for k in obs:
        model(obs[k]).backward(gh[k])
    want = [p.grad.cpu().numpy() for p in model.parameter_tensors()]
    ws = ng.workspace(n, 35, 64, 19, DEV)
    out = ng.backward(obs, model.parameter_tensors(), gh, activation, workspace=ws)
    out2 = ng.backward(obs, model.parameter_tensors(), gh, activation, out=out, workspace=ws)
    assert [t.data_ptr() for t in out] == [t.data_ptr() for t in out2]
    share, beyond = G.worst_share([t.cpu().numpy() for t in out], refs, tols)
    assert not beyond
    # torch's float32 route is held to the same tolerance, so the two routes differ by at most the sum of the two
    for name, a, b, tol in zip(G.NAMES, out, want, tols):
        assert (np.abs(a.cpu().numpy() - b) <= 2 * tol).all(), name
    model.zero_grad(set_to_none=True)
    head = model.evaluate(obs)
    assert head["a"].requires_grad and tuple(head["b"].shape) == (n, 19)
    assert torch.equal(head["a"].detach(), model.act(obs)["a"])
    torch.autograd.backward([head["a"], head["b"]], [gh["a"], gh["b"]])
    first = [p.grad.clone() for p in model.parameter_tensors()]
    for a, b in zip(first, out):
        assert torch.equal(a, b)
    head = model.evaluate(obs)
    torch.autograd.backward([head["a"], head["b"]], [gh["a"], gh["b"]])
    for p, a in zip(model.parameter_tensors(), first):
        assert torch.equal(p.grad, a + a)  # .grad accumulates
    # an expanded gradient, one agent, and a head whose other agent gets no gradient
    model.zero_grad(set_to_none=True)
    model.evaluate(obs["a"]).sum().backward()
    ones = [t.cpu().numpy() for t in ng.backward(obs["a"], model.parameter_tensors(), torch.ones(n, 19, device=DEV), activation)]
    for p, w in zip(model.parameter_tensors(), ones):
        assert np.array_equal(p.grad.cpu().numpy(), w)
    model.zero_grad(set_to_none=True)
    model.evaluate(obs)["b"].sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameter_tensors())
    print(f"backward / evaluate {activation}: worst error / tolerance {share:.4f}")


def test_captured_graph_sees_a_parameter_change(ng):
    from pikazoo_amd import net, ppo

    torch.manual_seed(1)
    model = net.ActorCritic().to(DEV)
    n, A = 256, 18
    obs = {k: torch.rand(n, 35, device=DEV) for k in "ab"}
    act = {k: torch.randint(0, A, (n,), device=DEV, dtype=torch.int32) for k in "ab"}
    old = {k: torch.full((n,), -2.9, device=DEV) for k in "ab"}
    adv = {k: torch.randn(n, device=DEV) for k in "ab"}
    ret = {k: torch.randn(n, device=DEV) for k in "ab"}
    P = [p.detach() for p in model.parameter_tensors()]
    ws = ng.workspace(n, 35, 64, 19, DEV)

    def update(head=None, loss=None, grads=None):
        head = net.forward(obs, P, out=head)
        loss = ppo.loss_and_grad(actions=act, old_log_probs=old, advantages=adv, returns=ret, head=head, num_actions=A, out=loss)
        grads = ng.backward(obs, P, loss["grad_head"], out=grads, workspace=ws)
        return head, loss, grads

    try:
        head, loss, grads = update()
    except (TypeError, KeyError) as e:
        pytest.fail(f"ppo.loss_and_grad(head=) is not as this test calls it: {e}")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        update(head, loss, grads)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            update(head, loss, grads)
    torch.cuda.current_stream().wait_stream(stream)
    with torch.no_grad():
        model.fc2.weight.mul_(0.5)
        model.head.bias.add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [g.clone() for g in grads]
    _, _, fresh = update()
    torch.cuda.synchronize()
    for a, b in zip(replayed, fresh):
        assert torch.equal(a, b)


def test_the_example_runs_on_both_update_routes():
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    logs = [ppo_selfplay.main(num_envs=256, iters=2, steps=8, native_update=flag, log=lambda line: None) for flag in (True, False)]
    for log in logs:
        assert len(log) == len(logs[0]) > 0 and all(np.isfinite(entry) for entry in log)
