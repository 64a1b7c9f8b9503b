"""GPU tests (``-m gpu``) of the policy-net launch (include/pikazoo_net.h: ``pz_mlp_forward``) and of ``pikazoo_amd.net``.

The judge is tests/net_judge.py: the header's definition in numpy float64 with a DERIVED tolerance per output (held to a
torch float64 ``nn.Sequential``, a float32 restatement and six mutants by tests/test_net_host.py).  No GPU result is ever an
expected value.  Every C-ABI launch writes into sentinel-filled outputs with elements in front of the first row, behind
the last one and in the pad columns, all of which must keep the sentinel; the pad columns of the observations and the
memory behind their last row hold NaN patterns (for the integer formats: a huge value), which must not reach any output.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import capture_net_bits as B
import net_judge as N
import policy_judge as J
from test_gpu_policy import SENT, TAIL, cpu, stream

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
NP_OBS = {"int32": np.int32, "int16": np.int16, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
TORCH_OBS = {"int32": torch.int32, "int16": torch.int16, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
N_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 4099)
SIZES = ((35, 64, 19), (35, 32, 19), (35, 128, 19), (1, 32, 1), (36, 64, 33), (72, 128, 40))


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import net

    return net.load()


def obs_bits(values, dtype):
    """the element patterns a device buffer of `dtype` holds for observation values representable in it"""
    if dtype in ("int32", "int16"):
        return np.asarray(values).astype(NP_OBS[dtype])
    return J.logit_bits(np.asarray(values, np.float32), dtype)


def device_obs(values, dtype, pitch, offset):
    """[n, K] observations -> (a flat device tensor holding them at `pitch` from row to row, `offset` elements in, the poison
    pattern everywhere else -- NaN for the float formats, the format's most negative value for the integer ones --, the
    address of the first row)"""
    n, K = values.shape
    bits = obs_bits(values, dtype)
    flat = np.empty(offset + n * pitch + TAIL, bits.dtype)
    flat[:] = np.iinfo(bits.dtype).min if dtype in ("int32", "int16") else J.logit_bits(np.array([np.nan], np.float32), dtype)[0]
    flat[offset:offset + n * pitch].reshape(n, pitch)[:, :K] = bits
    host = flat.view(np.int16) if flat.dtype == np.uint16 else flat
    t = torch.from_numpy(host).to("cuda:0")
    return t, t.data_ptr() + offset * flat.itemsize


def device_params(params, offset=0):
    """six float32 device tensors with `offset` NaN elements in front and a NaN tail: (the tensors, their addresses)"""
    ts, ptrs = [], []
    for p in params:
        host = np.full(offset + p.size + TAIL, np.nan, np.float32)
        host[offset:offset + p.size] = np.asarray(p, np.float32).ravel()
        t = torch.from_numpy(host).to("cuda:0")
        ts.append(t)
        ptrs.append(t.data_ptr() + 4 * offset)
    return ts, ptrs


def run_forward(lib, obs, obs_dtype, params, activation, out_dtype="float32", obs_pitch=None, out_pitch=None, offset=0, shared=False,
                expect=0):
    """pz_mlp_forward on one or two agents' observations (`obs`: a list of [n, K] arrays; `params`: a list of parameter
    sets, one per agent -- or one set with `shared`, whose pointers both agents then get): per side the [n, O] outputs as
    float32 values (a float64-exact view of what the device wrote), every buffer checked for what must not have been written"""
    sides = len(obs)
    n, K = obs[0].shape
    H, O = params[0][0].shape[0], params[0][4].shape[0]
    obs_pitch, out_pitch = obs_pitch or K, out_pitch or O
    xs = [device_obs(x, obs_dtype, obs_pitch, offset) for x in obs]
    sets = [device_params(p, offset) for p in params]
    if shared:
        sets = [sets[0]] * sides
    osize = 4 if out_dtype == "float32" else 2
    outs = [torch.full((offset + n * out_pitch + TAIL,), SENT, dtype=torch.int32 if osize == 4 else torch.int16, device="cuda:0") for _ in obs]
    optr = [o.data_ptr() + offset * osize for o in outs]
    second = sides == 2
    err = lib.pz_mlp_forward(xs[0][1], xs[1][1] if second else None, N.OBS_DTYPES.index(obs_dtype), n, K, obs_pitch, H, O,
                             N.ACTIVATIONS.index(activation), *sets[0][1], *(sets[1][1] if second else [None] * 6), optr[0],
                             optr[1] if second else None, N.OUT_DTYPES.index(out_dtype), out_pitch, stream())
    assert err == expect
    torch.cuda.synchronize()
    results = []
    for o in outs:
        flat = cpu(o)
        rows = flat[offset:offset + n * out_pitch].reshape(n, out_pitch)
        assert (flat[:offset] == SENT).all() and (flat[offset + n * out_pitch:] == SENT).all(), "an output outside its rows"
        assert (rows[:, O:] == SENT).all(), "a pad column of the output was written"
        bits = np.ascontiguousarray(rows[:, :O])
        results.append(J.bits_to_float(bits.view(np.float32 if osize == 4 else (np.float16 if out_dtype == "float16" else np.uint16)), out_dtype))
    return results


def check(have, obs, params, activation, out_dtype="float32", what=""):
    ref, tol = N.judge(obs, params, activation, out_dtype)
    worst, rows = N.worst_share(have, ref, tol)
    print(f"{what}: worst error / tolerance {worst:.4f}")
    assert worst <= 1, (what, worst, rows)
    return worst


@pytest.mark.parametrize("n", N_EDGES)
def test_batch_sizes(lib, n):
    """every tile edge, one-wave and many-wave workgroups, several workgroups: two agents with nets of their own"""
    K, H, O = SIZES[0]
    params = [N.make_params(K, H, O, seed) for seed in (1, 2)]
    obs = [N.make_obs(n, K, "float32", seed) for seed in (3, 4)]
    have = run_forward(lib, obs, "float32", params, "tanh")
    for s in (0, 1):
        check(have[s], obs[s], params[s], "tanh", what=f"n={n} side {s}")


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", SIZES)
def test_layer_sizes(lib, K, H, O, activation):
    """... at pitches above the widths and a base offset of one element, one agent and two agents on the same pointers"""
    n = 129
    params = [N.make_params(K, H, O, 5)]
    obs = [N.make_obs(n, K, "float32", seed) for seed in (6, 7)]
    one = run_forward(lib, obs[:1], "float32", params, activation, obs_pitch=K + 3, out_pitch=O + 2, offset=1)
    two = run_forward(lib, obs, "float32", params, activation, obs_pitch=K + 3, out_pitch=O + 2, offset=1, shared=True)
    check(one[0], obs[0], params[0], activation, what=f"{K}-{H}-{O} {activation} one agent")
    for s in (0, 1):
        check(two[s], obs[s], params[0], activation, what=f"{K}-{H}-{O} {activation} shared side {s}")
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)), "a row's bits changed with the other agent present"


@pytest.mark.parametrize("out_dtype", N.OUT_DTYPES)
@pytest.mark.parametrize("obs_dtype", N.OBS_DTYPES)
def test_formats(lib, obs_dtype, out_dtype):
    """all five observation formats into all three output formats, both activations; a 16-bit base offset by one element"""
    K, H, O = SIZES[0]
    n = 65
    params = [N.make_params(K, H, O, seed) for seed in (8, 9)]
    obs = [N.make_obs(n, K, obs_dtype, seed) for seed in (10, 11)]
    for activation, pitches in (("tanh", dict(obs_pitch=K + 1, out_pitch=O + 1, offset=1)), ("relu", {})):
        have = run_forward(lib, obs, obs_dtype, params, activation, out_dtype, **pitches)
        for s in (0, 1):
            check(have[s], obs[s], params[s], activation, out_dtype, what=f"{obs_dtype} -> {out_dtype} {activation} side {s}")


def test_int32_beyond_2_to_24_rounds_to_nearest_even(lib):
    K, H, O = 4, 32, 3
    obs = np.array([[2 ** 24 + 1, -(2 ** 24 + 3), 2 ** 30 + 65, 7]] * 3, np.int32)
    params = N.make_params(K, H, O, 12)
    params[0] = (params[0] * np.float32(2.0 ** -30)).astype(np.float32)
    have = run_forward(lib, [obs], "int32", [params], "tanh")[0]
    check(have, obs, params, "tanh", what="int32 beyond 2^24")
    # the definition's own conversion: as if the observation had been the rounded float32
    exact = run_forward(lib, [obs.astype(np.float32)], "float32", [params], "tanh")[0]
    assert np.array_equal(have.view(np.uint32), exact.view(np.uint32))


def test_exact_integer_layout_pin(lib):
    """Small-integer observations and asymmetric small-integer weights under relu: every float32 sum is exact, so the output
    must EQUAL the integer result.  A wrong operand map or a wrong k permutation of any layer cannot pass."""
    for n, K, H, O in ((65, 35, 64, 19), (65, 36, 128, 33), (33, 9, 32, 5)):
        x, params, want = N.integer_case(n, K, H, O)
        for dtype in ("int32", "float32"):
            have = run_forward(lib, [x], dtype, [params], "relu", obs_pitch=K + 2)[0]
            assert np.array_equal(have.astype(np.int64), want) and np.isfinite(have).all(), (n, K, H, O, dtype)


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
def test_nan_containment(lib, activation):
    """A row with a NaN gives NaN in every output; a row with an inf gives what the definition gives (NaN or inf, judged as
    such); every other row of their waves stays within its tolerance; the NaN patterns of the pad columns and behind the
    last row change nothing (they are in every launch of this file)."""
    K, H, O = SIZES[0]
    n = 70
    params = [N.make_params(K, H, O, 13)]
    obs = N.make_obs(n, K, "float32", 14)
    obs[5, 17] = np.nan
    obs[40, 0] = np.inf
    obs[69, K - 1] = np.nan
    have = run_forward(lib, [obs], "float32", params, activation, obs_pitch=K + 5)[0]
    assert np.isnan(have[5]).all() and np.isnan(have[69]).all()
    ref, tol = N.judge(obs, params[0], activation)
    clean = np.ones(n, bool)
    clean[[5, 40, 69]] = False
    assert np.isfinite(have[clean]).all()
    worst, _ = N.worst_share(have[clean], ref[clean], tol[clean])
    assert worst <= 1
    # the inf row: tanh saturates (finite outputs, judged); relu carries inf * w: non-finite where the definition's are
    if activation == "tanh":
        assert N.worst_share(have[40:41], ref[40:41], tol[40:41])[0] <= 1
    else:
        assert not np.isfinite(have[40]).any() or np.array_equal(np.isfinite(have[40]), np.isfinite(ref[40]))


def test_bits_do_not_depend_on_the_batch(lib):
    """two calls return equal bits; rows [g0, n) as a shard return the bits of the whole batch's tail; a row's bits do not
    change with the other agent present or absent, nor with the pitches or the output format of another call"""
    K, H, O = SIZES[0]
    n = 200
    params = [N.make_params(K, H, O, seed) for seed in (15, 16)]
    obs = [N.make_obs(n, K, "float32", seed) for seed in (17, 18)]
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    whole = run_forward(lib, obs, "float32", params, "tanh")
    again = run_forward(lib, obs, "float32", params, "tanh")
    for s in (0, 1):
        assert np.array_equal(bits(whole[s]), bits(again[s]))
    for g0 in (1, 31, 32, 64):
        shard = run_forward(lib, [x[g0:] for x in obs], "float32", params, "tanh")
        for s in (0, 1):
            assert np.array_equal(bits(shard[s]), bits(whole[s][g0:])), (g0, s)
    for s in (0, 1):
        alone = run_forward(lib, [obs[s]], "float32", [params[s]], "tanh", obs_pitch=K + 7, out_pitch=O + 3, offset=1)
        assert np.array_equal(bits(alone[0]), bits(whole[s])), s
    swapped = run_forward(lib, obs[::-1], "float32", params[::-1], "tanh")
    assert np.array_equal(bits(swapped[1]), bits(whole[0])) and np.array_equal(bits(swapped[0]), bits(whole[1]))
    single = run_forward(lib, [obs[0][77:78]], "float32", [params[0]], "tanh")
    assert np.array_equal(bits(single[0]), bits(whole[0][77:78]))


def rows_past_the_first_tile():
    """(compute units, n): the rule is pz_mlp_tile.hpp's grid cap -- at most two resident workgroups per compute unit, so no
    launch has more than 2 CUs workgroups of four 32-row tiles, 2 CUs * 128 rows a trip of the tile loop.  Twice that, one
    more workgroup's worth and 37 rows: every wave takes at least two tiles at every hidden width and either agent count
    (a smaller cap only adds trips), the workgroups' tile counts differ, and the last tile has 5 live rows."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, 2 * (2 * cus) * 128 + 128 + 37


LARGE_SIZES = {32: (35, 32, 19), 64: (35, 64, 19), 128: (72, 128, 40)}


@pytest.mark.parametrize("H", sorted(LARGE_SIZES))
def test_every_wave_past_its_first_tile(lib, H):
    """one agent and two agents on nets of their own at a batch beyond what the capped grid covers in one trip: every row
    within the float64 judge's tolerance; three shards of 4096 rows -- the head, a span that starts behind the widest
    first trip, the tail -- launched alone return the bits of the same rows of the whole launch"""
    K, _, O = LARGE_SIZES[H]
    cus, n = rows_past_the_first_tile()
    print(f"{cus} compute units: n = {n}")
    acts = ("tanh", "relu") if H != 64 else ("relu", "tanh")         # (both activations at both agent counts over the three H)
    params = [N.make_params(K, H, O, seed) for seed in (24, 25)]
    obs = [N.make_obs(n, K, "float32", seed) for seed in (26, 27)]
    pitches = dict(obs_pitch=K + 3, out_pitch=O + 2, offset=1)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    spans = (0, 2 * cus * 128 + 33, n - 4096)
    for sides, activation in zip((1, 2), acts):
        whole = run_forward(lib, obs[:sides], "float32", params[:sides], activation, **pitches)
        for s in range(sides):
            check(whole[s], obs[s], params[s], activation, what=f"H = {H} n = {n} {activation} {sides} agent(s) side {s}")
        for g0 in spans:
            shard = run_forward(lib, [x[g0:g0 + 4096] for x in obs[:sides]], "float32", params[:sides], activation, **pitches)
            for s in range(sides):
                assert np.array_equal(bits(shard[s]), bits(whole[s][g0:g0 + 4096])), (H, sides, g0, s)


@pytest.mark.parametrize("H", sorted(LARGE_SIZES))
def test_exact_integers_past_the_first_tile(lib, H):
    """the integer case at the same n: every row of every trip of the tile loop EQUALS the integer result"""
    K, _, O = LARGE_SIZES[H]
    cus, n = rows_past_the_first_tile()
    print(f"{cus} compute units: n = {n}")
    x, params, want = N.integer_case(n, K, H, O)
    for dtype in ("int32", "float32"):
        have = run_forward(lib, [x], dtype, [params], "relu", obs_pitch=K + 2)[0]
        assert np.isfinite(have).all() and np.array_equal(have.astype(np.int64), want), (H, dtype)


def test_bits_are_the_recorded_ones(lib):
    """tests/golden/net_forward_bits.json (tests/capture_net_bits.py) holds digests of what pz_mlp_forward wrote, taken from
    the library before its tile moved into csrc/pz_mlp_tile.hpp: every case must give those bits.  Every other test here
    allows a tolerance, and the pool's comparisons hold the tile to itself.  No skip on another compiler: tanhf comes from the
    toolchain, and a toolchain change is a reason to look."""
    import json

    record = json.loads(B.PATH.read_text())
    have = B.digests(lib, run_forward, obs_bits)
    assert list(have) == list(record["cases"]), "the cases are not the recorded ones"
    inputs = [name for name in have if have[name]["inputs"] != record["cases"][name]["inputs"]]
    moved = [name for name in have if have[name]["outputs"] != record["cases"][name]["outputs"]]
    if inputs or moved:
        print(f"recorded compiler: {record['compiler']}\ncurrent compiler:  {B.compiler_line()}")
    assert not inputs, f"the INPUTS differ from the recorded ones (net_judge.make_obs / make_params changed?): {inputs}"
    assert not moved, f"pz_mlp_forward no longer writes the recorded bits (recorded from build {record['build_id']}): {moved}"


def test_zero_rows_launch_nothing(lib):
    K, H, O = SIZES[0]
    run_forward(lib, [np.zeros((0, K), np.float32)], "float32", [N.make_params(K, H, O, 1)], "tanh")


# ---- pikazoo_amd.net -------------------------------------------------------------------------------------------------------
def module_params(model):
    return [cpu(p) for p in model.parameter_tensors()]


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
def test_forward_and_act_agree_with_the_module(activation):
    from pikazoo_amd import net

    torch.manual_seed(3)
    model = net.ActorCritic(activation=activation).to("cuda:0")
    with torch.no_grad():
        for p in model.parameters():  # (biases away from 0, the head's weights away from the 0.01 gain)
            p.add_(torch.empty_like(p).uniform_(-0.2, 0.2))
    n, K = 300, 35
    wide = {a: torch.from_numpy(N.make_obs(n, K + 1, "float32", seed)).to("cuda:0") for a, seed in ((A1, 20), (A2, 21))}
    for a in wide:
        wide[a][:, K] = float("nan")
    obs = {a: w[:, :K] for a, w in wide.items()}  # row stride K + 1
    head = model.act(obs)
    again = model.act(obs, out=head)
    assert all(again[a].data_ptr() == head[a].data_ptr() and tuple(head[a].shape) == (n, 19) and not head[a].requires_grad for a in obs)
    params = module_params(model)
    for a in obs:
        ref, tol = N.judge(cpu(obs[a]), params, activation)
        assert N.worst_share(cpu(head[a]), ref, tol)[0] <= 1
        torch_route = model(obs[a])
        assert torch_route.requires_grad
        # the two routes stand within the sum of their tolerances (torch's float32 route obeys the same bound: it holds for
        # every summation order)
        assert (np.abs(cpu(torch_route).astype(np.float64) - cpu(head[a])) <= 2 * tol).all()
    one = net.forward(obs[A1], model.parameter_tensors(), activation)
    assert torch.equal(one, head[A1])
    sep = net.forward(obs, {a: model.parameter_tensors() for a in obs}, activation, out_dtype=torch.bfloat16)
    assert sep[A2].dtype == torch.bfloat16
    ref, tol = N.judge(cpu(obs[A2]), params, activation, "bfloat16")
    assert N.worst_share(cpu(sep[A2].float()), ref, tol)[0] <= 1
    for dtype in (torch.int32, torch.int16, torch.float16, torch.bfloat16):
        raw = {a: (o * 400).to(dtype) for a, o in obs.items()}
        got = model.act(raw)
        ref, tol = N.judge(cpu(raw[A1].float() if dtype in (torch.float16, torch.bfloat16) else raw[A1]), params, activation)
        assert N.worst_share(cpu(got[A1]), ref, tol)[0] <= 1, dtype
    with pytest.raises(ValueError, match="overlaps"):
        net.forward(obs[A1], model.parameter_tensors(), activation, out=wide[A1][:, :19])


def test_a_captured_graph_sees_an_in_place_change_of_the_parameters():
    from pikazoo_amd import net

    torch.manual_seed(4)
    model = net.ActorCritic().to("cuda:0")
    obs = {a: torch.from_numpy(N.make_obs(257, 35, "float32", seed)).to("cuda:0") for a, seed in ((A1, 22), (A2, 23))}
    head = model.act(obs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.act(obs, out=head)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model.act(obs, out=head)
    graph.replay()
    torch.cuda.synchronize()
    before = {a: head[a].clone() for a in obs}
    assert all(torch.equal(before[a], model.act(obs)[a]) for a in obs)
    with torch.no_grad():
        model.fc2.weight.mul_(0.5).add_(0.01)
        model.head.bias.add_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    fresh = model.act(obs)
    params = module_params(model)
    for a in obs:
        assert torch.equal(head[a], fresh[a]) and not torch.equal(head[a], before[a])
        ref, tol = N.judge(cpu(obs[a]), params, "tanh")
        assert N.worst_share(cpu(head[a]), ref, tol)[0] <= 1


def test_chain_act_sample_step_and_the_loss_on_the_sampled_batch():
    """act -> policy.sample on head[:, :18] at pitch 19 -> env.step, two steps at 256 games; then ppo.loss on the torch
    route's head of the same observations: the ratio is 1 up to the two routes' roundoff, so approx_kl is 0 up to a bound
    DERIVED here.  With delta the largest distance of the two routes' logits (each within the judge's tolerance of the
    real value: delta <= 2 max tol) and lam the largest tolerance of a log-probability (policy_judge), the log-ratio
    obeys |d| <= 2 delta + 2 lam =: D (a log-softmax moves by at most twice the largest move of a logit).  Then
    kl = (exp(d) - 1) - d <= D^2 (for D < 1), computed in float32 from r = exp(d) (3 ulp of a value near 1), r - 1 (exact,
    Sterbenz) and one more subtraction: an absolute error of at most (2 * 3 + 1) U (1 + D) per row, and so of the mean."""
    from pikazoo_amd import net, pikazoo_v0, policy, ppo
    from pikazoo_amd.wrappers import NormalizeObservation

    torch.manual_seed(5)
    n, A = 256, 18
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device="cuda:0", seed=9))
    model = net.ActorCritic(in_features=35, hidden=64, num_actions=A).to("cuda:0")
    with torch.no_grad():
        model.head.weight.mul_(5.0)  # (logits of some spread: the 0.01 gain alone gives a uniform policy)
    obs, _ = env.reset()
    agents = env.agents
    for t in range(2):
        seen = {a: obs[a].clone() for a in agents}
        head = model.act(seen)
        picked = policy.sample({a: head[a][:, :A] for a in agents}, seed=9, step=t)
        assert all(head[a][:, :A].stride(0) == A + 1 for a in agents)
        obs, rewards, terminations, _, _ = env.step(picked["actions"])
    params = module_params(model)
    bound = 0.0
    for a in agents:
        ref, tol = N.judge(cpu(seen[a]), params, "tanh")
        st = J.stats(ref[:, :A])
        _, lam = J.log_prob(st, cpu(picked["actions"][a]))
        D = 2 * (2 * tol[:, :A].max()) + 2 * lam.max()
        bound = max(bound, D * D + (2 * J.EXP_ULP + 1) * J.U * (1 + D))
    assert bound <= 1e-5, bound
    gen = torch.Generator(device="cuda:0").manual_seed(6)
    noise = lambda: {a: torch.randn(n, device="cuda:0", generator=gen) for a in agents}  # noqa: E731
    loss, stats = ppo.loss(head={a: model(seen[a]) for a in agents}, num_actions=A, actions=picked["actions"],
                           old_log_probs=picked["log_probs"], advantages=noise(), returns=noise())
    for a in agents:
        kl = float(stats["approx_kl"][a])
        print(f"{a}: approx_kl {kl:.3e}, derived bound {bound:.3e}")
        assert abs(kl) <= bound
        assert float(stats["clip_fraction"][a]) == 0.0 and np.isfinite(float(loss[a].detach()))
    sum(loss.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_the_example_runs():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "examples"))
    import ppo_selfplay

    lines = []
    losses = ppo_selfplay.main(num_envs=256, iters=2, steps=8, log=lines.append)
    assert len(losses) == 2 * 2 * 4 and np.isfinite(losses).all() and len(lines) == 2
