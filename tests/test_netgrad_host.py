"""CPU tests (no GPU needed) of the policy-net backward library: libpikazoo_netgrad.so exports its header's four symbols and
carries the tree's build id, nothing loads it before its first use, its code object holds exactly the kernels named below
without scratch or spilled vector registers, the entry point refuses bad arguments before any launch and in the documented
order, ``pikazoo_amd.netgrad`` raises ``ValueError`` for malformed arguments before it needs the library, and the judge the
GPU tests compare with (tests/netgrad_judge.py) is the definition: equal to torch float64 autograd, wide enough for a float32
restatement in two row orders, and sharp enough that seven mutants fail; and, at batches of more passes than workgroups, with the
header's own count of roundings: wide enough for the restatement in the header's pass order, sharp enough for a lost pass."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import net_judge as N
import netgrad_judge as G
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_mlp_backward", "pz_mlp_backward_workspace_bytes", "pz_netgrad_abi_version", "pz_netgrad_build_id"]
KERNELS = sorted([f"pz_netgrad::mlp_backward_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1)]
                 + ["pz_netgrad::mlp_backward_reduce_kernel"])
CASES = [(35, H, 19) for H in (32, 64, 128)]
# every (n, K, H, O, agents, obs format, grad format) of a non-integer case that tests/test_gpu_netgrad.py draws with G.make_case
GPU_SEED = 11
GPU_BATCHES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 4099)
GPU_LAYERS = ((35, 64, 19), (35, 32, 19), (35, 128, 19), (1, 32, 1), (36, 64, 33), (72, 128, 40))


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.netgrad, the judge's included: none of them runs without the module"""
    from pikazoo_amd import netgrad

    return netgrad


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import netgrad

    return netgrad.load()


def declared_arguments(text, name):
    decl = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert decl, f"{name} is not shown"
    return [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]


def test_netgrad_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, learn, net, netgrad, policy, ppo

    assert header_functions("pikazoo_netgrad.h") == NAMES == sorted(netgrad.SIGNATURES) == dynamic_pz_symbols(pz_build.NETGRAD_LIB)
    assert pz_build.library_id(pz_build.NETGRAD_LIB) == pz_build.source_id() == lib.pz_netgrad_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.NETGRAD_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_netgrad.h") in pz_build.DEPS
    assert lib.pz_netgrad_abi_version() == netgrad.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_netgrad.h").read_text()
    assert "#define PZ_NETGRAD_ABI_VERSION 1" in header
    # no other library holds any of the names, and the older libraries' ABI versions did not move (the diagnostics library carries none
    # of its own: it is compiled against the product's)
    others = (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB, pz_build.PPO_LIB, pz_build.NET_LIB)
    for other in others:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    assert _native.load().pz_abi_version() == 10
    assert learn.load().pz_learn_abi_version() == learn.ABI_VERSION == 1
    assert policy.load().pz_policy_abi_version() == policy.ABI_VERSION == 1
    assert ppo.load().pz_ppo_abi_version() == ppo.ABI_VERSION == 1
    assert net.load().pz_net_abi_version() == net.ABI_VERSION == 1
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_mlp_backward")
    assert len(args) == 39 == len(netgrad.SIGNATURES["pz_mlp_backward"][1])
    assert declared_arguments(doc, "pz_mlp_backward") == args
    assert "pikazoo_netgrad.h" in doc and "libpikazoo_netgrad.so" in doc
    assert tuple(netgrad.GRAD_FORMATS) == tuple(net.OUT_FORMATS) and [str(d).split(".")[-1] for d in netgrad.GRAD_FORMATS] == list(G.GRAD_DTYPES)


def test_importing_the_step_path_learn_policy_ppo_or_net_does_not_load_the_netgrad_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net; "
            "assert 'pikazoo_amd.netgrad' not in sys.modules; m = net.ActorCritic(); "
            "\ntry:\n    m.act(__import__('torch').zeros(4, 35))\nexcept ValueError:\n    pass\n"
            "assert 'pikazoo_amd.netgrad' not in sys.modules; import pikazoo_amd as p; assert 'netgrad' in p.__all__; p.netgrad.backward; "
            "assert 'pikazoo_amd.netgrad' in sys.modules and p.netgrad._lib is None; "
            "assert not any('libpikazoo_netgrad' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_netgrad_library(pz_build):
    """Hidden width and activation are the COMPILE-TIME choices: 3 x 2 backward kernels and the reduction of the partial
    sums, nothing else; the formats are run-time.  None uses scratch or spills a vector register; the LDS is dynamic.  The two
    narrower widths stay within 256 registers, accumulation registers included; hidden 128 within 512."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.NETGRAD_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.NETGRAD_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0, (name, row)
        total = row[".vgpr_count"] + row.get(".agpr_count", 0)
        assert total <= (512 if "<128" in name else 256), (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


FAKE = 4096
BACKWARD = dict(obs_p1=FAKE, obs_p2=FAKE + 64, obs_format=2, n=8, in_features=35, obs_pitch=35, hidden=64, out_features=19, activation=0,
                w1_p1=FAKE, b1_p1=FAKE, w2_p1=FAKE, b2_p1=FAKE, w3_p1=FAKE, b3_p1=FAKE, w1_p2=FAKE, b1_p2=FAKE, w2_p2=FAKE, b2_p2=FAKE,
                w3_p2=FAKE, b3_p2=FAKE, grad_head_p1=FAKE, grad_head_p2=FAKE, grad_format=0, grad_pitch=19, dw1_p1=FAKE, db1_p1=FAKE,
                dw2_p1=FAKE, db2_p1=FAKE, dw3_p1=FAKE, db3_p1=FAKE, dw1_p2=FAKE, db1_p2=FAKE, dw2_p2=FAKE, db2_p2=FAKE, dw3_p2=FAKE,
                db3_p2=FAKE, workspace=FAKE, stream=None)


def test_argument_validation(lib):
    """every check on fake pointers: a call that passes them all has n = 0 and launches nothing"""
    def bwd(**over):
        a = dict(BACKWARD)
        assert not set(over) - set(a)
        a.update(over)
        return lib.pz_mlp_backward(*a.values())

    assert list(BACKWARD) == declared_arguments(re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_netgrad.h").read_text(), flags=re.S),
                                                "pz_mlp_backward")
    inputs2 = ["obs_p2", "w1_p2", "b1_p2", "w2_p2", "b2_p2", "w3_p2", "b3_p2", "grad_head_p2"]
    grads2 = ["dw1_p2", "db1_p2", "dw2_p2", "db2_p2", "dw3_p2", "db3_p2"]
    no_grads2 = {k: None for k in grads2}
    one_agent = {k: None for k in inputs2 + grads2}
    assert bwd(n=0) == 0 and bwd(n=0, **one_agent) == 0 and bwd(n=0, **no_grads2) == 0
    # NULL: everything of agent 1 and the workspace; agent 2's inputs all or none; its gradients all or none, none without it
    for name in [k for k in BACKWARD if k.endswith("_p1")] + ["workspace"]:
        assert bwd(**{name: None}) == -1, name
        assert bwd(n=0, **{name: None}) == -1, name
    for name in inputs2:
        assert bwd(**{name: None}) == -1, name
        assert bwd(**{other: None for other in inputs2 if other != name}, **no_grads2) == -1, name
    for name in grads2:
        assert bwd(**{name: None}) == -1, name
        assert bwd(**{other: None for other in grads2 if other != name}) == -1, name
    assert bwd(**{k: None for k in inputs2}) == -1  # gradients of an agent that is not there
    # a shared net: agent 2's gradients absent, its parameter pointers agent 1's
    for name in inputs2[1:7]:
        assert bwd(n=0, **no_grads2, **{name: FAKE + 64}) == -3, name
        assert bwd(n=0, **{name: FAKE + 64}) == 0, name  # (separate gradients: any parameters)
    # sizes: the box of the header
    assert bwd(n=-1) == -2 and bwd(n=(1 << 30) + 1) == -2
    assert bwd(in_features=0) == -2 and bwd(in_features=73, obs_pitch=80) == -2 and bwd(n=0, in_features=72, obs_pitch=72) == 0
    assert bwd(n=0, in_features=1) == 0
    for hidden in (0, 16, 33, 96, 256, -64):
        assert bwd(hidden=hidden) == -2, hidden
    assert bwd(n=0, hidden=32) == 0 and bwd(n=0, hidden=128) == 0
    assert bwd(out_features=0) == -2 and bwd(out_features=41, grad_pitch=41) == -2 and bwd(n=0, out_features=40, grad_pitch=40) == 0
    assert bwd(n=0, out_features=1) == 0
    assert bwd(obs_pitch=34) == -2 and bwd(grad_pitch=18) == -2 and bwd(obs_pitch=1 << 61) == -2 and bwd(grad_pitch=1 << 61) == -2
    assert bwd(n=0, obs_pitch=36, grad_pitch=20) == 0
    # formats and the activation
    for name, count in (("obs_format", 5), ("grad_format", 3), ("activation", 2)):
        assert bwd(**{name: count}) == -3 and bwd(**{name: -1}) == -3, name
        for value in range(count):
            assert bwd(n=0, **{name: value}) == 0, (name, value)
    # alignment to the element; the workspace to 16 bytes
    for name in (k for k in BACKWARD if k.endswith(("_p1", "_p2"))):
        assert bwd(**{name: FAKE + 1}) == -4, name
        two_bytes_go = (name.startswith("obs") and dict(obs_format=1)) or (name.startswith("grad_head") and dict(grad_format=2)) or None
        assert bwd(**{name: FAKE + 2}) == -4, name
        if two_bytes_go:
            assert bwd(n=0, **{name: FAKE + 2}, **two_bytes_go) == 0, name
    for off in (1, 4, 8):
        assert bwd(workspace=FAKE + off) == -4 and bwd(n=0, workspace=FAKE + off) == -4
    assert bwd(n=0, workspace=FAKE + 16) == 0
    # the order of the checks: NULL, size, config, alignment
    assert bwd(b3_p1=None, n=-1, activation=9, dw1_p1=FAKE + 2) == -1
    assert bwd(n=-1, activation=9, dw1_p1=FAKE + 2) == -2
    assert bwd(activation=9, dw1_p1=FAKE + 2) == -3
    assert bwd(w1_p2=FAKE + 64, dw1_p1=FAKE + 2, **no_grads2) == -3
    assert bwd(dw1_p1=FAKE + 2) == -4


def test_workspace_bytes_at_the_edges_of_the_box(lib):
    """0 outside the box; inside it, what the binding restates (without a device: a grid cap of 256 workgroups per agent)"""
    from pikazoo_amd import netgrad

    size = lib.pz_mlp_backward_workspace_bytes
    for bad in ((0, 35, 64, 19), (-1, 35, 64, 19), ((1 << 30) + 1, 35, 64, 19), (8, 0, 64, 19), (8, 73, 64, 19), (8, 35, 48, 19),
                (8, 35, 256, 19), (8, 35, 64, 0), (8, 35, 64, 41)):
        assert size(*bad) == 0 == netgrad.workspace_bytes(*bad), bad
    for good in ((1, 1, 32, 1), (1 << 30, 72, 128, 40), (129, 35, 64, 19), (64, 35, 64, 19), (65, 35, 64, 19), (256 * 32 + 1, 35, 128, 19)):
        n, K, H, O = good
        floats = H * K + H + H * H + H + O * H + O
        blocks = min(-(-n // (32 * (128 // H))), 256)
        assert size(*good) == netgrad.workspace_bytes(*good) == 2 * blocks * floats * 4, good


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, stride, alias and range errors raise ValueError -- on CPU tensors the device check stands behind the
    others, so every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import netgrad

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(netgrad, "load", refuse)

    n, K, H, O = 8, 35, 64, 19
    shapes = [(H, K), (H,), (H, H), (H,), (O, H), (O,)]
    good = [torch.zeros(s) for s in shapes]
    x, g = torch.zeros(n, K), torch.zeros(n, O)
    with pytest.raises(ValueError, match="GPU"):
        netgrad.backward(x, good, g)
    with pytest.raises(ValueError, match="GPU"):
        netgrad.backward({"a": x, "b": x}, good, {"a": g, "b": g.to(torch.bfloat16).float()}, "relu",
                         out=[torch.zeros(s) for s in shapes], workspace=torch.zeros(netgrad.workspace_bytes(n, K, H, O), dtype=torch.uint8))

    def swapped(i, t, base=None):
        return [t if j == i else p for j, p in enumerate(base or good)]

    outs = [torch.zeros(s) for s in shapes]
    two = dict(obs={"a": x, "b": x}, grad_head={"a": g, "b": g})
    bad_calls = [
        dict(obs=torch.zeros(n)), dict(obs=torch.zeros(n, 73)), dict(obs=torch.zeros(n, K, dtype=torch.float64)),
        dict(obs=torch.zeros(K, n).t()), dict(obs={}), dict(obs=None), dict(obs={"a": x, "b": torch.zeros(n + 1, K)}, grad_head=two["grad_head"]),
        dict(activation="gelu"), dict(params=good[:5]), dict(params=good[0]), dict(params={"a": good}),
        dict(params=swapped(0, torch.zeros(H, K + 1))), dict(params=swapped(0, torch.zeros(48, K))),
        dict(params=swapped(0, torch.zeros(H, K, dtype=torch.float16))), dict(params=swapped(1, torch.zeros(H + 1))),
        dict(params=swapped(2, torch.zeros(H, H + 1)[:, :H])), dict(params=swapped(4, torch.zeros(41, H))),
        dict(params=swapped(5, torch.zeros(O + 1))), dict(params=swapped(3, None)),
        # grad_head: shape, dtype, stride, agents
        dict(grad_head=torch.zeros(n, O + 1)), dict(grad_head=torch.zeros(n + 1, O)), dict(grad_head=torch.zeros(n, O, dtype=torch.float64)),
        dict(grad_head=torch.zeros(O, n).t()), dict(grad_head=torch.zeros(1, O).expand(n, O)), dict(grad_head={"a": g}), dict(grad_head=None),
        dict(obs={"a": x, "b": x}, grad_head=g), dict(obs={"a": x, "b": x}, grad_head={"a": g, "c": g}),
        dict(obs={"a": x, "b": x}, grad_head={"a": g, "b": torch.zeros(n, O + 1)[:, :O]}),
        dict(obs={"a": x, "b": x}, grad_head={"a": g, "b": g.half()}),
        # shared
        dict(shared=True), dict(**two, params={"a": good, "b": [p.clone() for p in good]}, shared=True),
        # out
        dict(out=outs[:5]), dict(out=outs[0]), dict(out=swapped(0, torch.zeros(H, K + 1), outs)),
        dict(out=swapped(1, torch.zeros(H, dtype=torch.float64), outs)), dict(out=swapped(2, torch.zeros(H, 2 * H)[:, :H], outs)),
        dict(out={"a": outs}), dict(**two, params={"a": good, "b": good}, out=outs), dict(**two, shared=False, out=outs),
        dict(**two, shared=False, out={"a": outs, "b": outs}),                      # (the two agents' outputs overlap)
        dict(out=swapped(3, outs[1], outs)), dict(out=swapped(0, good[0], outs)),   # (an output twice; an output that is an input)
        dict(out=swapped(5, g[0], outs)),
        # workspace
        dict(workspace=torch.zeros(15, dtype=torch.uint8)), dict(workspace=torch.zeros(1 << 20, dtype=torch.float32)),
        dict(workspace=torch.zeros(1 << 20, dtype=torch.uint8)[1:]), dict(workspace=torch.zeros(2, 1 << 19, dtype=torch.uint8)),
        dict(workspace=x.view(torch.uint8).reshape(-1)), dict(workspace=None, out=None, obs=torch.zeros(n, 0)),
    ]
    for i, bad in enumerate(bad_calls):
        args = dict(obs=x, params=good, grad_head=g, activation="tanh")
        args.update(bad)
        with pytest.raises(ValueError):
            netgrad.backward(**args)
            pytest.fail(f"bad call {i} was accepted: {sorted(bad)}")
    for bad in (dict(params={"a": good}), dict(params=good[:5]), dict(obs=None)):
        args = dict(obs=x, params=good)
        args.update(bad)
        with pytest.raises(ValueError):
            netgrad.head(**args)


# ---- the judge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", CASES + [(1, 32, 1), (72, 128, 40)])
def test_judge_equals_torch_float64_autograd(K, H, O, activation):
    import torch

    sides, params = G.make_case(97, K, H, O, activation, 31, agents=2)
    layers = [torch.nn.Linear(K, H), torch.nn.Linear(H, H), torch.nn.Linear(H, O)]
    act = torch.nn.Tanh if activation == "tanh" else torch.nn.ReLU
    seq = torch.nn.Sequential(layers[0], act(), layers[1], act(), layers[2]).double()
    with torch.no_grad():
        for layer, (W, b) in zip(layers, zip(params[0::2], params[1::2])):
            layer.weight.copy_(torch.from_numpy(W).double())
            layer.bias.copy_(torch.from_numpy(b).double())
    for x, g in sides:
        seq(torch.from_numpy(x).double()).backward(torch.from_numpy(g).double())
    refs, tols, ambiguous = G.judge(sides, params, activation)
    assert ambiguous == 0
    want = [p.grad.numpy() for layer in layers for p in (layer.weight, layer.bias)]
    for name, ref, w, tol in zip(G.NAMES, refs, want, tols):
        assert ref.shape == w.shape == tol.shape, name
        assert np.abs(ref - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), name
        assert (tol >= 0).all() and tol.max() < 1e-3 * max(1.0, np.abs(w).max()), name
    # the forward half of the recursion is net_judge's, bit for bit
    z, e = G.forward_tolerance(sides[0][0], params, activation)
    z0, e0 = N.judge(sides[0][0], params, activation)
    assert np.array_equal(z, z0) and np.array_equal(e, e0)


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", CASES)
def test_float32_restatement_stays_under_a_share_of_the_tolerance(K, H, O, activation):
    """A float32 chain of fused multiply-adds with the rows summed in index order and in a drawn order, one agent and two on a
    shared net, float32 and int32 observations.  Observed here: at most 0.0228 of the tolerance (H = 128, relu; 0.0097 for tanh); asserted with a margin of 2: 0.0456.
    (The bound is a worst case over roundings that all push one way; roundoff that cancels stays far below it.)"""
    worst = 0.0
    for dtype in ("float32", "int32"):
        sides, params = G.make_case(96, K, H, O, activation, 2, agents=2, obs_dtype=dtype)
        for use in (sides[:1], sides):
            refs, tols, ambiguous = G.judge(use, params, activation)
            assert ambiguous == 0
            for order in (None, np.random.default_rng(3)):
                share, beyond = G.worst_share(G.restate_float32(use, params, activation, order=order), refs, tols)
                assert not beyond
                worst = max(worst, share)
    print(f"{K}-{H}-{O} {activation}: worst error / tolerance {worst:.5f}")
    assert 0 < worst <= RESTATEMENT_SHARE


RESTATEMENT_SHARE = 0.0456  # (twice the measurement: see the docstring above)


@pytest.mark.parametrize("K,H,O", CASES)
def test_every_mutant_exceeds_the_tolerance(K, H, O):
    """each of the seven mutants leaves the tolerance in at least one gradient tensor at every hidden width"""
    for activation in N.ACTIVATIONS:
        sides, params = G.make_case(96, K, H, O, activation, 2, agents=2)
        refs, tols, _ = G.judge(sides, params, activation)
        for mutant in G.MUTANTS:
            if mutant == "tanh_derivative_not_squared" and activation == "relu":
                continue
            if mutant == "relu_derivative_one_at_zero":
                continue
            share, beyond = G.worst_share(G.restate_float32(sides, params, activation, mutant=mutant), refs, tols)
            assert share > 1 and beyond, (mutant, activation, share)
            print(mutant, activation, f"{share:.3g}", beyond)
    # relu'(0) = 1: on the integer case, where units sit at z == 0 exactly
    x, params, d3, want = G.integer_case(65, K, H, O)
    good = G.restate_float32([(x, d3)], params, "relu")
    bad = G.restate_float32([(x, d3)], params, "relu", mutant="relu_derivative_one_at_zero")
    assert all(np.array_equal(g.astype(np.int64), w) for g, w in zip(good, want))
    assert any(not np.array_equal(b.astype(np.int64), w) for b, w in zip(bad, want))


def test_the_exact_integer_cases_are_exact_in_float32():
    for n, K, H, O, small in ((65, 35, 64, 19, False), (65, 36, 128, 33, False), (33, 9, 32, 5, False), (1000, 35, 64, 19, True)):
        x, params, d3, want = G.integer_case(n, K, H, O, small=small)
        for order in (None, np.random.default_rng(4)):
            got = G.restate_float32([(x, d3)], params, "relu", order=order)
            for name, g, w in zip(G.NAMES, got, want):
                assert np.array_equal(g.astype(np.int64), w), name
        assert all(np.abs(w).max() > 0 for w in want) and not np.array_equal(params[2], params[2].T)


def test_no_relu_case_of_the_gpu_tests_has_an_ambiguous_unit():
    """the condition under which no element is ever excused: asserted for every relu case the GPU tests draw, each side under
    its own parameters and, for a shared net, all rows together"""
    for n in GPU_BATCHES + (257,):
        sides, sets = G.make_case(n, 35, 64, 19, "relu", GPU_SEED, agents=2, nets=2)
        assert not np.array_equal(sets[0][0], sets[1][0])
        assert all(G.judge([side], params, "relu")[2] == 0 for side, params in zip(sides, sets))
    for K, H, O in GPU_LAYERS:
        sides, params = G.make_case(129, K, H, O, "relu", GPU_SEED, agents=2)
        assert all(G.judge([s], params, "relu")[2] == 0 for s in sides) and G.judge(sides, params, "relu")[2] == 0


# ---- the large end: more passes than workgroups ------------------------------------------------------------------------------
CUS = 256  # the MI355X's compute units: what the host tests size the large cases for (the GPU tests ask the device)
LARGE_LAYERS = {32: (35, 32, 19), 64: (35, 64, 19), 128: (72, 128, 40)}
LARGE_SEED = 11


def large_n(hidden, cus=CUS):
    """the smallest batch of the shape the large tests want: one pass per workgroup, one more for workgroup 0 and a partial
    one (33 rows) for workgroup 1 -- some workgroups carry their accumulators into a second pass, most do not"""
    R = 32 * (128 // hidden)
    return cus * R + R + 33


def large_cases(hidden, activation, cus=CUS):
    """the three launches of tests/test_gpu_netgrad.py's large tolerance test: [(what, sides, params of the call, shared, [(the
    sides of an output group, its parameters)])]"""
    K, H, O = LARGE_LAYERS[hidden]
    n = large_n(hidden, cus)
    sides, sets = G.make_case(n, K, H, O, activation, LARGE_SEED, agents=2, nets=2)
    both, params = G.make_case(n, K, H, O, activation, LARGE_SEED, agents=2)
    return [("one agent", sides[:1], sets[0], False, [(sides[:1], sets[0])]),
            ("two nets", sides, sets, False, [([sides[0]], sets[0]), ([sides[1]], sets[1])]),
            ("a shared net", both, params, True, [(both, params)])]


def test_documented_roundings_is_the_headers_sentence():
    assert G.documented_roundings(1, 64, 256) == 64 and G.documented_roundings(65, 64, 256) == 64 + 1
    assert G.documented_roundings(256 * 64, 64, 256) == 64 + 255 and G.documented_roundings(256 * 64 + 1, 64, 256) == 128 + 255
    assert G.documented_roundings(32833, 64, 256, shared=True) == 3 * 64 + 255 + 1 == 448
    assert G.documented_roundings(large_n(32), 32, 256) == 2 * 128 + 255 and G.documented_roundings(large_n(128, 304), 128, 304, True) == 2 * 32 + 304
    # the default of judge is the number of rows
    sides, params = G.make_case(70, 35, 64, 19, "tanh", 3, agents=2)
    a, b = G.judge(sides, params, "tanh"), G.judge(sides, params, "tanh", roundings=140)
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    tight = G.judge(sides, params, "tanh", roundings=64 + 1)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], tight[0])) and all((t < u).all() for t, u in zip(tight[1], a[1]))


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("hidden", sorted(LARGE_LAYERS))
def test_the_large_cases_and_the_pass_order_restatement(hidden, activation):
    """At n = CUS * R + R + 33 the float32 restatement that walks the rows in the header's pass order -- workgroup b its passes
    b, b + B, ..., the partials in index order, agent 2's total last -- stays within the tolerance of the header's own count
    of roundings, for one agent and for a shared net; every case the GPU test draws has no ambiguous relu unit."""
    n = large_n(hidden)
    for what, sides, params, shared, groups in large_cases(hidden, activation):
        m = G.documented_roundings(n, hidden, CUS, shared)
        for own, own_params in groups:
            refs, tols, ambiguous = G.judge(own, own_params, activation, roundings=m)
            assert ambiguous == 0, what
        if what == "two nets":
            continue
        share, beyond = G.worst_share(G.restate_float32_in_pass_order(sides, params, activation, CUS), refs, tols)
        print(f"H = {hidden} {activation} n = {n} {what}: {m} roundings, worst error / tolerance {share:.4f}")
        assert not beyond and 0 < share <= 1, (what, share, beyond)


@pytest.mark.parametrize("hidden", sorted(LARGE_LAYERS))
def test_a_lost_pass_exceeds_the_tightened_tolerance(hidden):
    """A pass dropped, a pass counted twice and the partial last pass dropped, as the float64 sum over the rows such a kernel
    would take: each leaves the tolerance of the documented count of roundings, under both activations (observed: 17 to 2 500
    tolerances).  The share of the tolerance at roundings = n is printed beside it: at these n -- the smallest that reach a
    second pass -- it is 0.39 to 0.88 at hidden 32 under tanh, where a lost pass goes unseen, and above 1 elsewhere; it falls
    like 1 / n, and the test below holds the three mutants inside it at the exact case's n."""
    K, H, O = LARGE_LAYERS[hidden]
    n = large_n(hidden)
    for activation in N.ACTIVATIONS:
        sides, params = G.make_case(n, K, H, O, activation, LARGE_SEED)
        x, g = sides[0]
        refs, tols, _ = G.judge(sides, params, activation, roundings=G.documented_roundings(n, hidden, CUS))
        _, loose, _ = G.judge(sides, params, activation)
        for mutant in G.PASS_MUTANTS:
            rows = G.pass_mutant_rows(n, hidden, mutant)
            have = G.judge([(x[rows], g[rows])], params, activation)[0]
            share, beyond = G.worst_share(have, refs, tols)
            wide = G.worst_share(have, refs, loose)[0]
            print(f"H = {hidden} {activation} {mutant}: {share:.3g} of the tightened tolerance in {beyond}, {wide:.3g} of the one at roundings = n")
            assert share > 1 and beyond, (mutant, activation, share)


def test_a_lost_pass_stays_inside_the_tolerance_of_n_roundings():
    """Why `roundings` exists.  At (32833, 35, 64, 19), tanh -- every workgroup of 256 in its third pass, as the GPU test's exact
    case -- the same three mutants stay INSIDE the tolerance at the default roundings = n (it grows like n^2: gamma(n) times a
    sum of n magnitudes), and leave the one at the documented count, 448 with a shared net's last addition."""
    n, hidden = 32833, 64
    sides, params = G.make_case(n, 35, hidden, 19, "tanh", 11)
    x, g = sides[0]
    refs, loose, _ = G.judge(sides, params, "tanh")
    _, tight, _ = G.judge(sides, params, "tanh", roundings=G.documented_roundings(n, hidden, CUS, shared=True))
    for mutant in G.PASS_MUTANTS:
        rows = G.pass_mutant_rows(n, hidden, mutant)
        have = G.judge([(x[rows], g[rows])], params, "tanh")[0]
        wide, share = G.worst_share(have, refs, loose)[0], G.worst_share(have, refs, tight)[0]
        print(f"{mutant}: {wide:.3g} of the tolerance at roundings = n, {share:.3g} of the one at 448")
        assert 0 < wide <= 1 < share, (mutant, wide, share)


def test_the_integer_cases_are_what_int64_products_give():
    """integer_case's products are float64 BLAS calls (exact below 2^53, asserted there): at the sizes the tests had before, the
    results equal those of numpy's int64 products on the same draws, for this judge and for net_judge's"""
    for n, K, H, O, small in ((65, 35, 64, 19, False), (65, 36, 128, 33, False), (33, 9, 32, 5, False), (1000, 35, 64, 19, True)):
        x, params, d3, want = G.integer_case(n, K, H, O, small=small)
        assert x.dtype == d3.dtype == np.int64 and all(w.dtype == np.int64 for w in want)
        W1, b1, W2, b2, W3, b3 = (p.astype(np.int64) for p in params)
        z1 = x @ W1.T + b1
        h1 = np.maximum(z1, 0)
        z2 = h1 @ W2.T + b2
        h2 = np.maximum(z2, 0)
        d2 = (d3 @ W3) * (z2 > 0)
        d1 = (d2 @ W2) * (z1 > 0)
        plain = [d1.T @ x, d1.sum(axis=0), d2.T @ h1, d2.sum(axis=0), d3.T @ h2, d3.sum(axis=0)]
        assert all(np.array_equal(a, b) for a, b in zip(want, plain)), (n, K, H, O)
    for n, K, H, O in ((65, 35, 64, 19), (65, 36, 128, 33), (33, 9, 32, 5)):
        x, params, want = N.integer_case(n, K, H, O)
        h = x
        for layer in range(3):
            h = h @ params[2 * layer].astype(np.int64).T + params[2 * layer + 1].astype(np.int64)
            h = np.maximum(h, 0) if layer < 2 else h
        assert want.dtype == np.int64 and np.array_equal(want, h), (n, K, H, O)
    with pytest.raises(AssertionError):
        N.exact_matmul(np.full((1, 2), 2 ** 27), np.full((2, 1), 2 ** 26))


def test_the_large_integer_cases_stay_exact():
    """the '< 2^24' assertions of integer_case hold at the cap-sized row counts of the GPU test, and at twice that for the
    shared net's sum over both agents"""
    for hidden in sorted(LARGE_LAYERS):
        n = 2 * CUS * 32 * (128 // hidden) + 65
        x, params, d3, want = G.integer_case(2 * n, 35, hidden, 19, small=True)
        assert len(x) == 2 * n and all(np.abs(w).max() > 0 for w in want)
