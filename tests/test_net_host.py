"""CPU tests (no GPU needed) of the policy-net library: libpikazoo_net.so exports its header's symbols and carries the tree's
build id, nothing loads it before its first use, its code object holds exactly the six kernels named below without scratch
or spilled vector registers, the entry point refuses bad arguments before any launch and in the documented order,
``pikazoo_amd.net`` raises ``ValueError`` for malformed arguments before it needs the library, and the judge the GPU tests
compare with (tests/net_judge.py) is the definition: equal to a torch float64 ``nn.Sequential``, wide enough for a float32
restatement in two summation orders, and sharp enough that six mutants fail."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import net_judge as N
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_mlp_forward", "pz_net_abi_version", "pz_net_build_id"]
KERNELS = sorted(f"pz_net::mlp_forward_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1))
CASES = [(35, H, 19) for H in (32, 64, 128)]


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def net_lib(pz_build):
    from pikazoo_amd import net

    return net.load()


def declared_arguments(text, name):
    decl = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert decl, f"{name} is not shown"
    return [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]


def test_net_library_exports_exactly_its_header(pz_build, net_lib):
    from pikazoo_amd import _native, net

    assert header_functions("pikazoo_net.h") == NAMES == sorted(net.SIGNATURES) == dynamic_pz_symbols(pz_build.NET_LIB)
    assert pz_build.library_id(pz_build.NET_LIB) == pz_build.source_id() == net_lib.pz_net_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.NET_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_net.h") in pz_build.DEPS
    assert (pz_build.CSRC / "pz_mlp_tile.hpp") in pz_build.DEPS
    assert net_lib.pz_net_abi_version() == net.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_net.h").read_text()
    assert "#define PZ_NET_ABI_VERSION 1" in header
    # no other library holds any of the names, and the product's ABI did not move
    assert _native.load().pz_abi_version() == 10
    for other in (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB, pz_build.PPO_LIB):
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_mlp_forward")
    assert len(args) == 26 == len(net.SIGNATURES["pz_mlp_forward"][1])
    assert declared_arguments(doc, "pz_mlp_forward") == args
    assert "pikazoo_net.h" in doc and "libpikazoo_net.so" in doc
    # the binding's tables are the header's enums, and the box is the header's
    for table, prefix in ((net.OBS_FORMATS, "PZ_NET_OBS_"), (net.OUT_FORMATS, "PZ_NET_OUT_"), (net.ACTIVATIONS, "PZ_NET_ACT_")):
        for key, value in table.items():
            name = prefix + (key if isinstance(key, str) else str(key).split(".")[-1]).upper()
            assert re.search(r"%s = %d\b" % (name, value), header), name
    assert [str(d).split(".")[-1] for d in net.OBS_FORMATS] == list(N.OBS_DTYPES)
    assert [str(d).split(".")[-1] for d in net.OUT_FORMATS] == list(N.OUT_DTYPES) and tuple(net.ACTIVATIONS) == N.ACTIVATIONS
    assert f"#define PZ_NET_MAX_IN {net.MAX_IN}" in header and f"#define PZ_NET_MAX_OUT {net.MAX_OUT}" in header


def test_importing_the_step_path_learn_policy_or_ppo_does_not_load_the_net_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo; "
            "assert 'pikazoo_amd.net' not in sys.modules; import pikazoo_amd as p; assert 'net' in p.__all__; p.net.forward; "
            "assert 'pikazoo_amd.net' in sys.modules and p.net._lib is None; "
            "assert not any('libpikazoo_net' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_net_library(pz_build):
    """Hidden width and activation are the COMPILE-TIME choices: 3 x 2 kernels and nothing else; the observation and the
    output format are run-time.  None uses scratch or spills a vector register; the LDS is dynamic (the staged parameter
    set: its size depends on in_features and out_features), so the static segment is empty.  The two narrower widths
    leave room for two waves per SIMD (at most 256 registers, accumulation registers included)."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.NET_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.NET_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0, (name, row)
        total = row[".vgpr_count"] + row.get(".agpr_count", 0)
        assert total <= (512 if "<128" in name else 256), (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


FAKE = 4096
FORWARD = dict(obs_p1=FAKE, obs_p2=FAKE, obs_format=2, n=8, in_features=35, obs_pitch=35, hidden=64, out_features=19, activation=0,
               w1_p1=FAKE, b1_p1=FAKE, w2_p1=FAKE, b2_p1=FAKE, w3_p1=FAKE, b3_p1=FAKE, w1_p2=FAKE, b1_p2=FAKE, w2_p2=FAKE, b2_p2=FAKE,
               w3_p2=FAKE, b3_p2=FAKE, out_p1=FAKE, out_p2=FAKE, out_format=0, out_pitch=19, stream=None)


def test_argument_validation(net_lib):
    """every check on fake pointers: a call that passes them all has n = 0 and launches nothing"""
    def fwd(**over):
        a = dict(FORWARD)
        assert not set(over) - set(a)
        a.update(over)
        return net_lib.pz_mlp_forward(*a.values())

    side2 = [k for k in FORWARD if k.endswith("_p2")]
    assert len(side2) == 8
    assert fwd(n=0) == 0 and fwd(n=0, **{k: None for k in side2}) == 0
    # NULL: everything of agent 1; agent 2 all or none
    for name in (k for k in FORWARD if k.endswith("_p1")):
        assert fwd(**{name: None}) == -1, name
    for name in side2:
        assert fwd(**{name: None}) == -1, name
        assert fwd(**{other: None for other in side2 if other != name}) == -1, name
    # shared weights: agent 2's parameter pointers are agent 1's
    assert fwd(n=0, obs_p2=FAKE + 64, out_p2=FAKE + 128) == 0
    # sizes: the box of the header
    assert fwd(n=-1) == -2 and fwd(n=(1 << 30) + 1) == -2
    assert fwd(in_features=0) == -2 and fwd(in_features=73, obs_pitch=80) == -2 and fwd(n=0, in_features=72, obs_pitch=72) == 0
    assert fwd(n=0, in_features=1) == 0
    for hidden in (0, 16, 33, 96, 256, -64):
        assert fwd(hidden=hidden) == -2, hidden
    assert fwd(n=0, hidden=32) == 0 and fwd(n=0, hidden=128) == 0
    assert fwd(out_features=0) == -2 and fwd(out_features=41, out_pitch=41) == -2 and fwd(n=0, out_features=40, out_pitch=40) == 0
    assert fwd(n=0, out_features=1) == 0
    assert fwd(obs_pitch=34) == -2 and fwd(out_pitch=18) == -2 and fwd(obs_pitch=1 << 61) == -2 and fwd(out_pitch=1 << 61) == -2
    assert fwd(n=0, obs_pitch=36, out_pitch=20) == 0
    # formats and the activation
    for name, count in (("obs_format", 5), ("out_format", 3), ("activation", 2)):
        assert fwd(**{name: count}) == -3 and fwd(**{name: -1}) == -3, name
        for value in range(count):
            assert fwd(n=0, **{name: value}) == 0, (name, value)
    # alignment to the element
    for name in (k for k in FORWARD if k.endswith(("_p1", "_p2"))):
        assert fwd(**{name: FAKE + 1}) == -4, name
        two_bytes_go = (name.startswith("obs") and dict(obs_format=1)) or (name.startswith("out") and dict(out_format=2)) or None
        assert fwd(**{name: FAKE + 2}) == -4, name
        if two_bytes_go:
            assert fwd(n=0, **{name: FAKE + 2}, **two_bytes_go) == 0, name
    assert fwd(obs_format=3, obs_p2=FAKE + 1) == -4 and fwd(n=0, obs_format=4, obs_p1=FAKE + 2, obs_p2=FAKE + 6) == 0
    # the order of the checks: NULL, size, config, alignment
    assert fwd(b3_p1=None, n=-1, activation=9, out_p1=FAKE + 2) == -1
    assert fwd(n=-1, activation=9, out_p1=FAKE + 2) == -2
    assert fwd(activation=9, out_p1=FAKE + 2) == -3
    assert fwd(out_p1=FAKE + 2) == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device and range errors raise ValueError -- on CPU tensors the device check stands behind the others,
    so every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import net

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(net, "load", refuse)

    n, K, H, O = 8, 35, 64, 19
    good = [torch.zeros(H, K), torch.zeros(H), torch.zeros(H, H), torch.zeros(H), torch.zeros(O, H), torch.zeros(O)]
    x = torch.zeros(n, K)
    with pytest.raises(ValueError, match="GPU"):
        net.forward(x, good)
    with pytest.raises(ValueError, match="GPU"):
        net.forward({"a": x, "b": x}, good, "relu", out_dtype=torch.bfloat16)

    def swapped(i, t):
        return [t if j == i else p for j, p in enumerate(good)]

    bad_calls = [
        dict(obs=torch.zeros(n)), dict(obs=torch.zeros(n, 73)), dict(obs=torch.zeros(n, K, dtype=torch.float64)),
        dict(obs=torch.zeros(n, K, dtype=torch.int64)), dict(obs=torch.zeros(K, n).t()), dict(obs={}), dict(obs=None),
        dict(obs={"a": x, "b": torch.zeros(n + 1, K)}), dict(obs={"a": x, "b": torch.zeros(n, K + 1)[:, :K]}),
        dict(obs={"a": x, "b": x, "c": x}), dict(activation="gelu"), dict(out_dtype=torch.float64), dict(params=good[:5]),
        dict(params=good[0]), dict(params={"a": good}), dict(obs={"a": x}, params={"b": good}),
        dict(params=swapped(0, torch.zeros(H, K + 1))), dict(params=swapped(0, torch.zeros(48, K))),
        dict(params=swapped(0, torch.zeros(H, K, dtype=torch.float16))), dict(params=swapped(1, torch.zeros(H + 1))),
        dict(params=swapped(2, torch.zeros(H, H + 1)[:, :H])), dict(params=swapped(4, torch.zeros(41, H))),
        dict(params=swapped(5, torch.zeros(O + 1))), dict(params=swapped(3, None)),
        dict(out=torch.zeros(n, O + 1)), dict(out=torch.zeros(n, O, dtype=torch.float64)), dict(out={"a": torch.zeros(n, O)}),
    ]
    for bad in bad_calls:
        args = dict(obs=x, params=good, activation="tanh")
        args.update(bad)
        with pytest.raises(ValueError):
            net.forward(**args)
    for bad in (dict(in_features=0), dict(in_features=73), dict(hidden=48), dict(num_actions=40), dict(activation="gelu")):
        with pytest.raises(ValueError):
            net.ActorCritic(**bad)


# ---- the judge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", CASES + [(1, 32, 1), (72, 128, 40)])
def test_judge_equals_a_torch_float64_sequential(K, H, O, activation):
    import torch

    params = N.make_params(K, H, O, 31)
    x = N.make_obs(97, K, "float32", 32)
    layers = [torch.nn.Linear(K, H), torch.nn.Linear(H, H), torch.nn.Linear(H, O)]
    act = torch.nn.Tanh if activation == "tanh" else torch.nn.ReLU
    seq = torch.nn.Sequential(layers[0], act(), layers[1], act(), layers[2]).double()
    with torch.no_grad():
        for layer, (W, b) in zip(layers, zip(params[0::2], params[1::2])):
            layer.weight.copy_(torch.from_numpy(W).double())
            layer.bias.copy_(torch.from_numpy(b).double())
        want = seq(torch.from_numpy(x).double()).numpy()
    ref, tol = N.judge(x, params, activation)
    assert np.allclose(ref, want, rtol=0, atol=1e-13)
    assert (tol > N.U).all() and tol.max() < 1e-3  # (the a-priori bound of three inner products: some 1e-4 at the widest net)


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O", CASES)
def test_float32_restatement_stays_under_a_share_of_the_tolerance(K, H, O, activation):
    """A float32 chain of fused multiply-adds, in index order and in a drawn order, on observations uniform in [0, 1) and on
    raw integer observations in [-20, 432].  Observed here: at most 0.0041 of the tolerance ([0, 1), H = 32, tanh, index
    order), 0.0034 in a drawn order, 0.0002 on the integer observations; asserted with a margin of 2: 0.0082.  (The bound
    is a worst case over K + 1 roundings that all push one way; roundoff that cancels stays two orders below it.)"""
    params = N.make_params(K, H, O, 1)
    worst = 0.0
    for dtype in ("float32", "int32"):
        x = N.make_obs(256, K, dtype, 2)
        ref, tol = N.judge(x, params, activation)
        for order in (None, np.random.default_rng(3)):
            share, rows = N.worst_share(N.restate_float32(x, params, activation, order=order), ref, tol)
            assert rows == 0
            worst = max(worst, share)
    print(f"{K}-{H}-{O} {activation}: worst error / tolerance {worst:.5f}")
    assert 0 < worst <= 0.0082


@pytest.mark.parametrize("K,H,O", CASES)
def test_every_mutant_exceeds_the_tolerance(K, H, O):
    """each of the six mutants fails in at least 74 % of the rows at every hidden width on the [0, 1) inputs; the two
    bfloat16 ones in all rows.  (The rational tanh is a mutant of the tanh net only.)"""
    params = N.make_params(K, H, O, 1)
    x = N.make_obs(256, K, "float32", 2)
    for activation in N.ACTIVATIONS:
        ref, tol = N.judge(x, params, activation)
        for mutant in N.MUTANTS:
            if mutant == "rational_tanh" and activation == "relu":
                continue
            share, rows = N.worst_share(N.restate_float32(x, params, activation, mutant=mutant), ref, tol)
            assert share > 1 and rows >= 0.74, (mutant, activation, share, rows)
            if mutant.startswith("bfloat16"):
                assert rows == 1.0 and share > 4, (mutant, activation, share)


def test_sixteen_bit_outputs_add_half_a_unit_of_the_format():
    params = N.make_params(35, 64, 19, 1)
    x = N.make_obs(64, 35, "float32", 2)
    ref, tol = N.judge(x, params, "tanh")
    for dtype, mant in (("float16", 10), ("bfloat16", 7)):
        ref16, tol16 = N.judge(x, params, "tanh", dtype)
        assert np.array_equal(ref16, ref) and (tol16 > tol).all()
        assert (tol16 - tol <= 2.0 ** (np.floor(np.log2(np.abs(ref) + tol)) - mant - 1) * 1.0001).all()
        rounded, _ = N.J.round_to(N.restate_float32(x, params, "tanh").astype(np.float64), dtype)
        assert N.worst_share(rounded, ref, tol16)[0] <= 1


def test_the_exact_integer_cases_are_exact_in_float32():
    for n, K, H, O in ((65, 35, 64, 19), (65, 36, 128, 33), (33, 9, 32, 5)):
        x, params, want = N.integer_case(n, K, H, O)
        for order in (None, np.random.default_rng(4)):
            assert np.array_equal(N.restate_float32(x, params, "relu", order=order).astype(np.int64), want)
        assert len(np.unique(want)) > want.size // 4 and not np.array_equal(params[2], params[2].T)


def test_the_integer_case_keeps_its_results_and_its_bounds_at_the_large_batch():
    """integer_case's products are float64 BLAS calls, exact below 2^53 (asserted by exact_matmul): at the sizes above the result
    is what numpy's int64 products give on the same draws; and its own bounds hold at the batch of
    tests/test_gpu_net.py's large tests on 256 compute units"""
    for n, K, H, O in ((65, 35, 64, 19), (65, 36, 128, 33), (33, 9, 32, 5)):
        x, params, want = N.integer_case(n, K, H, O)
        h = x
        for layer in range(3):
            h = h @ params[2 * layer].astype(np.int64).T + params[2 * layer + 1].astype(np.int64)
            h = np.maximum(h, 0) if layer < 2 else h
        assert x.dtype == want.dtype == np.int64 and np.array_equal(want, h), (n, K, H, O)
    with pytest.raises(AssertionError):
        N.exact_matmul(np.full((1, 2), 2 ** 27), np.full((2, 1), 2 ** 26))
    n = 2 * (2 * 256) * 128 + 128 + 37
    for K, H, O in ((35, 32, 19), (35, 64, 19), (72, 128, 40)):
        x, params, want = N.integer_case(n, K, H, O)
        assert want.shape == (n, O) and np.abs(want).max() > 0


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
def test_actor_critic_forward_matches_the_judge_on_the_cpu(activation):
    import torch

    from pikazoo_amd import net

    torch.manual_seed(0)
    model = net.ActorCritic(activation=activation)
    W1, b1, W2, b2, W3, b3 = model.parameter_tensors()
    assert tuple(W1.shape) == (64, 35) and tuple(W3.shape) == (19, 64) and all(float(b.detach().abs().max()) == 0 for b in (b1, b2, b3))
    # orthogonal rows (or columns) at the gains sqrt 2, sqrt 2 and 0.01
    for W, gain in ((W1, 2.0), (W2, 2.0), (W3, 1e-4)):
        M = W.detach().double()
        G = M.T @ M if M.shape[0] >= M.shape[1] else M @ M.T
        assert torch.allclose(G, gain * torch.eye(G.shape[0], dtype=torch.float64), atol=1e-5 * gain)
    with torch.no_grad():
        for b in (b1, b2, b3):
            b.uniform_(-0.2, 0.2)
    params = [p.detach().numpy() for p in model.parameter_tensors()]
    for dtype in ("float32", "int32", "bfloat16"):
        x = N.make_obs(128, 35, dtype, 41)
        t = torch.from_numpy(x) if dtype != "bfloat16" else torch.from_numpy(x).to(torch.bfloat16)
        out = model(t)
        assert out.requires_grad and tuple(out.shape) == (128, 19)
        ref, tol = N.judge(x, params, activation)
        assert N.worst_share(out.detach().numpy(), ref, tol)[0] <= 1, dtype
    with pytest.raises(ValueError, match="GPU"):
        model.act(torch.zeros(4, 35))
