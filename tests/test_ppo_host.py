"""CPU tests (no GPU needed) of the PPO-loss library: libpikazoo_ppo.so exports its header's symbols and carries the tree's
build id, nothing loads it before its first use, its code object holds exactly the six kernels named below without scratch
or spills, the entry points refuse bad arguments before any launch and in the documented order, and the judge the GPU
tests compare with (tests/ppo_judge.py) is the definition: equal to central differences and to a torch float64
formulation under autograd, within its own derived tolerances of a float32 restatement, rarely ambiguous on the GPU tests'
cases, and sharp enough that six mutants fail."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import policy_judge as J
import ppo_judge as P
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_ppo_abi_version", "pz_ppo_build_id", "pz_ppo_loss", "pz_ppo_moments", "pz_ppo_workspace_bytes"]
KERNELS = sorted([f"pz_ppo::loss_kernel<{lf}>" for lf in (0, 1, 2)] +
                 ["pz_ppo::loss_finish_kernel", "pz_ppo::moments_kernel", "pz_ppo::moments_finish_kernel"])


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def ppo_lib(pz_build):
    from pikazoo_amd import ppo

    return ppo.load()


def declared_arguments(text, name):
    decl = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert decl, f"{name} is not shown"
    return [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]


def test_ppo_library_exports_exactly_its_header(pz_build, ppo_lib):
    from pikazoo_amd import _native, ppo

    assert header_functions("pikazoo_ppo.h") == NAMES == sorted(ppo.SIGNATURES) == dynamic_pz_symbols(pz_build.PPO_LIB)
    assert pz_build.library_id(pz_build.PPO_LIB) == pz_build.source_id() == ppo_lib.pz_ppo_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.PPO_SOURCES[0] in pz_build.DEPS and (pz_build.CSRC / "pz_policy_rows.hpp") in pz_build.DEPS
    assert ppo_lib.pz_ppo_abi_version() == ppo.ABI_VERSION == 1
    assert "#define PZ_PPO_ABI_VERSION 1" in (REPO / "include" / "pikazoo_ppo.h").read_text()
    # no other library holds any of the names, and the product's ABI did not move
    assert _native.load().pz_abi_version() == 10
    for other in (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB):
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    # INTEGRATION.md shows the entry points as the header declares them (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_ppo.h").read_text(), flags=re.S)
    for name, count in (("pz_ppo_moments", 7), ("pz_ppo_loss", 36)):
        args = declared_arguments(header, name)
        assert len(args) == count == len(ppo.SIGNATURES[name][1]), name
        assert declared_arguments(doc, name) == args, name
    assert "pikazoo_ppo.h" in doc and "libpikazoo_ppo.so" in doc and "pz_ppo_workspace_bytes" in doc
    # the binding's own formula of the workspace is the library's
    for n in (-1, 0, 1, 64, 65, 4096, 4097, 19141, 1 << 20, 1 << 30, (1 << 30) + 1):
        assert ppo.workspace_bytes(n) == ppo_lib.pz_ppo_workspace_bytes(n), n
        assert ppo.workspace_bytes(n) % 16 == 0
    assert (ppo.ROWS_PER_PARTIAL, ppo.FINISH_THREADS) == (P.ROWS_PER_WAVE, P.FINISH_THREADS)


def test_importing_the_package_learn_or_policy_does_not_load_the_ppo_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; from pikazoo_amd import env, pikazoo_v0, learn, policy; "
            "assert 'pikazoo_amd.ppo' not in sys.modules; import pikazoo_amd as p; assert 'ppo' in p.__all__; p.ppo.loss; "
            "assert 'pikazoo_amd.ppo' in sys.modules and p.ppo._lib is None and p.policy._lib is None; "
            "assert not any('libpikazoo_ppo' in line or 'libpikazoo_policy' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_ppo_library(pz_build):
    """The logit format is the one COMPILE-TIME choice of the loss kernel: 3 loss kernels, their finisher, the moments
    kernel and its finisher, and nothing else.  None uses scratch or spills a register; a loss kernel holds one wave's
    transposed image in LDS (64 rows of 33 dwords), a finisher the 256 float64 sums it folds."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.PPO_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    assert all(count > 100 for name, (_, count) in table.items() if name in KERNELS)
    notes = kernel_notes.notes(pz_build.PPO_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".vgpr_count"] <= 128, (name, row)
        if "loss_kernel" in name:
            assert row[".group_segment_fixed_size"] == 64 * 33 * 4, (name, row)
        elif "finish" in name:
            assert row[".group_segment_fixed_size"] == 256 * 8, (name, row)


FAKE = 4096
LOSS = dict(logits_p1=FAKE, logits_p2=FAKE, logit_format=0, num_actions=18, n=8, logit_pitch=18, action_format=1, act_p1=FAKE, act_p2=FAKE,
            old_logp_p1=FAKE, old_logp_p2=FAKE, adv_p1=FAKE, adv_p2=FAKE, ret_p1=FAKE, ret_p2=FAKE, values_p1=FAKE, values_p2=FAKE,
            value_format=0, value_pitch=1, old_values_p1=FAKE, old_values_p2=FAKE, old_value_format=0, adv_norm=FAKE, clip=0.2,
            value_clip=0.2, vf_coef=0.5, ent_coef=0.01, grad_logits_p1=FAKE, grad_logits_p2=FAKE, grad_pitch=18, grad_values_p1=FAKE,
            grad_values_p2=FAKE, grad_value_pitch=1, stats=FAKE, workspace=FAKE, stream=None)
MOMENTS = dict(x_p1=FAKE, x_p2=FAKE, n=0, eps=1e-8, out=FAKE, workspace=FAKE, stream=None)


def call(fn, defaults, **over):
    a = dict(defaults)
    assert not set(over) - set(a)
    a.update(over)
    return fn(*a.values())


def test_argument_validation(ppo_lib):
    """every check on fake pointers: a call that passes them all has n = 0 and launches nothing"""
    loss = lambda **o: call(ppo_lib.pz_ppo_loss, LOSS, **o)  # noqa: E731
    mom = lambda **o: call(ppo_lib.pz_ppo_moments, MOMENTS, **o)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    assert loss(n=0) == 0
    side2 = [k for k in LOSS if k.endswith("_p2")]
    assert loss(n=0, **{k: None for k in side2}) == 0
    # NULL: what agent 1 must have; agent 2 all or none, and exactly where agent 1 has the optional ones
    for name in ("logits_p1", "act_p1", "old_logp_p1", "adv_p1", "ret_p1", "values_p1", "stats", "workspace"):
        assert loss(**{name: None}) == -1, name
    for name in side2:
        assert loss(**{name: None}) == -1, name
        assert loss(**{other: None for other in side2 if other != name}) == -1, name
    assert loss(old_values_p1=None, old_values_p2=None) == -1                       # required: value_clip > 0
    assert loss(n=0, old_values_p1=None, old_values_p2=None, value_clip=0.0) == 0   # ... and not otherwise
    assert loss(n=0, value_clip=0.0) == 0                                           # (given and ignored)
    assert loss(grad_logits_p1=None) == -1 and loss(grad_values_p2=None) == -1
    assert loss(n=0, grad_logits_p1=None, grad_logits_p2=None) == 0 and loss(n=0, grad_values_p1=None, grad_values_p2=None) == 0
    assert loss(n=0, grad_logits_p1=None, grad_logits_p2=None, grad_values_p1=None, grad_values_p2=None, adv_norm=None) == 0
    # sizes
    assert loss(n=-1) == -2 and loss(n=(1 << 30) + 1) == -2
    assert loss(num_actions=1) == -2 and loss(num_actions=33, logit_pitch=40, grad_pitch=40) == -2
    assert loss(logit_pitch=17) == -2 and loss(grad_pitch=17) == -2 and loss(logit_pitch=1 << 61) == -2
    assert loss(n=0, grad_pitch=17, grad_logits_p1=None, grad_logits_p2=None) == 0  # (no gradient: its pitch is not read)
    assert loss(value_pitch=0) == -2 and loss(grad_value_pitch=0) == -2 and loss(value_pitch=1 << 61) == -2
    assert loss(n=0, grad_value_pitch=0, grad_values_p1=None, grad_values_p2=None) == 0
    assert loss(n=0, value_pitch=19, grad_value_pitch=19, logit_pitch=19, grad_pitch=19) == 0  # the fused head
    # formats and coefficients
    for name in ("logit_format", "action_format", "value_format", "old_value_format"):
        assert loss(**{name: 3}) == -3 and loss(**{name: -1}) == -3, name
    assert loss(n=0, old_value_format=7, value_clip=0.0, old_values_p1=None, old_values_p2=None) == 0
    for bad in (0.0, 1.0, -0.1, 1.5, inf, nan):
        assert loss(clip=bad) == -3, bad
    for name in ("value_clip", "vf_coef", "ent_coef"):
        for bad in (-0.5, inf, nan):
            assert loss(**{name: bad}) == -3, (name, bad)
    assert loss(n=0, vf_coef=0.0, ent_coef=0.0, clip=0.999) == 0
    # alignment to the element; the workspace to 16 bytes
    for name in ("logits_p1", "logits_p2", "grad_logits_p1", "grad_logits_p2", "values_p1", "values_p2", "grad_values_p1", "grad_values_p2",
                 "old_values_p1", "old_values_p2", "old_logp_p1", "old_logp_p2", "adv_p1", "adv_p2", "ret_p1", "ret_p2", "adv_norm", "stats"):
        assert loss(**{name: FAKE + 2}) == -4, name
    assert loss(n=0, logit_format=2, logits_p1=FAKE + 2, grad_logits_p2=FAKE + 2) == 0 and loss(logit_format=1, logits_p1=FAKE + 1) == -4
    assert loss(n=0, value_format=1, values_p1=FAKE + 2, grad_values_p1=FAKE + 2) == 0 and loss(n=0, old_value_format=2, old_values_p2=FAKE + 2) == 0
    assert loss(act_p1=FAKE + 4) == -4 and loss(n=0, action_format=0, act_p1=FAKE + 4) == 0
    assert loss(workspace=FAKE + 8) == -4 and loss(workspace=FAKE + 4) == -4
    # the order of the checks: NULL, size, config, alignment
    assert loss(stats=None, n=-1, clip=2.0, workspace=FAKE + 8) == -1
    assert loss(n=-1, clip=2.0, workspace=FAKE + 8) == -2
    assert loss(clip=2.0, workspace=FAKE + 8) == -3
    assert loss(workspace=FAKE + 8) == -4
    # the moments
    assert mom() == 0 and mom(x_p2=None) == 0
    for name in ("x_p1", "out", "workspace"):
        assert mom(**{name: None}) == -1, name
    assert mom(n=1) == -2 and mom(n=-1) == -2 and mom(n=(1 << 30) + 1) == -2
    assert mom(eps=-1.0) == -3 and mom(eps=inf) == -3 and mom(eps=nan) == -3 and mom(eps=0.0) == 0
    assert mom(x_p1=FAKE + 2) == -4 and mom(x_p2=FAKE + 2) == -4 and mom(out=FAKE + 2) == -4 and mom(workspace=FAKE + 8) == -4
    assert mom(out=None, n=1, eps=-1.0, workspace=FAKE + 8) == -1 and mom(n=1, eps=-1.0, workspace=FAKE + 8) == -2
    assert mom(eps=-1.0, workspace=FAKE + 8) == -3
    assert ppo_lib.pz_ppo_workspace_bytes(0) == 0 and ppo_lib.pz_ppo_workspace_bytes(1) == 48


def test_python_errors_come_before_any_launch():
    """shape, dtype, device, range and aliasing errors raise ValueError -- on CPU tensors the device check stands behind the
    shape checks of the logits, so those are reachable here"""
    import torch

    from pikazoo_amd import ppo

    n, A = 8, 18
    l, v, a = torch.zeros(n, A), torch.zeros(n), torch.zeros(n, dtype=torch.int64)
    f = torch.zeros(n)
    with pytest.raises(ValueError, match="GPU"):
        ppo.loss_and_grad(l, v, a, f, f, f)
    with pytest.raises(ValueError, match="GPU"):
        ppo.loss(l, v, a, f, f, f)
    with pytest.raises(ValueError, match="GPU"):
        ppo.moments(f)
    for bad in (dict(logits=torch.zeros(n)), dict(logits=torch.zeros(n, 33)), dict(logits=torch.zeros(n, A, dtype=torch.float64)),
                dict(logits=None), dict(values=None), dict(actions=None), dict(head=torch.zeros(n, A + 1)),
                dict(logits=None, values=None, head=torch.zeros(n, A), num_actions=A),
                dict(logits=None, values=None, head=torch.zeros(n, A + 1))):
        args = dict(logits=l, values=v, actions=a, old_log_probs=f, advantages=f, returns=f)
        args.update(bad)
        with pytest.raises(ValueError):
            ppo.loss_and_grad(**args)
    for bad in (torch.zeros(1), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 2).t(), {}):
        with pytest.raises(ValueError):
            ppo.moments(bad)
    with pytest.raises(ValueError):
        ppo.moments(f, eps=-1.0)
    with pytest.raises(ValueError, match="out"):
        ppo.loss(l, v, a, f, f, f, out={})


# ---- the judge ------------------------------------------------------------------------------------------------------------
def value_of(case):
    return P.judge(case)["stats"]["loss"][0]


def small_case(A, value_clip, normalize):
    case = P.make_case(40, A, "float32", "float32", seed=21, value_clip=value_clip, normalize=normalize,
                       kinds=("random0.5", "random2", "equal"))
    for key in ("logits", "values"):
        case[key] = case[key].astype(np.float64)
    return case


@pytest.mark.parametrize("value_clip,normalize", [(0.0, False), (P.VALUE_CLIP, True)])
@pytest.mark.parametrize("A", J.A_EDGES)
def test_judge_gradients_equal_central_differences(A, value_clip, normalize):
    """d loss / d logits and d loss / d values of the judged alternative of every row, against central differences of the
    judged loss in float64 (h = 1e-5; the advantages, and with them their moments, are constants of the loss)"""
    case = small_case(A, value_clip, normalize)
    jd = P.judge(case)
    assert not jd["ambiguous"].any()
    rows = np.arange(40)
    analytic = np.where(jd["glp_k"][:, None] == 0, jd["grad_logits"][0], jd["grad_logits"][1])
    h = 1e-5
    for g in range(40):
        for i in list(range(A)) + [None]:
            up, down = dict(case), dict(case)
            key = "values" if i is None else "logits"
            step = np.zeros_like(case[key])
            step[(g,) if i is None else (g, i)] = h
            up[key], down[key] = case[key] + step, case[key] - step
            numeric = (value_of(up) - value_of(down)) / (2 * h)
            want = jd["grad_values"][g, jd["v_k"][g]] if i is None else analytic[g, i]
            assert abs(numeric - want) <= 1e-8, (g, i, numeric, want)
    assert (jd["glp_k"] == 1).sum() >= 1 and (jd["glp_k"] == 0).sum() >= 20  # both branches of g_lp are among the rows
    if value_clip > 0:
        # (alternative 1 -- the clipped loss chosen on an UNCLAMPED row -- is judged only where roundoff makes ec^2 > e^2)
        assert {0, 2} <= set(jd["v_k"][rows].tolist()) and (jd["v_k"] == 2).sum() >= 5


def torch_formulation(case):
    """The loss as a trainer writes it (CleanRL's ppo.py, its value clip included), torch CPU float64 under autograd:
    (the six statistics, d loss / d logits, d loss / d values)"""
    import torch

    t = lambda x: torch.tensor(np.asarray(x, np.float64))  # noqa: E731
    logits, values = t(case["logits"]).requires_grad_(True), t(case["values"]).requires_grad_(True)
    dist = torch.distributions.Categorical(logits=logits)
    newlogp, entropy = dist.log_prob(torch.tensor(case["actions"])), dist.entropy()
    logratio = newlogp - t(case["old_logp"])
    ratio = logratio.exp()
    adv = t(case["adv"])
    if case["normalize"]:
        adv = (adv - adv.mean()) / (adv.std() + P.f32(1e-8))
    clip, vclip = P.f32(case["clip"]), P.f32(case["value_clip"])
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    ret = t(case["ret"])
    v_unclipped = (values - ret) ** 2
    if vclip > 0:
        old_v = t(case["old_values"])
        v_clipped = old_v + torch.clamp(values - old_v, -vclip, vclip)
        v_loss = 0.5 * torch.max(v_unclipped, (v_clipped - ret) ** 2).mean()
    else:
        v_loss = 0.5 * v_unclipped.mean()
    ent = entropy.mean()
    loss = pg + P.f32(case["vf_coef"]) * v_loss - P.f32(case["ent_coef"]) * ent
    loss.backward()
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
        cf = ((ratio - 1.0).abs() > clip).double().mean()
    return [float(x.detach()) for x in (loss, pg, v_loss, ent, kl, cf)], logits.grad.numpy(), values.grad.numpy()


@pytest.mark.parametrize("value_clip,normalize", [(0.0, False), (P.VALUE_CLIP, True), (P.VALUE_CLIP, False)])
@pytest.mark.parametrize("A", J.A_EDGES)
def test_judge_equals_a_torch_formulation_under_autograd(A, value_clip, normalize):
    """torch.max, torch.clamp and CleanRL's value clip, and what autograd makes of them at float64: the judge's statistics
    and the gradients of its judged alternatives, to 1e-12 (rows without a masked logit: Categorical refuses none, but its
    entropy of one is NaN where the definition's is not)"""
    case = P.make_case(300, A, "float32", "float32", seed=22, value_clip=value_clip, normalize=normalize,
                       kinds=("random0.5", "random2", "random6", "equal", "plus80", "minus100"))
    jd = P.judge(case)
    stats, glogits, gvalues = torch_formulation(case)
    for name, have in zip(P.STAT_NAMES, stats):
        assert abs(have - jd["stats"][name][0]) <= 1e-12 * (1 + abs(have)), name
    rows = np.arange(300)
    quiet = ~jd["ambiguous"]
    assert quiet.sum() >= 297
    analytic = np.where(jd["glp_k"][:, None] == 0, jd["grad_logits"][0], jd["grad_logits"][1])
    assert np.allclose(glogits[quiet], analytic[quiet], rtol=0, atol=1e-13)
    assert np.allclose(gvalues[quiet], jd["grad_values"][rows, jd["v_k"]][quiet], rtol=0, atol=1e-13)
    assert 0.05 < stats[5] < 0.6  # the clip binds on some rows and not on others


@pytest.mark.parametrize("dtype", J.LOGIT_DTYPES)
@pytest.mark.parametrize("A", J.A_EDGES)
def test_float32_restatement_stays_within_the_derived_tolerances(A, dtype):
    """... on the very cases of tests/test_gpu_ppo.py, of which at most 1 % of the rows may be ambiguous by the float64 judge
    alone (the planted rows, listed by name, are the exception).  The worst share of a bound the restatement uses is
    printed, and must show the bounds neither tight by luck nor loose by orders of magnitude."""
    worst = {}
    for name, case, vdt, planted in ((f"{name} side {side}", case, vdt, planted) for name, cases, vdt, planted, _ in P.gpu_cases(A, dtype)
                                     for side, case in enumerate(cases)):
        jd = P.judge(case)
        amb = np.nonzero(jd["ambiguous"])[0]
        if planted:
            assert amb.tolist() == list(range(len(P.PLANTED))), (name, amb)
        else:
            assert amb.size <= 0.01 * jd["n"], (name, amb.size)
        res = P.compare(jd, P.restate_float32(case), dtype, vdt)
        assert not P.failures(res), (name, res)
        for key, (_, share) in res.items():
            worst[key] = max(worst.get(key, 0.0), share)
    print(f"A={A} {dtype}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1 for v in worst.values())
    assert worst["grad_logits"] >= 0.02 and worst["grad_values"] >= 0.02 and worst["value_loss"] >= 0.005 and worst["loss"] >= 0.001


def test_every_mutant_fails_on_a_committed_case():
    """each of the six mutants of ppo_judge.MUTANTS, applied to the float32 restatement, leaves the judge's bounds on the
    committed case n = 191, A = 18 (value clip and normalisation on); the restatement itself stays inside"""
    case = P.make_case(191, 18, "float32", "float32", seed=300)
    jd = P.judge(case)
    assert not P.failures(P.compare(jd, P.restate_float32(case)))
    told = {}
    for m in ("clip_on_the_wrong_side", "value_clip_gradient_kept", "entropy_sign_flipped", "mean_missing_from_value_gradient", "biased_variance"):
        told[m] = P.failures(P.compare(jd, P.restate_float32(case, m)))
        assert told[m], m
    assert "policy_loss" in told["clip_on_the_wrong_side"] and "grad_logits" in told["clip_on_the_wrong_side"]
    assert told["value_clip_gradient_kept"] == ["grad_values"] and told["mean_missing_from_value_gradient"] == ["grad_values"]
    assert "loss" in told["entropy_sign_flipped"] and "grad_logits" in told["entropy_sign_flipped"]
    assert "grad_logits" in told["biased_variance"]
    # the offset case: advantages = 1000 + noise of spread 1e-3.  The judged moments are those of the float32 values; a
    # sum of x^2 in float32 (1e6 per term, one part in 1.7e7 each) has lost the variance, 1e-6, entirely
    offset = P.moments_cases()["offset"]
    mean, rscale, t_mean, t_rs = P.moments(offset)
    assert abs(mean - 1000) < 1e-3 and 500 < rscale < 2000
    m32, r32 = P.restate_moments_float32(offset)
    assert abs(m32 - mean) <= t_mean and abs(r32 - rscale) <= t_rs
    m_naive, r_naive = P.restate_moments_float32(offset, mutant="naive_sum_of_squares")
    assert not abs(r_naive - rscale) <= t_rs
    told["naive_sum_of_squares"] = ["rscale"]
    mb, rb, _, _ = P.moments(offset, mutant="biased_variance")
    assert abs(rb - rscale) > t_rs
    assert sorted(told) == sorted(P.MUTANTS)


def test_judged_moments_equal_numpy_and_their_bounds_are_small():
    for name, x in P.moments_cases().items():
        mean, rscale, t_mean, t_rs = P.moments(x)
        x64 = x.astype(np.float64)
        assert abs(mean - x64.mean()) <= 1e-12 * (1 + abs(mean)), name
        if name != "constant":
            want = 1 / (x64.std(ddof=1) + P.f32(1e-8))
            assert abs(rscale - want) <= 1e-7 * want, name  # (the offset case: numpy's own two-pass value)
            assert t_rs <= 1.01 * J.U * rscale, name  # float64 sums: the float32 rounding of the result is all that is left
        else:
            assert rscale == 1 / P.f32(1e-8) and t_rs <= 1.01 * J.U * rscale
        assert t_mean <= 1.01 * J.U * abs(mean) + 1e-9, name  # (n * 2^-53 * mean |x - K|: 2e-10 at 1.2 million rows)
