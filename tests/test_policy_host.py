"""CPU tests (no GPU needed) of the policy-head library: libpikazoo_policy.so exports its header's symbols and carries the
tree's build id, nothing loads it before its first use, its code object holds exactly the nine kernels of
``pz_policy::{sample,log_probs,backward}_kernel`` without scratch or spills, the three entry points refuse bad arguments
before any launch and in the documented order, and the judge the GPU tests compare with (tests/policy_judge.py) is the
definition: equal to a second formulation, to central differences, within its own derived tolerances of a float32
restatement, rarely ambiguous on the GPU tests' cases, and sharp enough that six mutants fail."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import policy_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_action_log_probs", "pz_action_log_probs_backward", "pz_policy_abi_version", "pz_policy_build_id", "pz_sample_actions"]


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def policy_lib(pz_build):
    from pikazoo_amd import policy

    return policy.load()


def declared_arguments(text, name):
    decl = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert decl, f"{name} is not shown"
    return [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]


def test_policy_library_exports_exactly_its_header(pz_build, policy_lib):
    from pikazoo_amd import _native, policy

    assert header_functions("pikazoo_policy.h") == NAMES == sorted(policy.SIGNATURES) == dynamic_pz_symbols(pz_build.POLICY_LIB)
    assert pz_build.library_id(pz_build.POLICY_LIB) == pz_build.source_id() == policy_lib.pz_policy_build_id().decode()
    assert not pz_build.needs_build()
    assert policy_lib.pz_policy_abi_version() == policy.ABI_VERSION == 1
    assert "#define PZ_POLICY_ABI_VERSION 1" in (REPO / "include" / "pikazoo_policy.h").read_text()
    # the product library did not move: its ABI, and none of the new names in it or in the learning library
    assert _native.load().pz_abi_version() == 10
    for other in (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB):
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    # INTEGRATION.md shows the three entry points as the header declares them (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_policy.h").read_text(), flags=re.S)
    for name, count in (("pz_sample_actions", 18), ("pz_action_log_probs", 14), ("pz_action_log_probs_backward", 17)):
        args = declared_arguments(header, name)
        assert len(args) == count == len(policy.SIGNATURES[name][1]), name
        assert declared_arguments(doc, name) == args, name
    assert "pikazoo_policy.h" in doc and "libpikazoo_policy.so" in doc


def test_importing_the_package_the_env_or_learn_does_not_load_the_policy_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; from pikazoo_amd import env, pikazoo_v0, learn; "
            "assert 'pikazoo_amd.policy' not in sys.modules; import pikazoo_amd as p; assert 'policy' in p.__all__; p.policy.sample; "
            "assert 'pikazoo_amd.policy' in sys.modules and p.policy._lib is None; "
            "assert not any('libpikazoo_policy' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_policy_library(pz_build):
    """The logit format is the one COMPILE-TIME choice: 3 launches x 3 formats = 9 kernels and nothing else in the code
    object.  None uses scratch or spills a register; each holds one wave's transposed image in LDS: 64 rows of 33 dwords."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    want = sorted(f"pz_policy::{kind}_kernel<{lf}>" for kind in ("sample", "log_probs", "backward") for lf in (0, 1, 2))
    table = kernel_digest.kernels(pz_build.POLICY_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == want
    assert all(count > 100 for name, (_, count) in table.items() if name in want)
    notes = kernel_notes.notes(pz_build.POLICY_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == want
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 64 * 33 * 4 and row[".vgpr_count"] <= 128, (name, row)


FAKE = 4096
SAMPLE = dict(logits_p1=FAKE, logits_p2=FAKE, logit_format=0, num_actions=18, n=8, logit_pitch=18, seed=7, first_game=0, step=0,
              step_dev=None, action_format=1, act_p1=FAKE, act_p2=FAKE, logp_p1=FAKE, logp_p2=FAKE, ent_p1=FAKE, ent_p2=FAKE, stream=None)
FORWARD = {k: v for k, v in SAMPLE.items() if k not in ("seed", "first_game", "step", "step_dev")}
BACKWARD = dict(logits_p1=FAKE, logits_p2=FAKE, logit_format=0, num_actions=18, n=8, logit_pitch=18, action_format=1, act_p1=FAKE,
                act_p2=FAKE, glogp_p1=FAKE, glogp_p2=FAKE, gent_p1=FAKE, gent_p2=FAKE, grad_p1=FAKE, grad_p2=FAKE, grad_pitch=18,
                stream=None)


def call(fn, defaults, **over):
    """an entry point on fake pointers (every check runs before the launch), both agents, n = 8, A = 18, pitch 18"""
    a = dict(defaults)
    assert not set(over) - set(a)
    a.update(over)
    return fn(*a.values())


def test_argument_validation(policy_lib):
    lib = policy_lib
    sample = lambda **o: call(lib.pz_sample_actions, SAMPLE, **o)  # noqa: E731
    forward = lambda **o: call(lib.pz_action_log_probs, FORWARD, **o)  # noqa: E731
    backward = lambda **o: call(lib.pz_action_log_probs_backward, BACKWARD, **o)  # noqa: E731
    one_side = dict(logits_p2=None, act_p2=None, logp_p2=None, ent_p2=None)
    for fn in (sample, forward):
        # NULL: the logits and the actions of agent 1; agent 2 all or none, and where agent 1 has the optional output
        assert fn(logits_p1=None) == -1 and fn(act_p1=None) == -1
        for name in one_side:
            assert fn(**{name: None}) == -1, name
            assert fn(**{other: None for other in one_side if other != name}) == -1, name
        assert fn(logp_p1=None) == -1 and fn(ent_p2=None) == -1
        # either optional pair may be NULL, and both
        assert fn(n=0, logp_p1=None, logp_p2=None) == 0 and fn(n=0, ent_p1=None, ent_p2=None) == 0
        assert fn(n=0, logp_p1=None, logp_p2=None, ent_p1=None, ent_p2=None) == 0 and fn(n=0, **one_side) == 0
        # sizes
        assert fn(n=-1) == -2 and fn(n=(1 << 30) + 1) == -2
        assert fn(num_actions=1, logit_pitch=18) == -2 and fn(num_actions=33, logit_pitch=40) == -2 and fn(num_actions=0) == -2
        assert fn(logit_pitch=17) == -2 and fn(logit_pitch=1 << 61) == -2
        assert fn(logit_pitch=((2 ** 63 - 1) // 4) // 8 + 1) == -2  # the first pitch whose 8 rows pass int64 in bytes
        assert fn(n=0, logit_pitch=((2 ** 63 - 1) // 4) // 8) == 0
        # formats
        assert fn(logit_format=3) == -3 and fn(logit_format=-1) == -3 and fn(action_format=2) == -3 and fn(action_format=-1) == -3
        # alignment to the element: logits 4 or 2, actions 4 or 8, floats 4
        for name in ("logits_p1", "logits_p2"):
            assert fn(**{name: FAKE + 2}) == -4 and fn(logit_format=1, **{name: FAKE + 1}) == -4, name
            assert fn(n=0, logit_format=2, **{name: FAKE + 2}) == 0, name
        for name in ("act_p1", "act_p2"):
            assert fn(**{name: FAKE + 4}) == -4 and fn(action_format=0, **{name: FAKE + 2}) == -4, name
            assert fn(n=0, action_format=0, **{name: FAKE + 4}) == 0, name
        for name in ("logp_p1", "logp_p2", "ent_p1", "ent_p2"):
            assert fn(**{name: FAKE + 2}) == -4, name
        # the order of the checks: NULL, size, config, alignment
        assert fn(logits_p1=None, n=-1, logit_format=9, act_p1=FAKE + 1) == -1
        assert fn(n=-1, logit_format=9, act_p1=FAKE + 1) == -2
        assert fn(logit_format=9, act_p1=FAKE + 1) == -3
        assert fn(act_p1=FAKE + 1) == -4
        assert fn(n=0) == 0
    # what only the sampling launch takes
    assert sample(first_game=-1) == -2 and sample(step=1 << 62) == -2 and sample(step=(1 << 64) - 1) == -2
    assert sample(n=0, step=(1 << 62) - 1, first_game=(1 << 62)) == 0
    assert sample(step_dev=FAKE + 4) == -4 and sample(n=0, step_dev=FAKE + 8) == 0
    assert sample(first_game=-1, logit_format=9) == -2 and sample(step=1 << 62, step_dev=FAKE + 4) == -2
    # the backward: the gradient and at least one upstream pair are required
    assert backward(n=0) == 0 and backward(n=0, logits_p2=None, act_p2=None, glogp_p2=None, gent_p2=None, grad_p2=None) == 0
    assert backward(n=0, glogp_p1=None, glogp_p2=None) == 0 and backward(n=0, gent_p1=None, gent_p2=None) == 0
    assert backward(glogp_p1=None, glogp_p2=None, gent_p1=None, gent_p2=None) == -1
    for name in ("logits_p1", "act_p1", "grad_p1", "logits_p2", "act_p2", "grad_p2", "glogp_p1", "glogp_p2", "gent_p1", "gent_p2"):
        assert backward(**{name: None}) == -1, name
    assert backward(grad_pitch=17) == -2 and backward(logit_pitch=17) == -2 and backward(grad_pitch=1 << 61) == -2
    assert backward(n=-1) == -2 and backward(num_actions=33, logit_pitch=40, grad_pitch=40) == -2
    assert backward(logit_format=3) == -3 and backward(action_format=2) == -3
    for name in ("glogp_p1", "glogp_p2", "gent_p1", "gent_p2", "grad_p1", "grad_p2", "logits_p2"):
        assert backward(**{name: FAKE + 2}) == -4, name
    assert backward(logit_format=1, grad_p1=FAKE + 1) == -4 and backward(n=0, logit_format=1, grad_p1=FAKE + 2) == 0
    assert backward(grad_p1=None, grad_pitch=17, logit_format=3, act_p1=FAKE + 1) == -1
    assert backward(grad_pitch=17, logit_format=3, act_p1=FAKE + 1) == -2
    assert backward(logit_format=3, act_p1=FAKE + 1) == -3


def test_python_errors_come_before_any_launch():
    """shape, dtype, device and range errors raise ValueError -- on CPU tensors the device check is the last one standing,
    so everything before it is reachable here"""
    import torch

    from pikazoo_amd import policy

    l = torch.zeros(8, 18)
    with pytest.raises(ValueError, match="GPU"):
        policy.sample(l, seed=1)
    with pytest.raises(ValueError, match="GPU"):
        policy.log_probs(l, torch.zeros(8, dtype=torch.int64))
    for bad in (torch.zeros(8), torch.zeros(8, 1), torch.zeros(8, 33), torch.zeros(8, 18, dtype=torch.float64),
                torch.zeros(18, 8).t(), {}, {"player_1": l, "player_2": torch.zeros(8, 13)},
                {"player_1": l, "player_2": torch.zeros(8, 19)[:, :18]}, [l]):
        with pytest.raises(ValueError):
            policy.sample(bad, seed=1)


# ---- the judge ------------------------------------------------------------------------------------------------------------
def second_formulation(l, u):
    """independent of policy_judge.stats: log_softmax by logsumexp, the draw by searchsorted on the normalised CDF"""
    l = np.asarray(l, np.float64)
    n, A = l.shape
    act, logp, ent = np.zeros(n, np.int64), np.zeros((n, A)), np.zeros(n)
    for g in range(n):
        row = l[g]
        lse = row.max() + np.log(np.exp(row - row.max()).sum())
        ls = row - lse
        logp[g] = ls
        pr = np.exp(ls)
        ent[g] = -sum(pr[i] * ls[i] for i in range(A) if pr[i] > 0)
        cdf = np.cumsum(pr)
        a = int(np.searchsorted(cdf[:A - 1], u[g], side="right"))
        alive = np.nonzero(pr > 0)[0]
        act[g] = min(a, alive[-1])
    return act, logp, ent


@pytest.mark.parametrize("A", J.A_EDGES)
def test_judge_equals_a_second_formulation(A):
    kinds = tuple(k for k in J.ROW_KINDS if k not in ("nan", "plus_inf", "all_minus_inf"))
    l, kind = J.make_rows(600, A, "float32", seed=11, kinds=kinds)
    u = J.uniforms(3, 17, 5, None, 600)[0]
    a, amb, nb, st = J.sample(l, u)
    a2, logp2, ent2 = second_formulation(l, u)
    assert np.array_equal(a[~amb], a2[~amb]) and ((a2 >= nb[:, 0]) & (a2 <= nb[:, 1])).all()
    logp, _ = J.log_prob(st, a)
    assert np.allclose(logp, logp2[np.arange(600), a], rtol=0, atol=1e-12 * (1 + np.abs(logp)))
    assert np.allclose(st["H"], ent2, rtol=0, atol=1e-12)
    # what the row kinds promise
    k = np.array(kind)
    assert np.allclose(st["H"][k == "equal"], np.log(A), atol=1e-12) and np.allclose(logp[k == "equal"], -np.log(A), atol=1e-12)
    assert (st["H"][k == "one_hot"] == 0).all() and (logp[k == "one_hot"] == 0).all()
    assert (np.isfinite(l[np.arange(600), a])).all()  # a masked action is never drawn
    # step 6
    bad, _ = J.make_rows(30, A, "float32", seed=12, kinds=("nan", "plus_inf", "all_minus_inf"))
    a, amb, nb, st = J.sample(bad, J.uniforms(3, 0, 0, None, 30)[1])
    assert (a == 0).all() and not amb.any() and np.isnan(st["H"]).all() and np.isnan(J.log_prob(st, a)[0]).all()
    # an action outside [0, A): a NaN log-prob, a valid entropy
    good, _ = J.make_rows(4, A, "float32", seed=13, kinds=("random2",))
    st = J.stats(good)
    assert np.isnan(J.log_prob(st, [-1, A, 0, A - 1])[0]).tolist() == [True, True, False, False] and np.isfinite(st["H"]).all()


@pytest.mark.parametrize("A", J.A_EDGES)
def test_judge_gradient_equals_central_differences(A):
    rng = np.random.default_rng(A)
    l, _ = J.make_rows(40, A, "float32", seed=14, kinds=("random0.5", "random2", "equal"))
    l = l.astype(np.float64)
    a = rng.integers(0, A, 40)
    glogp, gent = rng.normal(size=40), rng.normal(size=40)

    def value(x):
        st = J.stats(x)
        return glogp * J.log_prob(st, a)[0] + gent * st["H"]

    grad, _ = J.gradient(J.stats(l), a, glogp, gent)
    h = 1e-5
    for i in range(A):
        step = np.zeros_like(l)
        step[:, i] = h
        numeric = (value(l + step) - value(l - step)) / (2 * h)
        assert np.allclose(grad[:, i], numeric, rtol=0, atol=1e-8), i
    # a masked logit gets no gradient, not a NaN; an out-of-range action no [i == a] term
    m, _ = J.make_rows(20, A, "float32", seed=15, kinds=("masked_tail", "one_hot"))
    st = J.stats(m)
    grad, tol = J.gradient(st, st["last"], np.ones(20), np.ones(20))
    assert np.isfinite(grad).all() and np.isfinite(tol).all() and (grad[~st["live"]] == 0).all()
    out, _ = J.gradient(J.stats(l), np.full(40, A), glogp, np.zeros(40))
    assert np.allclose(out, -glogp[:, None] * J.stats(l)["p"])


def sampling_cases(A, dtype):
    for n in J.N_EDGES:
        for index, draw in enumerate(J.DRAWS):
            yield n, index, draw, J.case_logits(n, A, dtype, index), J.uniforms(*draw, n)


@pytest.mark.parametrize("dtype", J.LOGIT_DTYPES)
@pytest.mark.parametrize("A", J.A_EDGES)
def test_float32_restatement_stays_within_the_derived_tolerances(A, dtype):
    """... on the very cases of tests/test_gpu_policy.py, of which at most 0.2 % may be ambiguous (a condition on the judge
    alone).  The restatement agrees on every unambiguous action, returns a live action between the neighbours on the
    others, and its log-prob and entropy stay within the tolerances -- by a margin that shows they are not tight by luck
    (numpy's exp and log, not the device's) and not loose by orders of magnitude."""
    rows = ambiguous = 0
    worst_logp = worst_ent = 0.0
    for n, index, draw, logits, us in sampling_cases(A, dtype):
        for side in (0, 1):
            l, _ = logits[side]
            a, amb, nb, st = J.sample(l, us[side])
            a32, logp32, ent32 = J.restate_float32(l, us[side])
            rows += n
            ambiguous += int(amb.sum())
            assert np.array_equal(a32[~amb], a[~amb])
            assert ((a32 >= nb[:, 0]) & (a32 <= nb[:, 1]) & (st["live"][np.arange(n), a32] | st["bad"])).all()
            logp, tol = J.log_prob(st, a32)
            good = ~st["bad"]
            assert np.array_equal(np.isnan(logp32), ~good) and np.array_equal(np.isnan(ent32), ~good)
            assert (np.abs(logp32 - logp)[good] <= tol[good]).all()
            tol_ent = J.entropy_tolerance(st)
            assert (np.abs(ent32 - st["H"])[good] <= tol_ent[good]).all()
            if good.any():
                worst_logp = max(worst_logp, float((np.abs(logp32 - logp)[good] / tol[good]).max()))
                worst_ent = max(worst_ent, float((np.abs(ent32 - st["H"])[good] / tol_ent[good]).max()))
    print(f"A={A} {dtype}: {rows} rows, {ambiguous} ambiguous, worst error / tolerance: logp {worst_logp:.3f}, entropy {worst_ent:.3f}")
    assert ambiguous <= 0.002 * rows
    assert 0.02 <= worst_logp <= 1 and 0.02 <= worst_ent <= 1


@pytest.mark.parametrize("A", J.A_EDGES)
def test_ambiguous_share_on_many_random_rows(A):
    """50 000 normal rows at each of the scales 0.5, 2 and 6: at most 0.2 % ambiguous, and the float32 restatement agrees
    with float64 on every other action"""
    rng = np.random.default_rng(A)
    n = 50_000
    for scale in (0.5, 2.0, 6.0):
        l = rng.normal(0.0, scale, (n, A)).astype(np.float32)
        u = J.uniforms(int(scale * 10), 0, 3, None, n)[0]
        a, amb, nb, st = J.sample(l, u)
        a32, logp32, _ = J.restate_float32(l, u)
        print(f"A={A} scale {scale}: {int(amb.sum())} of {n} ambiguous, largest tau {J.tau(st).max() * 2 ** 23:.1f} * 2^-23")
        assert amb.sum() <= 0.002 * n and np.array_equal(a[~amb], a32[~amb])
        assert (J.tau(st) <= (A + 5.5 + np.log(A)) * 2.0 ** -23 * (1 + 1e-12)).all()  # (2 EXP_ULP + A - 1 + q + 1/2, q <= log A)


def test_the_largest_u_and_the_clamp():
    """The committed pair of game ids draws the largest u there is, 1 - 2^-24, on rows with a masked tail.  The clamp of
    step 4 is a guard that correct rounding never needs: u * S = S - S 2^-24 lies at least as far from S as from the
    float below S (S = 1.f 2^e: S 2^-24 = 1.f 2^(e-24) >= (2 - 1.f) 2^(e-24)), so the rounded threshold stays below S, no
    c_i that equals S is ever counted, and the action found is one whose e_i raised the sum.  Hence float64, the float32
    restatement and the restatement WITHOUT the clamp agree here -- the one mutant that nothing can tell apart."""
    for side in (0, 1):
        for A in J.A_EDGES[1:]:
            l, first = J.largest_u_case(A, "float32", side)
            u = J.uniforms(J.LARGEST_U["seed"], first, J.LARGEST_U["step"], None, 64)[side]
            assert u[5] == 1 - 2.0 ** -24
            a, amb, _, st = J.sample(l, u)
            assert a[5] == st["last"][5] and st["last"][5] < A - 1 and not amb[5]
            assert (np.float32(u[5]) * st["S"].astype(np.float32) < st["S"].astype(np.float32)).all()
            for mutant in (None, "clamp_dropped"):
                a32 = J.restate_float32(l, u, mutant=mutant)[0]
                assert np.array_equal(a32[~amb], a[~amb]) and a32[5] == a[5]
            assert np.array_equal(J.sample(l, u, mutant="clamp_dropped")[0], a)


def test_every_mutant_fails_on_the_committed_cases():
    """... every mutant that CAN fail: five do, on most rows they touch; dropping the clamp changes no action at all."""
    A, n = 18, 191
    index, draw = 2, J.DRAWS[2]  # (the draw with a first game and a device part of the step)
    logits = J.case_logits(n, A, "float32", index)
    us = J.uniforms(*draw, n)
    told = {}
    for m in ("words_swapped", "first_game_ignored", "step_dev_ignored"):
        um = J.uniforms(*draw, n, mutant=m)
        assert not np.array_equal(um, us)
        a, amb, nb, _ = J.sample(logits[0][0], us[0])
        am = J.sample(logits[0][0], um[0])[0]
        told[m] = int(((am != a) & ~amb).sum())
        assert told[m] > n // 4, m  # most rows draw another action
    assert np.array_equal(J.uniforms(*draw, n, mutant="words_swapped")[0], us[1])
    # the max not subtracted: logits near 100 overflow float32's exp (those near 80 do not: exp(80) = 5.5e34)
    l, kind = logits[0]
    rows = np.array(kind) == "plus100"
    st, stm = J.stats(l), J.stats(l, mutant="max_not_subtracted")
    assert np.isfinite(st["H"][rows]).all() and not np.isfinite(stm["H"][rows]).any()
    told["max_not_subtracted"] = int(rows.sum())
    # the entropy's sign
    stm = J.stats(l, mutant="entropy_sign_flipped")
    good = ~st["bad"] & (st["q"] > 1e-3)
    assert good.sum() > n // 2 and (np.abs(stm["H"] - st["H"])[good] > 100 * J.entropy_tolerance(st)[good]).all()
    told["entropy_sign_flipped"] = int(good.sum())
    # the clamp dropped: equal to the judge everywhere (test_the_largest_u_and_the_clamp says why) -- listed, and blind
    for side in (0, 1):
        assert np.array_equal(J.sample(logits[side][0], us[side], mutant="clamp_dropped")[0], J.sample(logits[side][0], us[side])[0])
    told["clamp_dropped"] = 0
    assert sorted(told) == sorted(J.MUTANTS)


def test_rounding_to_the_formats():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3, 65504.0, 1e-9, np.nan])
    r, ulp = J.round_to(x, "bfloat16")
    assert r[0] == 1 and r[1] == 1 and r[2] == 1 + 2.0 ** -6 and ulp[0] == 2.0 ** -7 and np.isnan(r[6])  # ties to even
    r, ulp = J.round_to(x, "float16")
    assert r[4] == 65504 and ulp[0] == 2.0 ** -10 and ulp[5] == 2.0 ** -24
    for dtype in J.LOGIT_DTYPES:
        v = J.as_logit_dtype(np.array([0.1, -7.3, 80.2, -np.inf], np.float32), dtype)
        assert np.array_equal(J.bits_to_float(J.logit_bits(v, dtype), dtype), v)
