"""CPU tests (no GPU needed) of the act library: libpikazoo_act.so exports its header's symbols and carries the tree's build
id, ``build()`` and ``needs_build()`` cover it without a twelfth entry in ``TARGETS``, nothing loads it before its first use,
its code object holds exactly six kernels without scratch or spilled vector registers, the entry point refuses bad arguments
before any launch and in the documented order, ``pikazoo_amd.act`` raises ``ValueError`` for malformed arguments before it
needs the library, and the judge of the GPU tests (tests/act_judge.py) passes the float32 restatement on the GPU test's own
cases within the cap on ambiguous rows and fails seven mutants of the seam between the net and the head."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import act_judge as AJ
import net_judge as N
import policy_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions
from test_net_host import declared_arguments

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_act_abi_version", "pz_act_build_id", "pz_mlp_act"]
KERNELS = sorted(f"pz_act::mlp_act_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1))


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def act_lib(pz_build):
    from pikazoo_amd import act

    return act.load()


def test_act_library_exports_exactly_its_header(pz_build, act_lib):
    from pikazoo_amd import _native, act, batch, league, learn, net, netgrad, optim, policy, pool, ppo

    assert header_functions("pikazoo_act.h") == NAMES == sorted(act.SIGNATURES) == dynamic_pz_symbols(pz_build.ACT_LIB)
    assert pz_build.library_id(pz_build.ACT_LIB) == pz_build.source_id() == act_lib.pz_act_build_id().decode()
    assert not pz_build.needs_build()
    # the twelfth library is walked by build() and needs_build() through ALL_TARGETS; TARGETS keeps its eleven entries
    assert len(pz_build.TARGETS) == 11 and pz_build.TARGETS[-1][0] == pz_build.LEAGUE_LIB
    assert pz_build.ACT_LIB not in [lib for lib, _ in pz_build.TARGETS]
    assert pz_build.ALL_TARGETS[:11] == pz_build.TARGETS and pz_build.ALL_TARGETS[11] == (pz_build.ACT_LIB, pz_build.ACT_SOURCES)
    assert pz_build.ACT_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_act.h") in pz_build.DEPS
    assert (pz_build.CSRC / "pz_mlp_tile.hpp") in pz_build.DEPS and (pz_build.CSRC / "pz_policy_rows.hpp") in pz_build.DEPS
    assert act_lib.pz_act_abi_version() == act.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_act.h").read_text()
    assert "#define PZ_ACT_ABI_VERSION 1" in header and f"#define PZ_ACT_MAX_ACTIONS {act.MAX_ACTIONS}" in header
    # no other library holds the entry point, and no older ABI version moved
    for other, _ in pz_build.TARGETS:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    assert _native.load().pz_abi_version() == 10
    assert net.load().pz_net_abi_version() == net.ABI_VERSION == 1 and policy.load().pz_policy_abi_version() == policy.ABI_VERSION == 1
    assert batch.load().pz_batch_abi_version() == batch.ABI_VERSION == 1 and pool.load().pz_pool_abi_version() == pool.ABI_VERSION == 1
    assert league.load().pz_league_abi_version() == league.ABI_VERSION == 1
    assert learn.load().pz_learn_abi_version() == learn.ABI_VERSION == 1 and ppo.load().pz_ppo_abi_version() == ppo.ABI_VERSION == 1
    assert netgrad.load().pz_netgrad_abi_version() == netgrad.ABI_VERSION == 1 and optim.load().pz_optim_abi_version() == optim.ABI_VERSION == 1
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_mlp_act")
    assert len(args) == 39 == len(act.SIGNATURES["pz_mlp_act"][1])
    assert declared_arguments(doc, "pz_mlp_act") == args
    assert "pikazoo_act.h" in doc and "libpikazoo_act.so" in doc
    # the binding's tables are the two older headers' enums, by value
    assert act.OBS_FORMATS is net.OBS_FORMATS and act.ACTIVATIONS is net.ACTIVATIONS and act.ACTION_FORMATS is policy.ACTION_FORMATS
    nh, ph = (REPO / "include" / "pikazoo_net.h").read_text(), (REPO / "include" / "pikazoo_policy.h").read_text()
    for table, prefix, text in ((act.OBS_FORMATS, "PZ_NET_OBS_", nh), (act.ACTIVATIONS, "PZ_NET_ACT_", nh), (act.ACTION_FORMATS, "PZ_POLICY_ACTION_", ph)):
        for key, value in table.items():
            name = prefix + (key if isinstance(key, str) else str(key).split(".")[-1]).upper()
            assert re.search(r"%s = %d\b" % (name, value), text), name


def test_importing_the_older_modules_does_not_load_the_act_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim, batch, pool, league; "
            "assert 'pikazoo_amd.act' not in sys.modules; m = net.ActorCritic(); import pikazoo_amd as p; assert 'act' in p.__all__; "
            "p.act.sample; assert 'pikazoo_amd.act' in sys.modules and p.act._lib is None; "
            "assert not any('libpikazoo_act' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_act_library(pz_build):
    """hidden width and activation are the compile-time choices, as in the net library: 3 x 2 kernels and nothing else; none
    uses scratch or spills a vector register; the LDS (the staged parameters and the four waves' images) is dynamic; the two
    narrower widths leave room for two waves per SIMD"""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.ACT_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.ACT_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0, (name, row)
        total = row[".vgpr_count"] + row.get(".agpr_count", 0)
        assert total <= (512 if "<128" in name else 256), (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


FAKE = 4096
ACT = dict(obs_p1=FAKE, obs_p2=FAKE, obs_format=2, n=8, in_features=35, obs_pitch=35, hidden=64, out_features=19, activation=0,
           w1_p1=FAKE, b1_p1=FAKE, w2_p1=FAKE, b2_p1=FAKE, w3_p1=FAKE, b3_p1=FAKE, w1_p2=FAKE, b1_p2=FAKE, w2_p2=FAKE, b2_p2=FAKE,
           w3_p2=FAKE, b3_p2=FAKE, num_actions=18, seed=7, first_game=0, step=0, step_dev=None, action_format=1, act_p1=FAKE, act_p2=FAKE,
           logp_p1=FAKE, logp_p2=FAKE, ent_p1=FAKE, ent_p2=FAKE, val_p1=FAKE, val_p2=FAKE, head_p1=FAKE, head_p2=FAKE, head_pitch=19,
           stream=None)
INPUTS_2 = ["obs_p2", "w1_p2", "b1_p2", "w2_p2", "b2_p2", "w3_p2", "b3_p2"]
OUTPUTS = ["act", "logp", "ent", "val", "head"]


def test_argument_validation(act_lib):
    """every check on fake pointers, in the header's order: a call that passes them all has n = 0 and launches nothing"""
    def call(**over):
        a = dict(ACT)
        assert not set(over) - set(a)
        a.update(over)
        return act_lib.pz_mlp_act(*a.values())

    side2 = {k: None for k in ACT if k.endswith("_p2")}
    assert len(side2) == 12 and list(ACT) == declared_arguments(re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_act.h").read_text(), flags=re.S), "pz_mlp_act")
    assert call(n=0) == 0 and call(n=0, **side2) == 0
    # NULL: agent 1's observations, parameters and actions; agent 2's inputs all or none; every output pair together
    for name in ["obs_p1", "w1_p1", "b1_p1", "w2_p1", "b2_p1", "w3_p1", "b3_p1", "act_p1"]:
        assert call(**{name: None}) == -1, name
    for name in INPUTS_2:
        assert call(**{name: None}) == -1, name
        assert call(**{other: None for other in INPUTS_2 if other != name}) == -1, name
    for out in OUTPUTS:
        assert call(**{out + "_p2": None}) == -1, out
        assert call(**{**side2, out + "_p2": FAKE}) == -1, out
        if out != "act":
            assert call(**{out + "_p1": None}) == -1, out           # (agent 2's is there, agent 1's is not)
            assert call(n=0, **{out + "_p1": None, out + "_p2": None}) == 0, out
    assert call(n=0, logp_p1=None, logp_p2=None, ent_p1=None, ent_p2=None, val_p1=None, val_p2=None, head_p1=None, head_p2=None) == 0
    # shared weights: agent 2's parameter pointers are agent 1's
    assert call(n=0, obs_p2=FAKE + 64) == 0
    # sizes: the net's box with 2 <= A <= 32 and A <= O <= 40
    assert call(n=-1) == -2 and call(n=(1 << 30) + 1) == -2
    assert call(in_features=0) == -2 and call(in_features=73, obs_pitch=80) == -2 and call(n=0, in_features=72, obs_pitch=72) == 0
    for hidden in (0, 16, 33, 96, 256, -64):
        assert call(hidden=hidden) == -2, hidden
    assert call(n=0, hidden=32) == 0 and call(n=0, hidden=128) == 0
    assert call(num_actions=1) == -2 and call(num_actions=33, out_features=40, head_pitch=40) == -2
    assert call(n=0, num_actions=32, out_features=33, head_pitch=33) == 0 and call(n=0, num_actions=2) == 0
    assert call(num_actions=20) == -2 and call(out_features=41, head_pitch=41) == -2 and call(n=0, out_features=40, head_pitch=40) == 0
    novalue = dict(val_p1=None, val_p2=None)
    assert call(num_actions=19) == -2 and call(n=0, num_actions=19, **novalue) == 0      # a value needs O > A
    assert call(obs_pitch=34) == -2 and call(obs_pitch=1 << 61) == -2 and call(head_pitch=18) == -2 and call(head_pitch=1 << 61) == -2
    assert call(n=0, head_pitch=18, head_p1=None, head_p2=None) == 0                       # (the pitch of a head that is not asked for)
    assert call(n=0, obs_pitch=36, head_pitch=20) == 0
    assert call(first_game=-1) == -2 and call(step=1 << 62) == -2 and call(n=0, step=(1 << 62) - 1, first_game=(1 << 62)) == 0
    # formats and the activation
    for name, count in (("obs_format", 5), ("activation", 2), ("action_format", 2)):
        assert call(**{name: count}) == -3 and call(**{name: -1}) == -3, name
        for value in range(count):
            assert call(n=0, **{name: value}) == 0, (name, value)
    # alignment to the element; step_dev and int64 actions to 8 bytes
    for name in (k for k in ACT if k.endswith(("_p1", "_p2"))):
        assert call(**{name: FAKE + 1}) == -4, name
        assert call(**{name: FAKE + 2}) == -4, name
        if name.startswith("obs"):
            assert call(n=0, obs_format=1, **{name: FAKE + 2}) == 0, name
        if name.startswith("act"):
            assert call(**{name: FAKE + 4}) == -4 and call(n=0, action_format=0, **{name: FAKE + 4}) == 0, name
        elif not name.startswith("obs"):
            assert call(n=0, **{name: FAKE + 4}) == 0, name
    assert call(step_dev=FAKE + 4) == -4 and call(n=0, step_dev=FAKE + 8) == 0
    # the order of the checks: NULL, size, config, alignment
    assert call(b3_p1=None, n=-1, activation=9, act_p1=FAKE + 2) == -1
    assert call(n=-1, activation=9, act_p1=FAKE + 2) == -2
    assert call(step=1 << 62, action_format=9, act_p1=FAKE + 2) == -2
    assert call(activation=9, act_p1=FAKE + 2) == -3
    assert call(act_p1=FAKE + 2) == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device and range errors raise ValueError -- on CPU tensors the device check stands behind the others --
    and none of them asks for the library"""
    import torch

    from pikazoo_amd import act, net

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(act, "load", refuse)
    n, K, H, O, A = 8, 35, 64, 19, 18
    good = [torch.zeros(H, K), torch.zeros(H), torch.zeros(H, H), torch.zeros(H), torch.zeros(O, H), torch.zeros(O)]
    x = torch.zeros(n, K)
    with pytest.raises(ValueError, match="GPU"):
        act.sample(x, good, A, seed=1)
    with pytest.raises(ValueError, match="GPU"):
        act.sample({"a": x, "b": x}, good, A, seed=1, step=5, activation="relu", action_dtype=torch.int32, head=True)
    with pytest.raises(ValueError, match="GPU"):
        net.ActorCritic().act_sample(x, seed=1)
    vectors = lambda dtype=torch.int64: dict(actions=torch.zeros(n, dtype=dtype), log_probs=torch.zeros(n), entropy=torch.zeros(n), values=torch.zeros(n))  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        act.sample(x, good, A, seed=1, out=vectors())
    bad_calls = [
        dict(obs=torch.zeros(n)), dict(obs=torch.zeros(n, 73)), dict(obs=torch.zeros(n, K, dtype=torch.float64)), dict(obs={}),
        dict(obs={"a": x, "b": torch.zeros(n + 1, K)}), dict(activation="gelu"), dict(params=good[:5]), dict(obs={"a": x}, params={"b": good}),
        dict(params=[torch.zeros(48, K)] + good[1:]), dict(params=good[:4] + [torch.zeros(41, H), torch.zeros(41)]),
        dict(num_actions=1), dict(num_actions=33), dict(num_actions=20), dict(seed=-1), dict(seed=1 << 64), dict(first_game=-1),
        dict(first_game=1 << 62), dict(step=-1), dict(step=1 << 62), dict(step=torch.zeros(2, dtype=torch.int64)),
        dict(step=torch.zeros(1, dtype=torch.int32)), dict(action_dtype=torch.int16), dict(out=vectors(torch.int32)),
        dict(out={k: v for k, v in vectors().items() if k != "values"}), dict(out=vectors(), head=True),
        dict(out={**vectors(), "head": torch.zeros(n, O)}), dict(out={**vectors(), "head": torch.zeros(n, O + 1)}, head=True),
        dict(out={**vectors(), "log_probs": torch.zeros(n + 1)}), dict(out={"a": vectors()}), dict(out=torch.zeros(n)),
    ]
    for bad in bad_calls:
        args = dict(obs=x, params=good, num_actions=A, seed=1)
        args.update(bad)
        with pytest.raises(ValueError):
            act.sample(**args)
    # without a value column "values" is no key of the result, and an `out` that holds it is refused
    flat = good[:4] + [torch.zeros(A, H), torch.zeros(A)]
    with pytest.raises(ValueError, match="keys"):
        act.sample(x, flat, A, seed=1, out=vectors())
    with pytest.raises(ValueError, match="GPU"):
        act.sample(x, flat, A, seed=1, out={k: v for k, v in vectors().items() if k != "values"})


# ---- the judge ----------------------------------------------------------------------------------------------------------------
def run_cases(mutant=None):
    """{case index: (ambiguous rows per side, failures)} of the restatement over the judge cases of tests/test_gpu_act.py"""
    out = {}
    for index, (n, size, activation, obs_dtype, draw_index) in enumerate(AJ.JUDGE_CASES):
        K, H, O, A = size
        obs, params = AJ.case_inputs(n, K, H, O, obs_dtype, seed=index)
        got = AJ.restate_float32(obs, params, activation, A, AJ.DRAWS[draw_index], mutant=mutant)
        us = AJ.uniforms(AJ.DRAWS[draw_index], n)
        amb, fails = [], []
        for s in (0, 1):
            count, f = AJ.verdict(got[s], obs[s], params[s], activation, A, us[s], what=f"case {index} side {s}")
            amb.append(count)
            fails += f
        out[index] = (amb, fails)
    return out


@pytest.fixture(scope="module")
def unmutated():
    return run_cases()


def test_the_restatement_passes_and_stays_inside_the_cap(unmutated):
    """the float32 chain of the two judges' restatements passes every check of the GPU test's judge cases; the share of
    ambiguous rows, expected at about 2 tau (A - 1) = 1e-4, stays within max(1, 1 % of n) for the fixed seeds"""
    for index, (amb, fails) in unmutated.items():
        n, size = AJ.JUDGE_CASES[index][:2]
        print(f"case {index} n = {n} {size}: ambiguous rows per side {amb}, share {max(amb) / n:.5f}, cap {AJ.CAP(n)}")
        assert not fails, fails
        assert max(amb) <= AJ.CAP(n)


def test_the_wide_pitch_case_has_no_ambiguous_row():
    """tests/test_gpu_wide_pitch.py runs the act launch on 40 rows; CAP(40) = 1 is a condition on the case, so the case is
    picked to need none of it: the restatement passes with zero ambiguous rows for both agents"""
    c = AJ.WIDE_CASE
    K, H, O, A = c["size"]
    obs, params = AJ.wide_case_inputs()
    got = AJ.restate_float32(obs, params, c["activation"], A, AJ.DRAWS[c["draw"]])
    us = AJ.uniforms(AJ.DRAWS[c["draw"]], c["n"])
    assert AJ.CAP(c["n"]) == 1
    for s in (0, 1):
        amb, fails = AJ.verdict(got[s], obs[s], params[s], c["activation"], A, us[s], what=f"wide case side {s}")
        print(f"wide case n = {c['n']} side {s}: {amb} ambiguous rows, share {amb / c['n']:.5f}")
        assert not fails and amb == 0, (s, amb, fails)
        assert len(set(got[s]["actions"].tolist())) > 4 and len(set(got[s]["actions"][-3:].tolist())) > 1   # (a draw worth judging)


@pytest.mark.parametrize("mutant", AJ.MUTANTS)
def test_every_mutant_is_caught_by_the_gpu_tests_cases(mutant):
    caught = {index: fails for index, (_, fails) in run_cases(mutant).items() if fails}
    print(mutant, "caught by the cases", sorted(caught), "--", next(iter(caught.values()))[0] if caught else "")
    assert caught, mutant
    if mutant not in ("first_game_ignored", "step_dev_ignored"):
        assert 0 in caught, (mutant, "the default case")


def test_the_composition_in_float64_agrees_with_the_restatement(unmutated):
    """judge() -- net_judge.judge followed by policy_judge.sample on ITS head -- and the float32 restatement return the same action
    wherever a row is unambiguous for both heads (the two heads differ by float32 roundoff, which moves a boundary by far less
    than tau except in rows one of them calls ambiguous)"""
    n, (K, H, O, A), activation, obs_dtype, draw_index = AJ.JUDGE_CASES[0]
    obs, params = AJ.case_inputs(n, K, H, O, obs_dtype, seed=0)
    got = AJ.restate_float32(obs, params, activation, A, AJ.DRAWS[draw_index])
    us = AJ.uniforms(AJ.DRAWS[draw_index], n)
    for s in (0, 1):
        head, tol, a, amb, st = AJ.judge(obs[s], params[s], activation, A, us[s])
        _, amb32, _, _ = J.sample(got[s]["head"][:, :A].astype(np.float64), us[s])
        agree = (got[s]["actions"] == a) | amb | amb32
        assert agree.mean() >= 0.999 and N.worst_share(got[s]["head"], head, tol)[0] <= 1


@pytest.mark.parametrize("b3_kind", AJ.PLANTED_B3)
def test_the_planted_rows_are_exact_in_float32(b3_kind):
    """the construction gives its logits exactly in float32 (net_judge's chain, index order and a drawn order), and holds every
    kind of row it promises"""
    K, H, O, A = AJ.SIZES[0]
    x, params, logits, kind, masked = AJ.planted(97, K, H, O, A, b3_kind)
    for order in (None, np.random.default_rng(4)):
        head = N.restate_float32(x, params, "relu", order=order)
        assert np.array_equal(head[:, :A], logits, equal_nan=True)
    assert set(kind) == set(AJ.FINITE_KINDS) | {"nan"}
    assert np.isnan(logits[np.array(kind) == "nan"]).all()
    if b3_kind in ("masked", "one_hot"):
        assert masked.any() and not masked.all() and (logits[np.array(kind) != "nan"][:, masked] == -np.inf).all()
        assert masked.sum() == (A - 1 if b3_kind == "one_hot" else masked.sum()) and (b3_kind == "one_hot" or masked[A - 1])
    if b3_kind == "plus_inf":
        assert (logits == np.inf).any(1)[np.array(kind) != "nan"].all()
