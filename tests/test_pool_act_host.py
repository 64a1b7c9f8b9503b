"""CPU tests (no GPU needed) of the pool-act library: libpikazoo_pool_act.so exports its header's symbols and carries the tree's
build id, it is the thirteenth entry of ``ALL_TARGETS`` with ``TARGETS`` untouched, nothing loads it before its first use, its
code object holds exactly six kernels without scratch or spilled vector registers, the entry point refuses bad arguments
before any launch and in the documented order, ``pikazoo_amd.pool_act`` raises ``ValueError`` for malformed arguments before it
needs the library, and the judge of the GPU tests (tests/pool_act_judge.py) agrees in its two formulations on every case of
the GPU test, passes the float32 restatement within the cap on ambiguous rows and fails seven mutants on those cases.

No call here ever passes every check with rows to run: a call that passes them all has n = 0 and launches nothing."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import act_judge as AJ
import net_judge as N
import policy_judge as J
import pool_act_judge as PA
import pool_judge as PJ
from test_cabi_and_host import dynamic_pz_symbols, header_functions
from test_net_host import declared_arguments
from test_pool_host import FAKE, member_array

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_mlp_act_pool", "pz_pool_act_abi_version", "pz_pool_act_build_id"]
KERNELS = sorted(f"pz_pool_act::mlp_act_pool_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1))
HOST_ROWS = 5000   # the two re-staging cases are left to the GPU where a mutant has to be played on every case


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.pool_act, the judge's included: none of them runs without the module"""
    from pikazoo_amd import pool_act

    return pool_act


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import pool_act

    return pool_act.load()


def test_pool_act_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, act, net, policy, pool, pool_act

    assert header_functions("pikazoo_pool_act.h") == NAMES == sorted(pool_act.SIGNATURES) == dynamic_pz_symbols(pz_build.POOL_ACT_LIB)
    assert pz_build.library_id(pz_build.POOL_ACT_LIB) == pz_build.source_id() == lib.pz_pool_act_build_id().decode()
    assert not pz_build.needs_build()
    # the thirteenth library: ALL_TARGETS[12]; TARGETS keeps its eleven entries and ALL_TARGETS[11] stays the act library
    assert len(pz_build.TARGETS) == 11 and pz_build.TARGETS[-1][0] == pz_build.LEAGUE_LIB
    assert len(pz_build.ALL_TARGETS) == 13 and pz_build.ALL_TARGETS[:11] == pz_build.TARGETS
    assert pz_build.ALL_TARGETS[11] == (pz_build.ACT_LIB, pz_build.ACT_SOURCES)
    assert pz_build.ALL_TARGETS[12] == (pz_build.POOL_ACT_LIB, pz_build.POOL_ACT_SOURCES)
    assert pz_build.POOL_ACT_LIB.name == "libpikazoo_pool_act.so" and pz_build.POOL_ACT_SOURCES == [pz_build.CSRC / "pz_pool_act.hip"]
    assert pz_build.POOL_ACT_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_pool_act.h") in pz_build.DEPS
    for lib_path, _ in pz_build.ALL_TARGETS:
        assert pz_build.library_id(lib_path) == pz_build.source_id(), lib_path
    assert lib.pz_pool_act_abi_version() == pool_act.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_pool_act.h").read_text()
    assert "#define PZ_POOL_ACT_ABI_VERSION 1" in header and f"#define PZ_POOL_ACT_MAX_ACTIONS {pool_act.MAX_ACTIONS}" in header
    # no other library holds the entry point, and the two libraries it stands beside kept their exports and versions
    for other, _ in pz_build.ALL_TARGETS[:12]:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    assert pool.load().pz_pool_abi_version() == pool.ABI_VERSION == 1 and act.load().pz_act_abi_version() == act.ABI_VERSION == 1
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_mlp_act_pool")
    assert len(args) == 33 == len(pool_act.SIGNATURES["pz_mlp_act_pool"][1]) and args == list(POOL_ACT)
    assert declared_arguments(doc, "pz_mlp_act_pool") == args
    assert "pikazoo_pool_act.h" in doc and "libpikazoo_pool_act.so" in doc
    # the binding's tables and struct are the older bindings' own
    assert pool_act.OBS_FORMATS is net.OBS_FORMATS and pool_act.ACTIVATIONS is net.ACTIVATIONS and pool_act.ACTION_FORMATS is policy.ACTION_FORMATS
    assert pool_act.Member is pool.Member and pool_act.MAX_MEMBERS == pool.MAX_MEMBERS == 16 and pool_act.MAX_ACTIONS == act.MAX_ACTIONS


def test_importing_the_older_modules_does_not_load_the_pool_act_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim, batch, pool, league, act; "
            "assert 'pikazoo_amd.pool_act' not in sys.modules; m = net.ActorCritic(); s = pool.Snapshots(m, 3); s.act_sample; "
            "assert 'pikazoo_amd.pool_act' not in sys.modules; import pikazoo_amd as p; assert 'pool_act' in p.__all__; "
            "p.pool_act.sample; assert 'pikazoo_amd.pool_act' in sys.modules and p.pool_act._lib is None; "
            "assert not any('libpikazoo_pool_act' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_pool_act_library(pz_build):
    """hidden width and activation are the compile-time choices, as in the net library: 3 x 2 kernels and nothing else; none
    uses scratch or spills a vector register -- the 16 members' pointers are indexed in the kernel arguments --; the LDS (the
    staged parameters, the words of `first` and the four waves' images) is dynamic; the two narrower widths leave room for two
    waves per SIMD"""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.POOL_ACT_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.POOL_ACT_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0, (name, row)
        total = row[".vgpr_count"] + row.get(".agpr_count", 0)
        assert total <= (512 if "<128" in name else 256), (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


# ---- argument checking ----------------------------------------------------------------------------------------------------------
POOL_ACT = dict(obs_p1=FAKE, obs_p2=FAKE, obs_format=2, n=8, in_features=35, obs_pitch=35, hidden=64, out_features=19, activation=0, members=None,
                num_members=3, order_p1=FAKE, first_p1=FAKE, order_p2=FAKE, first_p2=FAKE, num_actions=18, seed=7, first_game=0, step=0,
                step_dev=None, action_format=1, act_p1=FAKE, act_p2=FAKE, logp_p1=FAKE, logp_p2=FAKE, ent_p1=FAKE, ent_p2=FAKE, val_p1=FAKE,
                val_p2=FAKE, head_p1=FAKE, head_p2=FAKE, head_pitch=19, stream=None)
OPTIONAL = ["logp", "ent", "val", "head"]


def test_argument_validation(lib):
    """every return code on fake pointers, in the header's order: NULL, the number of members, NULL of a member, size, config,
    alignment; a call that passes them all has n = 0 and launches nothing"""
    def call(members="good", **over):
        a = dict(POOL_ACT)
        assert not set(over) - set(a)
        a.update(over)
        a["members"] = member_array(max(1, min(a["num_members"], 16))) if isinstance(members, str) else members
        return lib.pz_mlp_act_pool(*a.values())

    side2 = {k: None for k in POOL_ACT if k.endswith("_p2")}
    assert len(side2) == 8
    assert call(n=0) == 0 and call(n=0, **side2) == 0 and call(n=0, num_members=1) == 0 and call(n=0, num_members=16) == 0
    assert call(n=0, order_p1=None, first_p1=None) == 0 and call(n=0, order_p1=None) == 0 and call(n=0, order_p2=None, first_p2=None) == 0
    # NULL: agent 1's observations and actions, the member array; agent 2's observations and actions together
    for name in ("obs_p1", "act_p1"):
        assert call(**{name: None}) == -1, name
    assert call(members=None) == -1
    assert call(obs_p2=None) == -1 and call(act_p2=None) == -1
    for name in side2:                                                 # an absent agent 2 has nothing at all
        if name not in ("obs_p2", "act_p2"):
            assert call(**{**side2, name: FAKE}) == -1, name
    # the optional outputs are optional per agent, each on its own -- unlike pz_mlp_act's
    for out in OPTIONAL:
        for gone in ([out + "_p1"], [out + "_p2"], [out + "_p1", out + "_p2"]):
            assert call(n=0, **{name: None for name in gone}) == 0, gone
    league = {out + "_p2": None for out in OPTIONAL}
    assert call(n=0, **league) == 0 and call(n=0, **{out + "_p1": None for out in OPTIONAL}) == 0
    assert call(n=0, **{out + s: None for out in OPTIONAL for s in ("_p1", "_p2")}) == 0
    # P out of range, before a member is looked at
    for P in (0, -1, 17, 1 << 20):
        assert call(num_members=P) == -2, P
        assert call(num_members=P, members=member_array(3, m0=dict(w1=None))) == -2, P
    # a NULL member pointer; first NULL while order is not; both in front of the sizes
    for i in (0, 2):
        for field in ("w1", "b1", "w2", "b2", "w3", "b3"):
            assert call(members=member_array(3, **{f"m{i}": {field: None}})) == -1, (i, field)
    assert call(n=0, members=member_array(3, m3=dict(w1=None))) == 0                                  # behind P: not looked at
    assert call(first_p1=None) == -1 and call(first_p2=None) == -1
    assert call(members=member_array(3, m1=dict(b2=None)), n=-1) == -1 and call(first_p1=None, hidden=48) == -1
    # sizes: the net's box with 2 <= A <= 32 and A <= O <= 40
    assert call(n=-1) == -2 and call(n=(1 << 30) + 1) == -2
    assert call(in_features=0) == -2 and call(in_features=73, obs_pitch=80) == -2 and call(n=0, in_features=72, obs_pitch=72) == 0
    for hidden in (0, 16, 33, 96, 256, -64):
        assert call(hidden=hidden) == -2, hidden
    assert call(n=0, hidden=32) == 0 and call(n=0, hidden=128) == 0
    assert call(num_actions=1) == -2 and call(num_actions=33, out_features=40, head_pitch=40) == -2
    assert call(n=0, num_actions=32, out_features=33, head_pitch=33) == 0 and call(n=0, num_actions=2) == 0
    assert call(num_actions=20) == -2 and call(out_features=41, head_pitch=41) == -2 and call(n=0, out_features=40, head_pitch=40) == 0
    # a value needs O > A, whichever agent asks for it
    assert call(num_actions=19) == -2 and call(num_actions=19, val_p1=None) == -2 and call(num_actions=19, val_p2=None) == -2
    assert call(n=0, num_actions=19, val_p1=None, val_p2=None) == 0
    assert call(obs_pitch=34) == -2 and call(obs_pitch=1 << 61) == -2 and call(head_pitch=18) == -2 and call(head_pitch=1 << 61) == -2
    assert call(head_pitch=18, head_p1=None) == -2 and call(head_pitch=18, head_p2=None) == -2            # one head is enough to need the pitch
    assert call(n=0, head_pitch=18, head_p1=None, head_p2=None) == 0                                      # (the pitch of a head nobody asks for)
    assert call(n=0, obs_pitch=36, head_pitch=20) == 0
    assert call(first_game=-1) == -2 and call(step=1 << 62) == -2 and call(n=0, step=(1 << 62) - 1, first_game=(1 << 62)) == 0
    # formats and the activation
    for name, count in (("obs_format", 5), ("activation", 2), ("action_format", 2)):
        assert call(**{name: count}) == -3 and call(**{name: -1}) == -3, name
        for value in range(count):
            assert call(n=0, **{name: value}) == 0, (name, value)
    # alignment to the element; step_dev and int64 actions to 8 bytes
    for name in (k for k in POOL_ACT if k.endswith(("_p1", "_p2"))):
        assert call(**{name: FAKE + 1}) == -4, name
        assert call(**{name: FAKE + 2}) == -4, name
        if name.startswith("obs"):
            assert call(n=0, obs_format=1, **{name: FAKE + 2}) == 0, name
        if name.startswith("act"):
            assert call(**{name: FAKE + 4}) == -4 and call(n=0, action_format=0, **{name: FAKE + 4}) == 0, name
        elif not name.startswith("obs"):
            assert call(n=0, **{name: FAKE + 4}) == 0, name
    assert call(step_dev=FAKE + 4) == -4 and call(n=0, step_dev=FAKE + 8) == 0
    for field in ("w1", "b3"):
        assert call(members=member_array(3, m2={field: FAKE + 2})) == -4, field
    assert call(n=0, members=member_array(3, m2=dict(w1=FAKE + 8))) == 0
    # the order of the checks
    broken = member_array(3, m1=dict(w3=None))
    assert call(members=broken, act_p1=None, num_members=0, n=-1, activation=9) == -1
    assert call(members=broken, num_members=17, n=-1, activation=9, act_p2=FAKE + 2) == -2
    assert call(members=broken, n=-1, activation=9, act_p2=FAKE + 2) == -1
    assert call(n=-1, activation=9, act_p2=FAKE + 2) == -2
    assert call(step=1 << 62, action_format=9, act_p2=FAKE + 2) == -2
    assert call(activation=9, act_p2=FAKE + 2) == -3
    assert call(act_p2=FAKE + 2) == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device and range errors raise ValueError -- on CPU tensors the device check stands behind the others --
    and none of them asks for the library"""
    import torch

    from pikazoo_amd import net, pool, pool_act

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(pool_act, "load", refuse)
    n, K, H, O, A, P = 8, 35, 64, 19, 18, 3
    one = lambda: [torch.zeros(H, K), torch.zeros(H), torch.zeros(H, H), torch.zeros(H), torch.zeros(O, H), torch.zeros(O)]  # noqa: E731
    good = [one() for _ in range(P)]
    x = torch.zeros(n, K)
    two = {"a": x, "b": torch.zeros(n, K)}

    def a_plan(rows=n, count=P, **over):
        fields = dict(order=torch.zeros(pool.capacity(rows, count), dtype=torch.int32), first=torch.zeros(count + 1, dtype=torch.int32),
                      errors=torch.zeros(1, dtype=torch.int32), n=rows, num_members=count)
        fields.update(over)
        return pool.Plan(**fields)

    both = {"a": None, "b": a_plan()}
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(x, good, a_plan(), A, seed=1)
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(two, good, both, A, seed=1, step=5, activation="relu", action_dtype=torch.int32, stats={"a"}, head={"b"})
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(x, good[:1], None, A, seed=1, stats=False, head=True)
    with pytest.raises(ValueError, match="GPU"):
        pool.Snapshots(net.ActorCritic(), 3).act_sample(two, {"a": None, "b": a_plan(count=1)}, seed=1, step=2, stats=["a"])
    vec = lambda dtype=torch.int64: dict(actions=torch.zeros(n, dtype=dtype), log_probs=torch.zeros(n), entropy=torch.zeros(n), values=torch.zeros(n))  # noqa: E731
    league_out = dict(actions={"a": torch.zeros(n, dtype=torch.int64), "b": torch.zeros(n, dtype=torch.int64)}, log_probs={"a": torch.zeros(n)},
                      entropy={"a": torch.zeros(n)}, values={"a": torch.zeros(n)})
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(x, good, a_plan(), A, seed=1, out=vec())
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(two, good, both, A, seed=1, stats={"a"}, out=league_out)
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(two, good, both, A, seed=1, stats={"a"}, head={"b"}, out={**league_out, "head": {"b": torch.zeros(n, O)}})

    def swapped(m, i, t):
        return [[t if (mm, j) == (m, i) else p for j, p in enumerate(ps)] for mm, ps in enumerate(good)]

    bad_calls = [
        dict(obs=torch.zeros(n)), dict(obs=torch.zeros(n, 73)), dict(obs=torch.zeros(n, K, dtype=torch.float64)), dict(obs={}),
        dict(obs={"a": x, "b": torch.zeros(n + 1, K)}, plans={"a": None, "b": None}), dict(activation="gelu"),
        dict(member_params=[]), dict(member_params=[one() for _ in range(17)], plans=None), dict(member_params=one()[0]),
        dict(member_params=[one()[:5]] * 3), dict(member_params=swapped(0, 0, torch.zeros(48, K))), dict(member_params=swapped(1, 0, torch.zeros(32, K))),
        dict(member_params=swapped(1, 4, torch.zeros(41, H))), dict(member_params=swapped(2, 2, torch.zeros(H, H, dtype=torch.float16))),
        dict(plans="plan"), dict(plans={"a": a_plan()}), dict(obs=two, plans={"a": a_plan()}), dict(obs=two, plans=a_plan()),
        dict(plans=a_plan(rows=n + 1)), dict(plans=a_plan(count=P + 1)), dict(plans=a_plan(order=torch.zeros(7, dtype=torch.int32))),
        dict(plans=a_plan(first=torch.zeros(P + 1, dtype=torch.int64))),
        dict(num_actions=1), dict(num_actions=33), dict(num_actions=20), dict(seed=-1), dict(seed=1 << 64), dict(first_game=-1),
        dict(first_game=1 << 62), dict(step=-1), dict(step=1 << 62), dict(step=torch.zeros(2, dtype=torch.int64)),
        dict(step=torch.zeros(1, dtype=torch.int32)), dict(action_dtype=torch.int16),
        dict(stats={"a"}), dict(stats="a"), dict(stats=3), dict(head={"a"}), dict(obs=two, plans=both, stats={"c"}), dict(obs=two, plans=both, head=["a", "c"]),
        dict(out=vec(torch.int32)), dict(out={k: v for k, v in vec().items() if k != "values"}), dict(out=vec(), head=True),
        dict(out={**vec(), "head": torch.zeros(n, O)}), dict(out={**vec(), "head": torch.zeros(n, O + 1)}, head=True),
        dict(out={**vec(), "log_probs": torch.zeros(n + 1)}), dict(out={"a": vec()}), dict(out=torch.zeros(n)), dict(out=vec(), stats=False),
        dict(out={**vec(), "actions": {"a": torch.zeros(n, dtype=torch.int64)}}),
        dict(obs=two, plans=both, out=league_out), dict(obs=two, plans=both, stats={"b"}, out=league_out),
        dict(obs=two, plans=both, stats={"a"}, out={**league_out, "actions": torch.zeros(n, dtype=torch.int64)}),
        dict(obs=two, plans=both, stats={"a"}, head={"a"}, out={**league_out, "head": {"b": torch.zeros(n, O)}}),
        dict(out={**vec(), "values": x[:, 0]}),
    ]
    for i, bad in enumerate(bad_calls):
        args = dict(obs=x, member_params=good, plans=a_plan(), num_actions=A, seed=1)
        args.update(bad)
        with pytest.raises(ValueError):
            pool_act.sample(**args)
            pytest.fail(f"bad call {i} was accepted: {sorted(bad)}")
    # without a value column "values" is no key of the result, and an `out` that holds it is refused
    flat = [ps[:4] + [torch.zeros(A, H), torch.zeros(A)] for ps in good]
    with pytest.raises(ValueError, match="keys"):
        pool_act.sample(x, flat, a_plan(), A, seed=1, out=vec())
    with pytest.raises(ValueError, match="GPU"):
        pool_act.sample(x, flat, a_plan(), A, seed=1, out={k: v for k, v in vec().items() if k != "values"})


# ---- the judge ----------------------------------------------------------------------------------------------------------------
CASES = PA.cases()


def test_the_case_table_holds_what_the_kernel_can_get_wrong():
    """the table of the GPU test, held to the list it was made from"""
    default = [c for c in CASES if (c["K"], c["H"], c["O"], c["A"]) == (35, 64, 19, 18)]
    assert {(c["n"], c["P"]) for c in default} >= {(n, P) for n in (1, 31, 32, 33, 127, 128, 129, 257, 4099) for P in (1, 3, 16)}
    sizes = {(c["K"], c["H"], c["O"], c["A"], c["activation"]) for c in CASES}
    assert sizes >= {(*size, act) for size in ((35, 32, 19, 18), (36, 64, 14, 13), (72, 128, 33, 32), (8, 32, 2, 2)) for act in ("tanh", "relu")}
    assert {(c["obs_dtype"], c["action_dtype"]) for c in CASES} == {(o, a) for o in N.OBS_DTYPES for a in J.ACTION_DTYPES}
    seen = set()
    for c in CASES:
        members = PA.case_members(c)
        seen |= {(kind, str(m.dtype)) for kind, m in zip(c["kinds"], members) if kind is not None}
    assert seen >= {(kind, dtype) for kind in ("round_robin", "invalid_entries", "one_member_empty", "every_count_1_mod_g", "reverse_sorted")
                    for dtype in PJ.MEMBER_DTYPES}
    shapes = {tuple(kind is not None for kind in c["kinds"]) for c in CASES}
    assert shapes >= {(False, True), (True, True), (True,)}
    assert any(c["head_extra"] > 0 and c["offset"] > 0 for c in CASES)
    assert {c["draw"] for c in CASES} == set(range(len(PA.DRAWS))) and PA.DRAWS[:3] == AJ.DRAWS and PA.DRAWS[1][1] > 1 << 32
    assert PA.DRAWS[2][3] is not None and PA.DRAWS[3] == (PA.DRAWS[2][0], PA.DRAWS[2][1], PA.DRAWS[2][2] + PA.DRAWS[2][3], None)
    assert {c["stats"] for c in CASES} >= {(True, True), (True, False), (False, True), (False, False), (False,)}
    big = [c for c in CASES if c["n"] >= 20000]
    assert [(c["n"], c["P"]) for c in big] == [(40000, 16), (20000, 3)] and big[1].get("max_cus") == 256
    assert (big[1]["K"], big[1]["H"], big[1]["O"], big[1]["A"]) == (72, 128, 40, 32)
    assert PA.CAP is AJ.CAP and len(PA.MUTANTS) == 7


def played(case, mutant=None):
    obs, params = PA.case_inputs(case)
    members = PA.case_members(case)
    return obs, params, members, PA.restate_float32(case, obs, params, members, mutant=mutant)


@pytest.fixture(scope="module")
def restated():
    """the restatement played once on every case of the GPU test"""
    return [played(case) for case in CASES]


@pytest.fixture(scope="module")
def unmutated(restated):
    """{case index: (ambiguous rows per agent, failures)} of the restatement over every case of the GPU test"""
    return {index: PA.verdict(case, restated[index][3], *restated[index][:3], what=f"case {index}") for index, case in enumerate(CASES)}


def test_the_restatement_passes_and_stays_inside_the_cap(unmutated):
    """the float32 chain of the judges' restatements passes every check on every case of the GPU test; the share of ambiguous
    rows, expected at about 2 tau (A - 1) = 1e-4, stays within max(1, 1 % of n) for the fixed seeds"""
    for index, (amb, fails) in unmutated.items():
        n = CASES[index]["n"]
        print(f"case {index} n = {n}: ambiguous rows per agent {amb}, share {max(amb) / n:.5f}, cap {PA.CAP(n)}")
        assert not fails, fails
        assert max(amb) <= PA.CAP(n)


def test_the_wide_pitch_case_has_no_ambiguous_row():
    """tests/test_gpu_wide_pitch.py runs the pool-act launch on 40 rows; CAP(40) = 1 is a condition on the case, so the case
    is picked to need none of it; each agent has exactly one row of an invalid member, one of them behind the 2^31 limit"""
    case, obs, params, members = PA.wide_case()
    got = PA.restate_float32(case, obs, params, members)
    amb, fails = PA.verdict(case, got, obs, params, members, what="wide case")
    print(f"wide case n = {case['n']}: ambiguous rows per agent {amb}, share {max(amb) / case['n']:.5f}")
    assert PA.CAP(case["n"]) == 1 and not fails and amb == [0, 0], (amb, fails)
    assert [np.flatnonzero(~g["written"]).tolist() for g in got] == [[5], [38]]
    assert all(set(PJ.effective_members(m, case["P"]).tolist()) == {-1, 0, 1, 2} for m in members)
    assert [str(m.dtype) for m in members] == ["int32", "int64"]


@pytest.mark.parametrize("mutant", PA.MUTANTS)
def test_every_mutant_is_caught_by_the_gpu_tests_cases(mutant):
    caught = {}
    for index, case in enumerate(CASES):
        if case["n"] > HOST_ROWS:
            continue
        obs, params, members, got = played(case, mutant)
        fails = PA.verdict(case, got, obs, params, members, what=f"case {index}")[1]
        if fails:
            caught[index] = fails
    print(mutant, "caught by", len(caught), "cases:", sorted(caught)[:12], "--", next(iter(caught.values()))[0] if caught else "")
    assert caught, mutant


def test_the_composition_in_float64_agrees_with_the_restatement(restated):
    """judge() -- pool_judge.judge followed by policy_judge.sample on ITS head -- and the float32 restatement write the same rows
    and return the same action wherever a row is unambiguous for both heads, on every case; the restatement's head lies within
    net_judge's tolerance of the float64 one"""
    agree = total = 0
    for index, case in enumerate(CASES):
        obs, params, members, got = restated[index]
        us = PA.uniforms(case)
        for s, (head, tol, a, amb, written) in enumerate(PA.judge(case, obs, params, members)):
            assert np.array_equal(written, got[s]["written"]), (index, s)
            assert N.worst_share(got[s]["head"][written], head[written], tol[written])[0] <= 1, (index, s)
            _, amb32, _, _ = J.sample(got[s]["head"][:, :case["A"]].astype(np.float64), us[s])
            same = (got[s]["actions"] == a) | amb | amb32
            assert same[written].all(), (index, s, int((~same[written]).sum()))
            agree += int(same[written].sum())
            total += int(written.sum())
    print(f"{agree} of {total} written rows agree")
    assert total > 100000
