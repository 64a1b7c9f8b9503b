"""CPU tests (no GPU needed) of the pool library: the plan judge the GPU tests compare with (tests/pool_judge.py) is the header's
plan -- equal to a scalar formulation, a stable partition of the valid rows with pads of -1, inside the capacity, which one
case meets with equality -- and sharp enough that seven mutants fail on the GPU tests' own cases; libpikazoo_pool.so exports
its header's five symbols and carries the tree's build id, nothing loads it before its first use, its code object holds seven
kernels without scratch or spilled vector registers, the entry points refuse bad arguments before any launch and in the
documented order, and ``pikazoo_amd.pool`` raises ``ValueError`` for malformed arguments before it needs the library.

No call here ever passes every check with rows to run: a call that did would launch a kernel on fake pointers wherever a GPU
is present.  A check is shown to PASS by planting a failure of a later one."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import net_judge as N
import pool_judge as PJ
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_mlp_forward_pool", "pz_pool_abi_version", "pz_pool_build_id", "pz_pool_capacity", "pz_pool_plan"]
KERNELS = sorted([f"pz_pool::mlp_forward_pool_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1)] + ["pz_pool::pool_plan_kernel"])
PLAN_DECL = ("int pz_pool_plan(const void *members, int32_t member_format, int64_t n, int32_t num_members, int32_t *order, int32_t *first, "
             "int32_t *errors, void *stream);")


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.pool, the judge's included: none of them runs without the module"""
    from pikazoo_amd import pool

    return pool


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import pool

    return pool.load()


# ---- the judge ----------------------------------------------------------------------------------------------------------------
def all_plan_cases():
    for n in PJ.PLAN_N:
        for kind, P, dtype, members in PJ.plan_cases(n):
            yield n, kind, P, dtype, members


def test_the_plan_judge_agrees_with_a_scalar_formulation_and_has_the_headers_properties():
    seen = set()
    for n, kind, P, dtype, members in all_plan_cases():
        order, first, errors = PJ.plan(members, P)
        s_order, s_first, s_errors = PJ.plan_scalar(members, P)
        assert order.tolist() == s_order and first.tolist() == s_first and errors == s_errors, (n, kind, P, dtype)
        n_rows = len(members)
        assert order.dtype == np.int32 and first.dtype == np.int32 and len(order) == PJ.capacity(n_rows, P) and len(first) == P + 1
        valid = PJ.valid_rows(members, P)
        assert errors == n_rows - valid.sum()
        assert first[0] == 0 and (np.diff(first) >= 0).all() and (first % PJ.G == 0).all() and first[P] <= PJ.capacity(n_rows, P)
        m = members.astype(np.int64)
        for p in range(P):
            group = order[first[p]:first[p + 1]]
            rows = group[group >= 0]
            assert np.array_equal(rows, np.flatnonzero(valid & (m == p))), (n, kind, P, p)          # the member's rows, ascending: stable
            assert (group[len(rows):] == -1).all() and len(group) - len(rows) < PJ.G                  # pads, less than a group of them
        assert (order[first[P]:] == -1).all()
        live = order[order >= 0]
        assert len(live) == valid.sum() == len(np.unique(live))                                       # a partition of the valid rows
        seen.add((kind, dtype))
        if kind == "every_count_1_mod_g":
            assert errors == 0 and (np.bincount(m, minlength=P) % PJ.G == 1).all()
            assert first[P] == PJ.capacity(n_rows, P), "the capacity bound is met with equality"
        if kind == "invalid_entries":
            assert errors > 0
    assert {k for k, _ in seen} == set(PJ.MEMBER_KINDS) and {d for _, d in seen} == set(PJ.MEMBER_DTYPES)
    assert sorted({n for n, *_ in all_plan_cases()}) == sorted(PJ.PLAN_N) and {P for _, _, P, _, _ in all_plan_cases()} == set(PJ.PLAN_P)


def test_the_capacity_is_a_bound_and_is_tight():
    rng = np.random.default_rng(1)
    for _ in range(300):
        P = int(rng.integers(1, 17))
        n = int(rng.integers(0, 3000))
        members = rng.integers(-1, P + 1, n)
        _, first, _ = PJ.plan(members, P)
        assert first[P] <= PJ.capacity(n, P)
    for P in (1, 5, 16):                                        # every count 1 mod G: equality
        members = np.repeat(np.arange(P), 1 + PJ.G * np.arange(P))
        order, first, errors = PJ.plan(members, P)
        assert first[P] == PJ.capacity(len(members), P) == len(order) and errors == 0
    assert PJ.capacity(0, 1) == PJ.G and PJ.capacity(127, 16) == 16 * PJ.G and PJ.capacity(128, 1) == 2 * PJ.G


def test_every_plan_mutant_is_caught_by_the_gpu_tests_own_member_vectors():
    """the GPU test compares order and first word for word: each mutant's plan differs from the definition's on some of its cases"""
    caught = {m: 0 for m in PJ.PLAN_MUTANTS}
    for n, kind, P, dtype, members in all_plan_cases():
        want = PJ.plan(members, P)
        for mutant in PJ.PLAN_MUTANTS:
            got = PJ.plan(members, P, mutant=mutant)
            caught[mutant] += not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
    print(caught)
    assert len(PJ.PLAN_MUTANTS) == 3 and all(count > 0 for count in caught.values()), caught


def test_every_forward_mutant_is_caught_by_the_gpu_tests_own_cases():
    """what the GPU test checks of a forward -- which rows are written, and every written row against net_judge under its own
    member's parameters -- fails under each mutant on at least one of its cases (the largest case is left to the GPU)"""
    caught = {m: 0 for m in PJ.FORWARD_MUTANTS}
    for case in PJ.forward_cases():
        if case["n"] > 5000:
            continue
        obs, params = PJ.case_inputs(case)
        members = PJ.case_members(case)
        for s in range(len(obs)):
            eff = PJ.effective_members(members[s], case["P"])
            ref, tol = PJ.judge(obs[s], params, eff, case["activation"], case["out_dtype"])
            written = np.ones(len(obs[s]), bool) if eff is None else eff >= 0
            for mutant in PJ.FORWARD_MUTANTS:
                other = members[0] if s == 1 else None
                bad = PJ.effective_members(members[s], case["P"], mutant=mutant, other=other)
                have, _ = PJ.judge(obs[s], params, bad, case["activation"], case["out_dtype"])
                bad_written = np.ones(len(obs[s]), bool) if bad is None else bad >= 0
                if not np.array_equal(bad_written, written):
                    caught[mutant] += 1                     # a row that must keep the sentinel was written, or the reverse
                elif N.worst_share(have[written], ref[written], tol[written])[0] > 1:
                    caught[mutant] += 1
    print(caught)
    assert len(PJ.FORWARD_MUTANTS) == 4 and all(count > 0 for count in caught.values()), caught


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_pool_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, batch, net, pool

    assert header_functions("pikazoo_pool.h") == NAMES == sorted(pool.SIGNATURES) == dynamic_pz_symbols(pz_build.POOL_LIB)
    assert pz_build.library_id(pz_build.POOL_LIB) == pz_build.source_id() == lib.pz_pool_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.POOL_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_pool.h") in pz_build.DEPS
    assert (pz_build.CSRC / "pz_mlp_tile.hpp") in pz_build.DEPS
    assert lib.pz_pool_abi_version() == pool.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_pool.h").read_text()
    assert "#define PZ_POOL_ABI_VERSION 1" in header
    assert f"#define PZ_POOL_MAX_MEMBERS {pool.MAX_MEMBERS}\n" in header and pool.MAX_MEMBERS == PJ.MAX_MEMBERS == 16
    assert f"#define PZ_POOL_GROUP_ROWS {pool.GROUP_ROWS}\n" in header and pool.GROUP_ROWS == PJ.G == 128
    for key, value in pool.MEMBER_FORMATS.items():
        assert re.search(r"PZ_POOL_MEMBER_%s = %d\b" % (str(key).split(".")[-1].upper(), value), header), key
    assert [str(d).split(".")[-1] for d in pool.MEMBER_FORMATS] == list(PJ.MEMBER_DTYPES)
    # the struct of the binding is the header's: six pointers
    assert C.sizeof(pool.Member) == 48
    body = re.search(r"typedef struct pz_pool_member \{(.*?)\} pz_pool_member;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in pool.Member._fields_]
    # the capacity is the header's function, the judge's and the binding's
    for n, P in ((0, 1), (1, 1), (127, 16), (128, 1), (4099, 3), (1 << 30, 16)):
        assert lib.pz_pool_capacity(n, P) == pool.capacity(n, P) == PJ.capacity(n, P) == (n // 128 + P) * 128
    for n, P in ((-1, 1), ((1 << 30) + 1, 1), (5, 0), (5, 17)):
        assert lib.pz_pool_capacity(n, P) == -1
    # no other library holds any of the names, and the older libraries' ABI versions did not move
    others = (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB, pz_build.PPO_LIB, pz_build.NET_LIB, pz_build.NETGRAD_LIB,
              pz_build.OPTIM_LIB, pz_build.BATCH_LIB)
    for other in others:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
        assert pz_build.library_id(other) == pz_build.source_id(), other
    assert not set(NAMES) & set(_native.exported_names())
    assert _native.load().pz_abi_version() == 10
    assert net.load().pz_net_abi_version() == net.ABI_VERSION == 1 and batch.load().pz_batch_abi_version() == batch.ABI_VERSION == 1
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_pool.h" in doc and "libpikazoo_pool.so" in doc
    assert PLAN_DECL in doc and PLAN_DECL in header
    from test_net_host import declared_arguments

    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_mlp_forward_pool")
    assert len(args) == 20 == len(pool.SIGNATURES["pz_mlp_forward_pool"][1]) and declared_arguments(doc, "pz_mlp_forward_pool") == args


def test_importing_the_other_modules_does_not_load_the_pool_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim, batch; "
            "assert 'pikazoo_amd.pool' not in sys.modules; import pikazoo_amd as p; assert 'pool' in p.__all__; "
            "p.pool.plan; p.pool.forward; p.pool.Snapshots; p.pool.Plan; "
            "assert 'pikazoo_amd.pool' in sys.modules and p.pool._lib is None; "
            "assert not any('libpikazoo_pool' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_pool_library(pz_build):
    """SEVEN kernels: the plan, and the forward per hidden width and activation (the compile-time choices of the net library).
    None uses scratch or spills a vector register -- the 16 members' pointers are indexed in the kernel arguments, not copied
    to private memory.  The forward's LDS is dynamic (one staged parameter set and the plan's `first`); the plan's is its
    (member, wave) counts.  Read from the code object's notes alone: nothing is disassembled."""
    import kernel_notes

    notes = kernel_notes.notes(pz_build.POOL_LIB)
    short = lambda name: name.replace("void ", "").split("(")[0]  # noqa: E731
    assert sorted(short(name) for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        total = row[".vgpr_count"] + row.get(".agpr_count", 0)
        if "plan" in name:
            assert 4 * (16 * 16 + 16 + 17 + 16) <= row[".group_segment_fixed_size"] <= 2048 and row[".sgpr_spill_count"] == 0 and total <= 64, (name, row)
        else:
            assert row[".group_segment_fixed_size"] == 0, (name, row)
            assert total <= (512 if "<128" in name else 256), (name, row)     # two waves per SIMD at the narrower widths
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row})


# ---- argument checking --------------------------------------------------------------------------------------------------------
FAKE = 4096


def member_array(P=3, **by_index):
    """good fake members; `m<index>={field: value}` overwrites fields of one"""
    from pikazoo_amd import pool

    array = (pool.Member * 16)()
    for i in range(P):
        array[i] = pool.Member(*[FAKE + 256 * i + 16 * j for j in range(6)])
    for i, fields in ((int(key[1:]), fields) for key, fields in by_index.items()):
        for field, value in fields.items():
            setattr(array[i], field, value)
    return array


# by default the LAST check fails: first_p2 is not 4-byte aligned
FORWARD = dict(obs_p1=FAKE, obs_p2=FAKE, obs_format=2, n=8, in_features=35, obs_pitch=35, hidden=64, out_features=19, activation=0, members=None,
               num_members=3, order_p1=FAKE, first_p1=FAKE, order_p2=FAKE, first_p2=FAKE + 2, out_p1=FAKE, out_p2=FAKE, out_format=0, out_pitch=19,
               stream=None)


def test_argument_validation_of_the_forward(lib):
    """Every return code in the documented order.  The LAST check (the alignment of agent 2's `first`) is planted in every
    call that is meant to pass the earlier ones: -4 then says that they all passed."""
    def fwd(members="good", **over):
        a = dict(FORWARD)
        assert not set(over) - set(a)
        a.update(over)
        a["members"] = member_array(max(1, min(a["num_members"], 16))) if isinstance(members, str) else members
        return lib.pz_mlp_forward_pool(*a.values())

    passes = lambda **kw: fwd(**kw) == -4  # noqa: E731
    assert passes() and passes(num_members=1) and passes(num_members=16) and passes(n=1 << 30) and passes(n=0)
    assert passes(order_p1=None, first_p1=None) and passes(order_p1=None) and passes(in_features=72, obs_pitch=72, hidden=128, out_features=40, out_pitch=40)
    assert passes(in_features=1, hidden=32, out_features=1) and passes(obs_pitch=36, out_pitch=20)
    ok = dict(first_p2=FAKE)
    assert fwd(n=0, **ok) == 0 and fwd(n=0, obs_p2=None, out_p2=None, order_p2=None, first_p2=None) == 0
    assert fwd(n=0, order_p1=None, first_p1=None, order_p2=None, first_p2=None) == 0
    # NULL: agent 1, the member array, agent 2 all or none
    for name in ("obs_p1", "out_p1"):
        assert fwd(**{name: None}) == -1, name
    assert fwd(members=None) == -1
    assert fwd(obs_p2=None) == -1 and fwd(out_p2=None) == -1
    assert fwd(obs_p2=None, out_p2=None) == -1 and fwd(obs_p2=None, out_p2=None, order_p2=None) == -1      # a plan of an absent agent
    assert fwd(obs_p2=None, out_p2=None, first_p2=None) == -1
    # P out of range, before a member is looked at
    for P in (0, -1, 17, 1 << 20):
        assert fwd(num_members=P) == -2, P
        assert fwd(num_members=P, members=member_array(3, m0=dict(w1=None))) == -2, P
    # a NULL member pointer; first NULL while order is not
    for i in (0, 2):
        for field in ("w1", "b1", "w2", "b2", "w3", "b3"):
            assert fwd(members=member_array(3, **{f"m{i}": {field: None}})) == -1, (i, field)
    assert passes(members=member_array(3, m3=dict(w1=None)))                                            # behind P: not looked at
    assert fwd(first_p1=None) == -1 and fwd(first_p2=None) == -1
    # ... and both stand in front of the sizes
    assert fwd(members=member_array(3, m1=dict(b2=None)), n=-1) == -1 and fwd(first_p1=None, hidden=48) == -1
    # sizes: the box of pikazoo_net.h
    for bad in (dict(n=-1), dict(n=(1 << 30) + 1), dict(in_features=0), dict(in_features=73, obs_pitch=80), dict(hidden=0), dict(hidden=48), dict(hidden=256),
                dict(out_features=0), dict(out_features=41, out_pitch=41), dict(obs_pitch=34), dict(out_pitch=18), dict(obs_pitch=1 << 61), dict(out_pitch=1 << 61)):
        assert fwd(**bad) == -2, bad
    # formats and the activation
    for name, count in (("obs_format", 5), ("out_format", 3), ("activation", 2)):
        assert fwd(**{name: count}) == -3 and fwd(**{name: -1}) == -3, name
        for value in range(count):
            assert fwd(n=0, **{name: value}, **ok) == 0, (name, value)
    # alignment to the element
    for name in ("obs_p1", "obs_p2", "out_p1", "out_p2", "order_p1", "first_p1", "order_p2", "first_p2"):
        assert fwd(**{**ok, name: FAKE + 1}) == -4, name
        assert fwd(**{**ok, name: FAKE + 2}) == -4, name
        assert fwd(n=0, **{**ok, name: FAKE + 4}) == 0, name
    assert fwd(n=0, obs_format=1, obs_p1=FAKE + 2, **ok) == 0 and fwd(n=0, out_format=2, out_p2=FAKE + 2, **ok) == 0
    for field in ("w1", "b3"):
        assert fwd(members=member_array(3, m2={field: FAKE + 2}), **ok) == -4, field
    assert fwd(n=0, members=member_array(3, m2=dict(w1=FAKE + 8)), **ok) == 0
    # the order of the checks: NULL, P, NULL of a member, size, config, alignment
    broken = member_array(3, m1=dict(w3=None))
    assert fwd(members=broken, out_p1=None, num_members=0, n=-1, activation=9) == -1
    assert fwd(members=broken, num_members=17, n=-1, activation=9) == -2
    assert fwd(members=broken, n=-1, activation=9) == -1
    assert fwd(n=-1, activation=9) == -2 and fwd(activation=9) == -3 and fwd() == -4


def test_argument_validation_of_the_plan(lib):
    """pz_pool_plan(members, member_format, n, num_members, order, first, errors, stream): its planted last failure is a
    misaligned `errors`"""
    def call(members=FAKE, member_format=1, n=64, num_members=3, order=FAKE, first=FAKE, errors=FAKE + 2):
        return lib.pz_pool_plan(members, member_format, n, num_members, order, first, errors, None)

    assert call() == -4 and call(n=1 << 30) == -4 and call(num_members=1) == -4 and call(num_members=16) == -4 and call(n=0, members=None) == -4
    for fmt in (0, 1, 2):
        assert call(member_format=fmt) == -4
    for name in ("order", "first", "errors"):
        assert call(**{name: None}) == -1, name
    assert call(members=None) == -1
    for bad in (dict(n=-1), dict(n=(1 << 30) + 1), dict(num_members=0), dict(num_members=17), dict(num_members=-3)):
        assert call(**bad) == -2, bad
    assert call(member_format=3) == -3 and call(member_format=-1) == -3
    good = dict(errors=FAKE)
    assert call(members=FAKE + 2, **good) == -4 and call(members=FAKE + 4, member_format=2, **good) == -4
    for name in ("order", "first", "errors"):
        for off in (1, 2, 3):
            assert call(**{**good, name: FAKE + off}) == -4, (name, off)
    assert call(order=None, n=-1, member_format=7) == -1 and call(n=-1, member_format=7) == -2 and call(member_format=7) == -3


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device and range errors raise ValueError -- on CPU tensors the device check stands behind the others, so
    every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import net, pool

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(pool, "load", refuse)
    n, K, H, O, P = 8, 35, 64, 19, 3
    one = lambda: [torch.zeros(H, K), torch.zeros(H), torch.zeros(H, H), torch.zeros(H), torch.zeros(O, H), torch.zeros(O)]  # noqa: E731
    good = [one() for _ in range(P)]
    x = torch.zeros(n, K)
    members = torch.zeros(n, dtype=torch.int64)

    def a_plan(rows=n, count=P, **over):
        fields = dict(order=torch.zeros(pool.capacity(rows, count), dtype=torch.int32), first=torch.zeros(count + 1, dtype=torch.int32),
                      errors=torch.zeros(1, dtype=torch.int32), n=rows, num_members=count)
        fields.update(over)
        return pool.Plan(**fields)

    # the plan
    with pytest.raises(ValueError, match="GPU"):
        pool.plan(members, P)
    with pytest.raises(ValueError, match="GPU"):
        pool.plan(members.to(torch.uint8), 16, out=a_plan(count=16))
    for bad in (dict(members=[0, 1]), dict(members=torch.zeros(n, 2, dtype=torch.int64)), dict(members=torch.zeros(2 * n, dtype=torch.int64)[::2]),
                dict(members=torch.zeros(n, dtype=torch.int16)), dict(members=torch.zeros(n)), dict(num_members=0), dict(num_members=17),
                dict(num_members=3.0), dict(num_members=True), dict(out="plan"), dict(out=a_plan(rows=n + 1)), dict(out=a_plan(count=P + 1)),
                dict(out=a_plan(order=torch.zeros(5, dtype=torch.int32))), dict(out=a_plan(first=torch.zeros(P + 1, dtype=torch.int64))),
                dict(out=a_plan(errors=torch.zeros(2, dtype=torch.int32))), dict(out=a_plan(errors=torch.zeros(1, dtype=torch.int32, device="meta")))):
        with pytest.raises(ValueError):
            pool.plan(**{**dict(members=members, num_members=P), **bad})
            pytest.fail(f"bad plan {sorted(bad)} was accepted")
    assert pool.capacity(4099, 3) == PJ.capacity(4099, 3)
    # the forward
    with pytest.raises(ValueError, match="GPU"):
        pool.forward(x, good, a_plan())
    with pytest.raises(ValueError, match="GPU"):
        pool.forward({"a": x, "b": x}, good, {"a": None, "b": a_plan()}, "relu", out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        pool.forward(x, good[:1], None)

    def swapped(m, i, t):
        return [[t if (mm, j) == (m, i) else p for j, p in enumerate(ps)] for mm, ps in enumerate(good)]

    bad_calls = [
        dict(obs=torch.zeros(n)), dict(obs=torch.zeros(n, 73)), dict(obs=torch.zeros(n, K, dtype=torch.float64)), dict(obs=torch.zeros(K, n).t()),
        dict(obs={}), dict(obs=None), dict(obs={"a": x, "b": torch.zeros(n + 1, K)}, plans={"a": None, "b": None}),
        dict(obs={"a": x, "b": x, "c": x}, plans={"a": None, "b": None, "c": None}), dict(activation="gelu"), dict(out_dtype=torch.float64),
        dict(member_params=[]), dict(member_params=[one() for _ in range(17)], plans=None), dict(member_params=one()[0]), dict(member_params={"a": good}),
        dict(member_params=[one()[:5]] * 3), dict(member_params=[one(), one(), None]), dict(member_params=swapped(2, 3, None)),
        dict(member_params=swapped(0, 0, torch.zeros(H, K + 1))), dict(member_params=swapped(0, 0, torch.zeros(48, K))),
        dict(member_params=swapped(1, 0, torch.zeros(32, K))),                                                     # members of different widths
        dict(member_params=swapped(2, 2, torch.zeros(H, H, dtype=torch.float16))), dict(member_params=swapped(1, 2, torch.zeros(H, H + 1)[:, :H])),
        dict(member_params=swapped(1, 4, torch.zeros(41, H))), dict(member_params=swapped(2, 5, torch.zeros(O + 1))),
        dict(member_params=swapped(1, 1, torch.zeros(H, device="meta"))),
        dict(plans="plan"), dict(plans={"a": a_plan()}), dict(obs={"a": x}, plans=a_plan()), dict(obs={"a": x}, plans={"b": a_plan()}),
        dict(obs={"a": x, "b": x}, plans={"a": a_plan()}), dict(plans=a_plan(rows=n + 1)), dict(plans=a_plan(count=P + 1)),
        dict(plans=a_plan(order=torch.zeros(7, dtype=torch.int32))), dict(plans=a_plan(first=torch.zeros(P + 1, dtype=torch.int64))),
        dict(plans=a_plan(order=torch.zeros(2 * pool.capacity(n, P), dtype=torch.int32)[::2])),
        dict(out=torch.zeros(n, O + 1)), dict(out=torch.zeros(n, O, dtype=torch.float64)), dict(out={"a": torch.zeros(n, O)}),
    ]
    for i, bad in enumerate(bad_calls):
        args = dict(obs=x, member_params=good, plans=a_plan(), activation="tanh")
        args.update(bad)
        with pytest.raises(ValueError):
            pool.forward(**args)
            pytest.fail(f"bad forward {i} was accepted: {sorted(bad)}")
    # the snapshots
    model = net.ActorCritic()
    league = pool.Snapshots(model, 3)
    assert len(league) == 1 and len(league.member_params()) == 1 and league.member_params()[0][0] is model.fc1.weight
    assert league.push() == 1 and league.push() == 2 and len(league) == 3 and league.push() == 1 and len(league) == 3 and league.pushes == 3
    with torch.no_grad():
        model.fc1.weight.add_(1.0)
    assert not torch.equal(league.member_params()[1][0], model.fc1.weight) and league.member_params()[1][0].requires_grad is False
    league.push()
    assert torch.equal(league.member_params()[2][0], model.fc1.weight) and league.member_params()[2][0] is not model.fc1.weight
    with pytest.raises(ValueError, match="GPU"):
        league.act(x, a_plan())
    for bad in (dict(model=torch.nn.Linear(3, 3)), dict(capacity=0), dict(capacity=17), dict(capacity=2.0)):
        with pytest.raises(ValueError):
            pool.Snapshots(**{**dict(model=model, capacity=4), **bad})
    with pytest.raises(ValueError, match="capacity 1"):
        pool.Snapshots(model, 1).push()
    errs = pool.Plan(None, None, torch.tensor([3], dtype=torch.int32), 10, 2)
    with pytest.raises(ValueError, match="3 of 10"):
        errs.check()
    assert pool.Plan(None, None, torch.zeros(1, dtype=torch.int32), 10, 2).check() is not None
