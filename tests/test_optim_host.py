"""CPU tests (no GPU needed) of the optimizer library: libpikazoo_optim.so exports its header's three symbols and carries the
tree's build id, nothing loads it before its first use, its code object holds exactly one kernel without scratch or spilled
registers, the entry point refuses bad arguments before any launch and in the documented order, ``pikazoo_amd.optim`` raises
``ValueError`` for malformed arguments before it needs the library, and the judge the GPU tests compare with
(tests/optim_judge.py) is the definition: equal to torch.optim.Adam / AdamW in float64 behind clip_grad_norm_, wide enough for
a float32 restatement of the header's operation order, and sharp enough that seven mutants fail on the GPU tests' own cases.

No call here ever passes every check: a call that did would launch a kernel on fake pointers wherever a GPU is present.  A
check is shown to PASS by planting a failure of a later one."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import optim_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_adam_step", "pz_optim_abi_version", "pz_optim_build_id"]
KERNELS = ["pz_optim::adam_step_kernel"]
LDS_BYTES = 928  # four pointer tables of 16, two prefix tables of 17, two flag tables of 16, 16 float64 wave sums, 2 floats


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.optim, the judge's included: none of them runs without the module"""
    from pikazoo_amd import optim

    return optim


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import optim

    return optim.load()


def test_optim_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, learn, net, netgrad, optim, policy, ppo

    assert header_functions("pikazoo_optim.h") == NAMES == sorted(optim.SIGNATURES) == dynamic_pz_symbols(pz_build.OPTIM_LIB)
    assert pz_build.library_id(pz_build.OPTIM_LIB) == pz_build.source_id() == lib.pz_optim_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.OPTIM_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_optim.h") in pz_build.DEPS
    assert lib.pz_optim_abi_version() == optim.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_optim.h").read_text()
    assert "#define PZ_OPTIM_ABI_VERSION 1" in header
    for name, value in (("PZ_OPTIM_MAX_TENSORS", optim.MAX_TENSORS), ("PZ_OPTIM_MAX_GROUPS", optim.MAX_GROUPS)):
        assert f"#define {name} {value}\n" in header
    assert "#define PZ_OPTIM_MAX_ELEMENTS (1 << 20)" in header and optim.MAX_ELEMENTS == 1 << 20
    # the structs of the binding are the header's: 8-byte pointers and int64 behind an int32 count
    assert C.sizeof(optim.Tensor) == 40 and C.sizeof(optim.Group) == 8 + 16 * 40 + 24 and C.sizeof(optim.Config) == 56
    for struct, name in ((optim.Tensor, "pz_optim_tensor"), (optim.Group, "pz_optim_group"), (optim.Config, "pz_adam_config")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
        fields = re.findall(r"(\w+)\s*(?:\[\w+\])?\s*[;,]", body)
        assert sorted(fields) == sorted(n for n, _ in struct._fields_), name
    # no other library holds any of the names, and the older libraries' ABI versions did not move
    others = (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB, pz_build.PPO_LIB, pz_build.NET_LIB, pz_build.NETGRAD_LIB)
    for other in others:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
        assert pz_build.library_id(other) == pz_build.source_id(), other
    assert not set(NAMES) & set(_native.exported_names())
    assert _native.load().pz_abi_version() == 10
    assert learn.load().pz_learn_abi_version() == learn.ABI_VERSION == 1
    assert policy.load().pz_policy_abi_version() == policy.ABI_VERSION == 1
    assert ppo.load().pz_ppo_abi_version() == ppo.ABI_VERSION == 1
    assert net.load().pz_net_abi_version() == net.ABI_VERSION == 1
    assert netgrad.load().pz_netgrad_abi_version() == netgrad.ABI_VERSION == 1
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_optim.h" in doc and "libpikazoo_optim.so" in doc
    assert "int pz_adam_step(const pz_optim_group *groups, int32_t n_groups, const pz_adam_config *cfg, void *stream);" in doc
    assert "int pz_adam_step(const pz_optim_group *groups, int32_t n_groups, const pz_adam_config *cfg, void *stream);" in header


def test_importing_the_other_modules_does_not_load_the_optim_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad; "
            "assert 'pikazoo_amd.optim' not in sys.modules; m = net.ActorCritic(); "
            "\ntry:\n    m.act(__import__('torch').zeros(4, 35))\nexcept ValueError:\n    pass\n"
            "assert 'pikazoo_amd.optim' not in sys.modules; import pikazoo_amd as p; assert 'optim' in p.__all__; p.optim.adam_step; p.optim.Adam; "
            "assert 'pikazoo_amd.optim' in sys.modules and p.optim._lib is None; "
            "assert not any('libpikazoo_optim' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_optim_library(pz_build):
    """ONE kernel: groups, tensor counts, both decays, the clip and the skip are run-time.  It uses no scratch and spills
    nothing; a workgroup of 1024 threads is 4 waves on each SIMD, which leaves a wave 512 / 4 = 128 vector registers; the LDS
    is the static table of the source, to the byte."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.OPTIM_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.OPTIM_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == LDS_BYTES, (name, row)
        assert row[".vgpr_count"] + row.get(".agpr_count", 0) <= 128 and row.get(".agpr_count", 0) == 0, (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


# ---- argument checking ------------------------------------------------------------------------------------------------------
FAKE = 4096


def fake_call(lib, n_groups=2, counts=(6, 2), groups_null=False, cfg_null=False, tensor=None, group=None, numel=None, **cfg):
    """pz_adam_step on fake pointers.  `tensor` = (group, index, field, value), `group` = (group, field, value) and `numel` =
    (group, index, value) overwrite one entry; `cfg` overwrites fields of a good configuration."""
    from pikazoo_amd import optim

    array = (optim.Group * 2)()
    for a in range(2):
        array[a].count = counts[a]
        for i in range(16):
            array[a].tensors[i] = optim.Tensor(100 + i, FAKE, FAKE + 16, FAKE + 32, FAKE + 48)
        array[a].step, array[a].stats, array[a].lr_device = FAKE + 8, FAKE + 4, None
    if tensor:
        a, i, field, value = tensor
        setattr(array[a].tensors[i], field, value)
    if numel:
        a, i, value = numel
        array[a].tensors[i].numel = value
    if group:
        a, field, value = group
        setattr(array[a], field, value)
    c = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.5, decoupled=0, skip_nonfinite=0)
    assert not set(cfg) - set(c)
    c.update(cfg)
    config = optim.Config(**c)
    return lib.pz_adam_step(None if groups_null else array, n_groups, None if cfg_null else C.byref(config), None)


def test_argument_validation(lib):
    """Every return code in the documented order.  The LAST check (alignment) is planted in every call that is meant to pass the
    earlier ones: -4 then says that NULL, size and configuration checks all passed."""
    bad_step = dict(group=(0, "step", FAKE + 4))  # 4-byte but not 8-byte aligned

    def passes(**kw):
        """the call fails only the planted alignment check"""
        planted = dict(bad_step)
        if "group" in kw:  # the group override is taken: plant a tensor pointer instead
            planted = dict(tensor=(0, 0, "param", FAKE + 2))
        return fake_call(lib, **planted, **kw) == -4

    assert passes() and passes(n_groups=1) and passes(counts=(1, 16)) and passes(counts=(16, 1))
    # NULL
    assert fake_call(lib, groups_null=True) == -1 and fake_call(lib, cfg_null=True) == -1
    for a in (0, 1):
        assert fake_call(lib, group=(a, "step", None)) == -1
        for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
            for i in (0, 5 if a == 0 else 1):
                assert fake_call(lib, tensor=(a, i, field, None)) == -1, (a, i, field)
    assert passes(tensor=(0, 6, "grad", None)) and passes(tensor=(1, 2, "param", None))          # behind count: not looked at
    assert fake_call(lib, n_groups=1, group=(1, "step", None), tensor=(0, 0, "param", FAKE + 2)) == -4   # behind n_groups: not looked at
    assert passes(group=(0, "stats", None)) and passes(group=(1, "lr_device", FAKE + 64))         # both optional
    # sizes
    for n in (0, 3, -1):
        assert fake_call(lib, n_groups=n) == -2, n
    for counts in ((0, 2), (17, 2), (6, 0), (6, 17), (-1, 2)):
        assert fake_call(lib, counts=counts) == -2, counts
    assert fake_call(lib, numel=(0, 3, 0)) == -2 and fake_call(lib, numel=(1, 1, -5)) == -2 and fake_call(lib, numel=(0, 0, (1 << 20) + 1)) == -2
    assert fake_call(lib, numel=(0, 0, (1 << 20) - 514)) == -2                 # the total: 2^20 - 514 + 101 + ... + 105 = 2^20 + 1
    assert passes(numel=(0, 0, (1 << 20) - 515)) and passes(numel=(1, 0, (1 << 20) - 101))         # exactly 2^20 in either group
    assert fake_call(lib, numel=(1, 0, (1 << 20) - 100)) == -2
    # configuration
    nan, inf = float("nan"), float("inf")
    for bad in (dict(lr=-1e-9), dict(lr=nan), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=nan),
                dict(eps=-1e-12), dict(eps=nan), dict(weight_decay=-1e-3), dict(weight_decay=nan), dict(decoupled=2), dict(decoupled=-1),
                dict(skip_nonfinite=2), dict(skip_nonfinite=-1)):
        assert fake_call(lib, **bad) == -3, bad
    for good in (dict(lr=0.0), dict(beta1=0.0, beta2=0.0), dict(eps=0.0), dict(weight_decay=0.5, decoupled=1), dict(skip_nonfinite=1),
                 dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=inf), dict(max_grad_norm=nan)):
        assert passes(**good), good
    # alignment
    for a in (0, 1):
        for off in (1, 2, 4, 12):
            assert fake_call(lib, group=(a, "step", FAKE + off)) == -4
        for field in ("stats", "lr_device"):
            for off in (1, 2, 3):
                assert fake_call(lib, group=(a, field, FAKE + off)) == -4
        for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
            for off in (1, 2, 3):
                assert fake_call(lib, tensor=(a, 1, field, FAKE + off)) == -4
    assert fake_call(lib, n_groups=1, group=(1, "step", FAKE + 4), tensor=(0, 0, "grad", FAKE + 6)) == -4
    # the order of the checks: NULL, size, config, alignment
    assert fake_call(lib, tensor=(0, 0, "grad", None), n_groups=3, lr=-1.0, **bad_step) == -1
    assert fake_call(lib, tensor=(1, 0, "grad", None), counts=(0, 2), lr=-1.0, **bad_step) == -1
    assert fake_call(lib, n_groups=3, lr=-1.0, **bad_step) == -2
    assert fake_call(lib, numel=(1, 1, 0), lr=-1.0, **bad_step) == -2
    assert fake_call(lib, lr=-1.0, **bad_step) == -3
    assert fake_call(lib, **bad_step) == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """dtype, contiguity, device, aliasing, counts, lengths and host ranges raise ValueError -- on CPU tensors the device check
    stands behind the others, so every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import optim

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(optim, "load", refuse)
    shapes = [(4, 3), (4,), (2, 4)]

    def fresh():
        return dict(params=[torch.zeros(s) for s in shapes], grads=[torch.zeros(s) for s in shapes], exp_avg=[torch.zeros(s) for s in shapes],
                    exp_avg_sq=[torch.zeros(s) for s in shapes], step=torch.zeros(2, dtype=torch.int64), lr=1e-3)

    with pytest.raises(ValueError, match="GPU"):
        optim.adam_step(**fresh())
    two = {k: ({"a": v, "b": fresh()[k]} if k != "lr" else v) for k, v in fresh().items()}
    with pytest.raises(ValueError, match="GPU"):
        optim.adam_step(**two, stats={"a": torch.zeros(2), "b": torch.zeros(2)}, max_grad_norm=0.5, weight_decay=0.1, decoupled=True,
                        skip_nonfinite=True, betas=(0.5, 0.75), eps=0.0)
    with pytest.raises(ValueError, match="GPU"):
        optim.adam_step(**{**fresh(), "lr": torch.tensor(1e-3)})

    def swapped(what, i, t):
        a = fresh()
        a[what][i] = t
        return a

    big = torch.zeros(64)
    shared = fresh()
    shared["exp_avg"][1] = shared["params"][1]
    overlap = fresh()
    overlap["params"][1], overlap["exp_avg_sq"][1] = big[0:4], big[3:7]
    grad_alias = fresh()
    grad_alias["grads"][0] = grad_alias["exp_avg"][0]
    bad_calls = [
        swapped("params", 0, torch.zeros(4, 3, dtype=torch.float64)), swapped("grads", 1, torch.zeros(4, dtype=torch.float16)),
        swapped("exp_avg", 2, torch.zeros(2, 4, dtype=torch.bfloat16)), swapped("exp_avg_sq", 0, torch.zeros(4, 3, dtype=torch.int32)),
        swapped("params", 0, torch.zeros(3, 4).t()), swapped("grads", 0, torch.zeros(4, 6)[:, ::2]), swapped("exp_avg", 2, torch.zeros(4, 2).t()),
        swapped("params", 1, torch.zeros(4, device="meta")), swapped("grads", 1, torch.zeros(4, device="meta")),
        swapped("grads", 1, torch.zeros(5)), swapped("exp_avg", 0, torch.zeros(3, 4)), swapped("exp_avg_sq", 2, torch.zeros(8)),
        swapped("params", 1, torch.zeros(0)), swapped("params", 1, None), swapped("grads", 2, 1.0),
        shared, overlap, grad_alias,
        {**fresh(), "params": [torch.zeros(1) for _ in range(17)], "grads": [torch.zeros(1) for _ in range(17)],
         "exp_avg": [torch.zeros(1) for _ in range(17)], "exp_avg_sq": [torch.zeros(1) for _ in range(17)]},
        {**fresh(), "params": [], "grads": [], "exp_avg": [], "exp_avg_sq": []},
        {**fresh(), "grads": fresh()["grads"][:2]}, {**fresh(), "exp_avg": fresh()["exp_avg"] + [torch.zeros(1)]},
        {**fresh(), "exp_avg_sq": fresh()["exp_avg_sq"][0]}, {**fresh(), "params": torch.zeros(4)},
        {**fresh(), "params": [torch.zeros((1 << 20) + 1)], "grads": [torch.zeros((1 << 20) + 1)], "exp_avg": [torch.zeros((1 << 20) + 1)],
         "exp_avg_sq": [torch.zeros((1 << 20) + 1)]},
        # step and stats
        {**fresh(), "step": torch.zeros(2, dtype=torch.int32)}, {**fresh(), "step": torch.zeros(3, dtype=torch.int64)},
        {**fresh(), "step": torch.zeros(4, dtype=torch.int64)[::2]}, {**fresh(), "step": None}, {**fresh(), "step": {"a": torch.zeros(2, dtype=torch.int64)}},
        {**fresh(), "stats": torch.zeros(2, dtype=torch.float64)}, {**fresh(), "stats": torch.zeros(1)},
        # groups: a dict of three, keys that differ, a dict beside a sequence
        {**two, "grads": {"a": two["grads"]["a"], "c": two["grads"]["b"]}}, {**two, "step": two["step"]["a"]}, {**two, "exp_avg": two["exp_avg"]["a"]},
        {**two, "params": {**two["params"], "c": fresh()["params"]}}, {**two, "params": {}},
        {**two, "params": {"a": two["params"]["a"], "b": two["params"]["a"]}},   # (the two groups' parameters overlap)
        # host hyperparameters
        {**fresh(), "lr": -1e-3}, {**fresh(), "lr": float("nan")}, {**fresh(), "lr": torch.tensor(1e-3, dtype=torch.float64)},
        {**fresh(), "lr": torch.zeros(2)}, {**fresh(), "betas": (1.0, 0.999)}, {**fresh(), "betas": (0.9, -0.1)}, {**fresh(), "betas": 0.9},
        {**fresh(), "eps": -1e-8}, {**fresh(), "weight_decay": -0.1}, {**fresh(), "max_grad_norm": float("nan")},
    ]
    lr_alias = fresh()
    lr_alias["lr"] = lr_alias["exp_avg"][1][0]
    bad_calls.append(lr_alias)
    for i, bad in enumerate(bad_calls):
        with pytest.raises(ValueError):
            optim.adam_step(**bad)
            pytest.fail(f"bad call {i} was accepted")
    # the class: the same host ranges at construction, at most two param groups, and the same tensor checks at step()
    w = torch.nn.Parameter(torch.zeros(4, 3))
    for bad in (dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            optim.Adam([w], **bad)
    with pytest.raises(ValueError):
        optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(1))]} for _ in range(3)])
    o = optim.Adam([w], lr=1e-3)
    assert o.step() is None and not o.state                     # no gradient anywhere: nothing to launch
    w.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="GPU"):
        o.step()
    assert int(o.steps) == 0 and int(o.skipped) == 0 and set(o.stats) == {"grad_norm", "clip_coef"} and o.stats["grad_norm"].dim() == 0
    w.grad = torch.zeros(3, 4).t()
    with pytest.raises(ValueError):
        o.step()


# ---- the judge --------------------------------------------------------------------------------------------------------------
TORCH_CASES = [
    ("adam_clip_engaged", dict(lr=1e-2, eps=1e-5, max_grad_norm=0.5), 1.0),
    ("adam_clip_idle", dict(lr=1e-2, eps=1e-5, max_grad_norm=1e3), 1.0),
    ("adam_no_clip", dict(lr=1e-2, eps=1e-8), 1.0),
    ("adam_l2", dict(lr=1e-2, eps=1e-8, weight_decay=0.1, max_grad_norm=0.5), 1.0),
    ("adamw", dict(lr=1e-2, eps=1e-8, weight_decay=0.1, decoupled=True, max_grad_norm=0.5), 1.0),
    ("zero_gradient", dict(lr=1e-2, eps=1e-8, max_grad_norm=0.5), 0.0),
]


@pytest.mark.parametrize("name,kw,scale", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_judge_equals_torch_float64_adam_behind_clip_grad_norm(name, kw, scale):
    """5 steps of step64 on its own float64 state against torch.optim.Adam / AdamW in float64 on the CPU behind
    clip_grad_norm_, two groups (two optimizers: a group has a norm and a step count of its own): float64 roundoff"""
    import torch

    o = J.options(**kw)
    engaged = []
    for a, shapes in enumerate((J.DEFAULT_NET, ((5, 3), (7,)))):
        grp = J.make_group(40 + a, shapes, scale)
        ps = [torch.nn.Parameter(torch.from_numpy(p).double()) for p in grp["p"]]
        cls = torch.optim.AdamW if o["decoupled"] else torch.optim.Adam
        # (the judge's hyperparameters ARE the float32 values: torch gets the same numbers)
        opt = cls(ps, lr=float(o["lr"]), betas=(float(o["beta1"]), float(o["beta2"])), eps=float(o["eps"]), weight_decay=float(o["wd"]),
                  foreach=False)
        p, m, v, t = grp["p"], grp["m"], grp["v"], 0
        for step in range(5):
            g = grp["g"] if step == 0 else J.fresh_gradients(90 + 10 * step + a, grp, scale)
            for q, gi in zip(ps, g):
                q.grad = torch.from_numpy(gi).double()
            if J.clipping(o):
                total = torch.nn.utils.clip_grad_norm_(ps, float(o["max_norm"]), foreach=False)
            p, m, v, t, norm, coef, skipped = J.step64(p, g, m, v, t, o)
            opt.step()
            assert not skipped and t == step + 1
            if J.clipping(o):
                assert abs(float(total) - norm) <= 1e-14 * max(norm, 1e-300)
                engaged.append(coef < 1)
            for q, pi, mi, vi in zip(ps, p, m, v):
                st = opt.state[q]
                for got, want in ((pi, q.detach().numpy()), (mi, st["exp_avg"].numpy()), (vi, st["exp_avg_sq"].numpy())):
                    assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-30), (name, step)
            if scale == 0.0:
                assert norm == 0.0 and coef == 1.0 and all(np.array_equal(pi, p0) for pi, p0 in zip(p, grp["p"]))
    if name == "adam_clip_engaged":
        assert all(engaged)
    if name == "adam_clip_idle":
        assert not any(engaged)


PER_TENSOR = dict(p=0.0, m=0.0, v=0.0)  # the worst share of each output since it was last cleared


def run_case(index, shapes, o, device, steps=J.STEPS, t=0, lr=None):
    """`steps` consecutive steps of `device` (a function of (group, options) -> dict(p, m, v, t, skipped, norm, coef)), each
    judged from the state the previous one left.  Returns (worst share, elements beyond, whether a clip engaged)."""
    groups = J.case_groups(index, shapes, t)
    worst, beyond, engaged = 0.0, 0, []
    for step in range(steps):
        for a, grp in enumerate(groups):
            if step:
                grp["g"] = J.case_gradients(index, a, step, grp)
            verdict = J.judge(grp, o, lr)
            for e in verdict["ep"] + verdict["em"] + verdict["ev"]:
                assert np.isfinite(e).all() and (e > 0).all(), "a tolerance of a test's own case is not finite"
            got = device(grp, o)
            w, b = J.check_group(got, verdict)
            for name in PER_TENSOR:
                PER_TENSOR[name] = max(PER_TENSOR[name], J.worst_share(got[name], verdict[name], verdict["e" + name])[0])
            assert got["t"] == verdict["t"] == t + step + 1 and got["skipped"] == verdict["skipped"] == 0
            if not (abs(float(got["norm"]) - verdict["norm"]) <= verdict["e_norm"] and abs(float(got["coef"]) - verdict["coef"]) <= verdict["e_coef"]):
                b += 1
            worst, beyond = max(worst, w), beyond + b
            engaged.append(verdict["coef"] < 1)
            grp.update(p=got["p"], m=got["m"], v=got["v"], t=got["t"])
    return worst, beyond, engaged


RESTATEMENT_SHARE = 1.0


def test_float32_restatement_stays_under_a_share_of_the_tolerance():
    """A float32 numpy restatement of the header's operation order on every case of the GPU tests, three steps each, and on the
    planted step counts.  These tolerances are TIGHT by construction: a parameter's update is orders of magnitude below the
    parameter, and from the second step on a moment is mostly its old value, so each bound is little more than the final
    rounding's U |x'|, which a correctly rounded result just above a power of two all but reaches.  Observed here: 0.989 (p),
    0.993 (m), 0.899 (v) of the tolerance; asserted: no element beyond it (a share of 1).  Clip engaged and idle both occur."""
    for name in PER_TENSOR:
        PER_TENSOR[name] = 0.0
    worst, engaged = 0.0, []
    for index, (name, shapes, oname) in enumerate(J.gpu_cases()):
        w, beyond, e = run_case(index, shapes, J.case_options(oname), J.restate_float32)
        assert not beyond, name
        print(f"{name}: worst error / tolerance {w:.4f}")
        worst = max(worst, w)
        if oname == "clip_engaged":
            engaged += e
    for t in J.PLANTED_T:
        w, beyond, _ = run_case(70, [J.DEFAULT_NET], J.options(lr=3e-4, betas=J.PLANTED_BETAS, eps=1e-8, max_grad_norm=0.5), J.restate_float32, steps=1, t=t)
        assert not beyond, t
        worst = max(worst, w)
    print(f"worst error / tolerance over all cases {worst:.4f}")
    assert any(engaged) and not all(engaged)
    print("worst share per output", {k: round(v, 4) for k, v in PER_TENSOR.items()})
    assert all(0 < PER_TENSOR[name] <= RESTATEMENT_SHARE for name in PER_TENSOR), PER_TENSOR


def test_every_mutant_exceeds_the_tolerance_on_the_gpu_tests_own_cases():
    """each of the seven mutants leaves the tolerance on a case that tests/test_gpu_optim.py runs"""
    cases = J.gpu_cases()
    names = [c[0] for c in cases]

    def on(name, mutant, **kw):
        index = names.index(name)
        _, shapes, oname = cases[index]
        return run_case(index, shapes, J.case_options(oname), lambda g, o, lr=None: J.restate_float32(g, o, lr, mutant=mutant), **kw)[:2]

    killers = {"no_bias_correction": "default_net_no_clip", "eps_inside_sqrt": "default_net_clip_engaged", "clip_without_1e-6": "single_1024",
               "norm_of_first_tensor": "default_net_clip_engaged", "decay_swapped": "default_net_l2_decay", "beta1_for_beta2": "single_65"}
    for mutant, name in killers.items():
        share, beyond = on(name, mutant, steps=1)
        print(mutant, name, f"{share:.3g}", beyond)
        assert share > 1 and beyond, (mutant, name, share)
    share, beyond = on("default_net_adamw", "decay_swapped", steps=1)
    assert share > 1 and beyond
    # the float32 pow at t = 10^6 (the planted step counts of the GPU tests); harmless at t = 0, where b^1 is exact
    planted = J.options(lr=3e-4, betas=J.PLANTED_BETAS, eps=1e-8, max_grad_norm=0.5)
    mutated = lambda g, o, lr=None: J.restate_float32(g, o, lr, mutant="float32_pow")  # noqa: E731
    share, beyond, _ = run_case(70, [J.DEFAULT_NET], planted, mutated, steps=1, t=999_999)
    print("float32_pow", f"{share:.3g}", beyond)
    assert share > 1 and beyond
    assert set(killers) | {"float32_pow"} == set(J.MUTANTS) and len(J.MUTANTS) == 7


def test_the_exact_pin_is_exact_in_float32():
    grp, o, want = J.exact_pin_case()
    got = J.restate_float32(grp, o)
    for name in ("p", "m", "v"):
        for g, w, before in zip(got[name], want[name], grp[name]):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), w.view(np.int32)), name
            assert not np.array_equal(g, before)
    assert got["t"] == 1 and got["coef"] == 1
    lr = float(o["lr"])
    assert all(np.array_equal(np.abs(a.astype(np.float64) - b), np.full(a.shape, lr)) for a, b in zip(got["p"], grp["p"]))
    # and the judge agrees with it to the last bit: its float64 values ARE float32 values here
    verdict = J.judge(grp, o)
    assert all(np.array_equal(r, w.astype(np.float64)) for name in ("p", "m", "v") for r, w in zip(verdict[name], want[name]))


def test_sum_of_squares_in_kernel_order_is_the_sum():
    rng = np.random.default_rng(1)
    for sizes in ((1,), (63, 2), (1024,), (1025, 7, 4097), (31016,)):
        g = [rng.standard_normal(n).astype(np.float32) for n in sizes]
        want = sum(float((x.astype(np.float64) ** 2).sum()) for x in g)
        got = J.sum_of_squares_in_kernel_order(g)
        assert abs(got - want) <= (sum(sizes) + 32) * J.D * want
    assert J.sum_of_squares_in_kernel_order([np.zeros(5, np.float32)]) == 0.0
    assert np.isnan(J.sum_of_squares_in_kernel_order([np.array([1, np.nan], np.float32)]))
    assert np.isinf(J.sum_of_squares_in_kernel_order([np.array([1, np.inf, 3e38], np.float32)]))
    assert np.isfinite(J.sum_of_squares_in_kernel_order([np.full(1 << 20, 3.4e38, np.float32)]))  # float64 does not overflow


def test_nonfinite_gradients_as_the_header_says():
    """what a NaN and an infinity reach, in the judge and in the restatement alike"""
    for bad, clip in ((np.nan, 0.5), (np.inf, 0.5), (np.nan, None), (-np.inf, None)):
        for skip in (False, True):
            grp = J.make_group(3, ((5, 3), (7,)), J.GRAD_SCALE, t=4)
            grp["g"][1][2] = bad
            o = J.options(max_grad_norm=clip, skip_nonfinite=skip)
            verdict, got = J.judge(grp, o), J.restate_float32(grp, o)
            assert not np.isfinite(verdict["norm"]) and not np.isfinite(got["norm"])
            assert J.check_group(got, verdict)[1] == 0
            if skip:
                assert verdict["did_skip"] and got["t"] == verdict["t"] == 4 and got["skipped"] == verdict["skipped"] == 1
                assert all(np.array_equal(a, b) for name in ("p", "m", "v") for a, b in zip(got[name], grp[name]))
                continue
            assert got["t"] == verdict["t"] == 5 and got["skipped"] == 0
            everything = np.concatenate([x.reshape(-1) for name in ("p", "m", "v") for x in verdict[name]])
            if clip and np.isnan(bad):
                assert np.isnan(everything).all()                                 # coef is NaN: the whole group
            else:
                # (0 * inf is NaN under a clip, and so is a NaN without one: p, m and v; an unclipped infinity leaves m and v infinite)
                assert np.isnan(verdict["p"][1][2]) and np.isnan(everything).sum() == (1 if clip is None and np.isinf(bad) else 3)
                assert np.isfinite(verdict["p"][0]).all()
