"""CPU tests (no GPU needed) of the batch library: libpikazoo_batch.so exports its header's four symbols and carries the tree's
build id, nothing loads it before its first use, its code object holds three kernels without scratch or spilled registers, the
entry points refuse bad arguments before any launch and in the documented order, ``pikazoo_amd.batch`` raises ``ValueError``
for malformed arguments before it needs the library, and the judge the GPU tests compare with (tests/batch_judge.py) is the
header's permutation: a bijection, equal to a second scalar formulation, different per epoch and seed, a partition per epoch,
and sharp enough that six mutants fail on the GPU tests' own shapes.

No call here ever passes every check with rows to move: a call that did would launch a kernel on fake pointers wherever a
GPU is present.  A check is shown to PASS by planting a failure of a later one."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import batch_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_batch_abi_version", "pz_batch_build_id", "pz_batch_copy", "pz_batch_gather"]
KERNELS = ["pz_batch::batch_kernel<0>", "pz_batch::batch_kernel<1>", "pz_batch::batch_kernel<2>"]
COPY_DECL = "int pz_batch_copy(const pz_batch_column *cols, int32_t ncols, int64_t n, void *stream);"
GATHER_DECL = ("int pz_batch_gather(const pz_batch_column *cols, int32_t ncols, int64_t k, int64_t n, int64_t minibatches, uint64_t seed, "
               "uint64_t counter, const uint64_t *counter_dev, const int64_t *index_in, int64_t *index_out, uint32_t *errors, void *stream);")


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.batch, the judge's included: none of them runs without the module"""
    from pikazoo_amd import batch

    return batch


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import batch

    return batch.load()


def test_batch_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, batch, learn, net, netgrad, optim, policy, ppo

    assert header_functions("pikazoo_batch.h") == NAMES == sorted(batch.SIGNATURES) == dynamic_pz_symbols(pz_build.BATCH_LIB)
    assert pz_build.library_id(pz_build.BATCH_LIB) == pz_build.source_id() == lib.pz_batch_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.BATCH_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_batch.h") in pz_build.DEPS
    assert lib.pz_batch_abi_version() == batch.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_batch.h").read_text()
    assert "#define PZ_BATCH_ABI_VERSION 1" in header
    assert f"#define PZ_BATCH_MAX_COLUMNS {batch.MAX_COLUMNS}\n" in header and batch.MAX_COLUMNS == 16
    assert f"#define PZ_BATCH_MAX_ROW_BYTES {batch.MAX_ROW_BYTES}\n" in header and batch.MAX_ROW_BYTES == 512
    # the struct of the binding is the header's: two pointers, three int64 pitches, two int32
    assert C.sizeof(batch.Column) == 48
    body = re.search(r"typedef struct pz_batch_column \{(.*?)\} pz_batch_column;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in batch.Column._fields_]
    # no other library holds any of the names, and the older libraries' ABI versions did not move
    others = (pz_build.LIB, pz_build.LEARN_LIB, pz_build.DIAG_LIB, pz_build.POLICY_LIB, pz_build.PPO_LIB, pz_build.NET_LIB, pz_build.NETGRAD_LIB,
              pz_build.OPTIM_LIB)
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
    assert optim.load().pz_optim_abi_version() == optim.ABI_VERSION == 1
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_batch.h" in doc and "libpikazoo_batch.so" in doc
    for decl in (COPY_DECL, GATHER_DECL):
        assert decl in doc and decl in header


def test_importing_the_other_modules_does_not_load_the_batch_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim; "
            "assert 'pikazoo_amd.batch' not in sys.modules; import pikazoo_amd as p; assert 'batch' in p.__all__; "
            "p.batch.copy; p.batch.gather; p.batch.permutation; p.batch.RolloutBuffer; "
            "assert 'pikazoo_amd.batch' in sys.modules and p.batch._lib is None; "
            "assert not any('libpikazoo_batch' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_batch_library(pz_build):
    """THREE kernels -- the copy, the permuted gather, the indexed gather; columns, widths and pitches are run-time.  None uses
    scratch or spills; the gathers' LDS is the 256 (step, game) pairs of a tile, the copy has none.  Read from the code object's
    notes alone: nothing is disassembled."""
    import kernel_notes

    notes = kernel_notes.notes(pz_build.BATCH_LIB)
    short = lambda name: name.replace("void ", "").split("(")[0]  # noqa: E731
    assert sorted(short(name) for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == (0 if short(name).endswith("<0>") else 256 * 8), (name, row)
        assert row[".vgpr_count"] + row.get(".agpr_count", 0) <= 128 and row.get(".agpr_count", 0) == 0, (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".sgpr_count") if k in row})


# ---- argument checking ------------------------------------------------------------------------------------------------------
FAKE = 4096


def columns(ncols=3, **by_index):
    """good fake columns (140-byte float32 rows); `c<index>={field: value}` overwrites fields of one"""
    from pikazoo_amd import batch

    array = (batch.Column * 16)()
    for i in range(16):
        array[i] = batch.Column(FAKE + 1024 * i, FAKE + 65536 + 1024 * i, 140 * 64, 140, 140, 140, 4)
    for i, fields in ((int(key[1:]), fields) for key, fields in by_index.items()):
        for field, value in fields.items():
            setattr(array[i], field, value)
    return array


def gather_call(lib, ncols=3, k=2, n=64, minibatches=4, counter=0, cols_null=False, counter_dev=None, index_in=None, index_out=None, errors=FAKE + 2,
                **overrides):
    """pz_batch_gather on fake pointers; by default the LAST check fails (errors is not 4-byte aligned)"""
    return lib.pz_batch_gather(None if cols_null else columns(ncols, **overrides), ncols, k, n, minibatches, 7, counter, counter_dev, index_in, index_out,
                               errors, None)


def copy_call(lib, ncols=3, n=64, cols_null=False, **overrides):
    return lib.pz_batch_copy(None if cols_null else columns(ncols, **overrides), ncols, n, None)


def test_argument_validation_of_gather(lib):
    """Every return code in the documented order.  The LAST check (the alignment of `errors`) is planted in every call that is
    meant to pass the earlier ones: -4 then says that NULL, size, configuration and column alignment checks all passed."""
    passes = lambda **kw: gather_call(lib, **kw) == -4  # noqa: E731
    assert passes() and passes(ncols=16) and passes(ncols=1) and passes(ncols=0, index_out=FAKE) and passes(minibatches=128) and passes(minibatches=1)
    assert passes(k=1 << 31, n=1) and passes(k=1, n=1 << 31) and passes(counter=(1 << 62) - 1) and passes(counter_dev=FAKE + 8, index_out=FAKE + 16)
    # NULL
    assert gather_call(lib, cols_null=True) == -1 and gather_call(lib, ncols=0) == -1
    for i in (0, 2):
        for field in ("src", "dst"):
            assert lib.pz_batch_gather(columns(3, **{f"c{i}": {field: None}}), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -1
    assert lib.pz_batch_gather(columns(3, **{f"c{3}": {"src": None}}), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -4   # behind ncols: not looked at
    # sizes
    for bad in (dict(ncols=17), dict(ncols=-1), dict(k=0), dict(k=-1), dict(n=-1), dict(k=1 << 31, n=2), dict(k=3, n=1 << 30), dict(minibatches=0),
                dict(minibatches=129), dict(minibatches=-4), dict(counter=1 << 62), dict(counter=(1 << 64) - 1)):
        assert gather_call(lib, **bad) == -2, bad

    def with_column(**fields):
        return lib.pz_batch_gather(columns(3, **{f"c{1}": fields}), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None)

    for fields in (dict(row_bytes=0), dict(row_bytes=-4), dict(row_bytes=516, src_game_pitch=516, dst_pitch=516), dict(src_game_pitch=136),
                   dict(dst_pitch=136), dict(src_step_pitch=136), dict(src_step_pitch=-140 * 64), dict(dst_pitch=0),
                   dict(src_game_pitch=1 << 58), dict(dst_pitch=1 << 59)):                                  # (the last two: an extent beyond int64)
        assert with_column(**fields) == -2, fields
    assert lib.pz_batch_gather(columns(3, c1=dict(src_step_pitch=1 << 62)), 3, 4, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -2   # 3 x 2^62
    for fields in (dict(row_bytes=512, src_game_pitch=512, dst_pitch=512), dict(row_bytes=4, src_game_pitch=76), dict(src_step_pitch=140),
                   dict(src_step_pitch=1 << 61), dict(dst_pitch=1 << 40), dict(row_bytes=1, elem_bytes=1), dict(elem_bytes=2), dict(elem_bytes=1)):
        assert with_column(**fields) == -4, fields
    # with index_in, `minibatches` carries B: 0 .. 2^31, and seed and the counters are not looked at
    assert gather_call(lib, index_in=FAKE, minibatches=1 << 31, counter=1 << 63) == -4
    assert gather_call(lib, index_in=FAKE, minibatches=(1 << 31) + 1) == -2 and gather_call(lib, index_in=FAKE, minibatches=-1) == -2
    # configuration
    for e in (0, 3, 5, 16, -1):
        assert with_column(elem_bytes=e) == -3, e
    # alignment
    for fields in (dict(src=FAKE + 2), dict(dst=FAKE + 65536 + 1), dict(src_game_pitch=142), dict(dst_pitch=141), dict(src_step_pitch=140 * 64 + 2),
                   dict(row_bytes=138), dict(elem_bytes=8)):
        assert with_column(**fields) == -4, fields
    ok = FAKE + 64
    for kw in (dict(counter_dev=FAKE + 4), dict(index_in=FAKE + 4, minibatches=8), dict(index_out=FAKE + 12), dict(errors=FAKE + 1), dict(errors=FAKE + 3)):
        assert gather_call(lib, **{"errors": ok, **kw}) == -4, kw
    # nothing to move: PZ_OK without a launch, behind every check
    assert gather_call(lib, n=0, errors=ok) == 0 and gather_call(lib, index_in=FAKE, minibatches=0, errors=ok) == 0
    assert gather_call(lib, n=0) == -4 and gather_call(lib, n=0, ncols=17, errors=ok) == -2
    # the order of the checks: NULL, size, config, alignment
    everything = {"c1": dict(src=None), "c2": dict(row_bytes=0, elem_bytes=3, dst=FAKE + 65536 + 2049)}
    assert lib.pz_batch_gather(columns(3, **everything), 3, 0, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -1
    del everything["c1"]
    assert lib.pz_batch_gather(columns(3, **everything), 3, 0, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -2   # k
    assert lib.pz_batch_gather(columns(3, **everything), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -2   # row_bytes
    everything["c2"]["row_bytes"] = 140
    assert lib.pz_batch_gather(columns(3, **everything), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -3
    everything["c2"]["elem_bytes"] = 4
    assert lib.pz_batch_gather(columns(3, **everything), 3, 2, 64, 4, 7, 0, None, None, None, FAKE + 2, None) == -4


def test_argument_validation_of_copy(lib):
    """pz_batch_copy: the same order; its planted last failure is a misaligned dst of the last column"""
    plant = {"c2": dict(dst=FAKE + 65536 + 2050)}

    def call(ncols=3, n=64, **fields):
        over = dict(plant)
        if fields:
            over["c1"] = fields
        return lib.pz_batch_copy(columns(ncols, **over), ncols, n, None)

    assert call() == -4 and call(n=1 << 31) == -4 and call(src_step_pitch=-3) == -4 and call(src_step_pitch=0) == -4      # the step pitch is ignored
    assert call(row_bytes=4, src_game_pitch=76, dst_pitch=4) == -4
    assert copy_call(lib, cols_null=True) == -1 and copy_call(lib, ncols=0) == -1 and call(src=None) == -1 and call(dst=None) == -1
    for bad in (dict(ncols=17), dict(ncols=-2), dict(n=-1), dict(n=(1 << 31) + 1)):
        assert copy_call(lib, **bad) == -2, bad
    for fields in (dict(row_bytes=0), dict(row_bytes=516, src_game_pitch=516, dst_pitch=516), dict(src_game_pitch=136), dict(dst_pitch=100),
                   dict(src_game_pitch=1 << 62)):
        assert call(**fields) == -2, fields
    assert call(elem_bytes=3) == -3 and call(elem_bytes=0) == -3
    for fields in (dict(src=FAKE + 1), dict(dst=FAKE + 65536 + 3), dict(src_game_pitch=141), dict(dst_pitch=142), dict(row_bytes=139), dict(elem_bytes=8)):
        assert lib.pz_batch_copy(columns(3, **{f"c{1}": fields}), 3, 64, None) == -4, fields
    assert copy_call(lib, n=0) == 0 and call(n=0) == -4
    assert call(src=None, row_bytes=0, elem_bytes=3, n=-1) == -1 and call(row_bytes=0, elem_bytes=3, n=-1) == -2
    assert call(row_bytes=0, elem_bytes=3) == -2 and call(elem_bytes=3) == -3


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device, overlap, stride and range errors raise ValueError -- on CPU tensors the device check stands behind
    the others, so every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import batch

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(batch, "load", refuse)
    n, k = 8, 3
    head = torch.zeros(n, 19)
    good = lambda: [(torch.zeros(n, 35), torch.zeros(n, 35)), (head[:, 18], torch.zeros(n)), (torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)),  # noqa: E731
                    (torch.zeros(n, 35, dtype=torch.bfloat16), torch.zeros(k, n, 35, dtype=torch.bfloat16)[1]), (torch.zeros(n, 2, 3), torch.zeros(n, 2, 3))]
    with pytest.raises(ValueError, match="GPU"):
        batch.copy(good())
    big = torch.zeros(64)
    bad_copies = [
        [], [(torch.zeros(n), torch.zeros(n))] * 17, torch.zeros(n), [(torch.zeros(n),)], [(torch.zeros(n), None)], [torch.zeros(n)],
        [(torch.zeros(n, 35), torch.zeros(n, 36))], [(torch.zeros(n), torch.zeros(n + 1))],                          # shape
        [(torch.zeros(n), torch.zeros(n)), (torch.zeros(n + 1), torch.zeros(n + 1))], [(torch.zeros(()), torch.zeros(()))],
        [(torch.zeros(n), torch.zeros(n, dtype=torch.float64))], [(torch.zeros(n, dtype=torch.int32), torch.zeros(n))],   # dtype
        [(torch.zeros(n, dtype=torch.complex64), torch.zeros(n, dtype=torch.complex64))],
        [(torch.zeros(n), torch.zeros(n, device="meta"))],                                                           # device
        [(big[0:8], big[7:15])], [(big[0:8], big[0:8])], [(torch.zeros(n), big[0:8]), (torch.zeros(n), big[4:12])],      # overlap
        [(torch.zeros(35, n).t(), torch.zeros(n, 35))], [(torch.zeros(n, 35), torch.zeros(n, 70)[:, ::2])],               # stride
        [(torch.zeros(n, 4), torch.zeros(1, 4).expand(n, 4))], [(torch.zeros(n, 129), torch.zeros(n, 129))],               # rows overlap; 516 bytes
    ]
    for i, bad in enumerate(bad_copies):
        with pytest.raises(ValueError):
            batch.copy(bad)
            pytest.fail(f"bad copy {i} was accepted")

    def sources():
        return {"obs": {"a": torch.zeros(k, n, 35), "b": torch.zeros(k, n, 35)}, "act": {"a": torch.zeros(k, n, dtype=torch.int64)},
                "val": torch.zeros(k + 1, n)[:k], "flags": torch.zeros(k, n, dtype=torch.bool)}

    with pytest.raises(ValueError, match="GPU"):
        batch.gather(sources(), 4, 0)
    with pytest.raises(ValueError, match="GPU"):
        batch.gather(sources(), 4, 0, counter=5, counter_dev=torch.zeros(1, dtype=torch.int64), index_out=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):
        batch.gather(sources(), 1, 0, index=torch.zeros(5, dtype=torch.int64), errors=torch.zeros(1, dtype=torch.int32))
    prev = {"obs": {"a": torch.zeros(6, 35), "b": torch.zeros(6, 35)}, "act": {"a": torch.zeros(6, dtype=torch.int64)}, "val": torch.zeros(6),
            "flags": torch.zeros(6, dtype=torch.bool)}
    with pytest.raises(ValueError, match="GPU"):
        batch.gather(sources(), 4, 0, out=prev)
    src = sources()
    bad_gathers = [
        dict(sources={}), dict(sources={"x": 1.0}), dict(sources={"x": torch.zeros(n)}),
        dict(sources={**src, "more": torch.zeros(k, n + 1)}), dict(sources={**src, "more": torch.zeros(k + 1, n)}),
        dict(sources={str(i): torch.zeros(k, n) for i in range(17)}), dict(sources={"x": torch.zeros(k, n, 129)}),
        dict(sources={"x": torch.zeros(k, 35, n).transpose(1, 2)}), dict(sources={"x": torch.zeros(k, n, dtype=torch.complex64)}),
        dict(sources={"x": torch.zeros(1, 1, 4).expand(k, n, 4)}), dict(sources={"x": torch.zeros(k, 0)}),
        dict(minibatches=0), dict(minibatches=k * n + 1), dict(minibatches=2.0), dict(minibatches=True), dict(counter=-1), dict(counter=1 << 62),
        dict(counter=1.5), dict(seed="7"), dict(seed=1.0),
        dict(counter_dev=torch.zeros(1, dtype=torch.int32)), dict(counter_dev=torch.zeros(2, dtype=torch.int64)), dict(counter_dev=3),
        dict(index=torch.zeros(4, dtype=torch.int32)), dict(index=torch.zeros(4, 2, dtype=torch.int64)), dict(index=torch.zeros(8, dtype=torch.int64)[::2]),
        dict(index=[1, 2]), dict(index_out=torch.zeros(5, dtype=torch.int64)), dict(index_out=torch.zeros(6, dtype=torch.int32)),
        dict(errors=torch.zeros(1, dtype=torch.int64)), dict(errors=torch.zeros(2, dtype=torch.int32)),
        dict(out={"obs": prev["obs"]}), dict(out={**prev, "val": torch.zeros(7)}), dict(out={**prev, "val": torch.zeros(6, dtype=torch.float64)}),
        dict(out={**prev, "obs": {"a": prev["obs"]["a"], "b": prev["obs"]["a"]}}),                                   # two outputs overlap
        dict(out={**prev, "val": src["val"][0, :6]}),                                                              # an output overlaps a source
        dict(out={**prev, "flags": torch.zeros(6, dtype=torch.bool, device="meta")}),
    ]
    for i, bad in enumerate(bad_gathers):
        kw = dict(sources=src, minibatches=4, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            batch.gather(**kw)
            pytest.fail(f"bad gather {i} was accepted: {sorted(bad)}")
    for bad in (dict(M=0), dict(M=(1 << 31) + 1), dict(M=2.0), dict(epoch=-1), dict(epoch=1 << 62), dict(seed=None), dict(device="cpu")):
        with pytest.raises(ValueError):
            batch.permutation(**{**dict(M=16, seed=0, epoch=0), **bad})
    # the rollout buffer
    agents = ("p1", "p2")
    step = lambda: dict(obs={a: torch.zeros(n, 35) for a in agents}, actions={a: torch.zeros(n, dtype=torch.int64) for a in agents},  # noqa: E731
                        log_probs={a: torch.zeros(n) for a in agents}, head={a: torch.zeros(n, 19) for a in agents},
                        rewards={a: torch.zeros(n, dtype=torch.int32) for a in agents}, terminations={a: torch.zeros(n, dtype=torch.bool) for a in agents})
    buf = batch.RolloutBuffer(k, n, step(), minibatches=4, seed=1)
    assert buf.obs["p1"].shape == (k, n, 35) and buf.values["p2"].shape == (k + 1, n) and buf.rewards["p1"].dtype == torch.int32
    assert buf.terminations.shape == (k, n) and buf.terminations.dtype == torch.bool and buf.actions["p1"].dtype == torch.int64
    with pytest.raises(ValueError, match="GPU"):
        buf.store(1, **step())
    s = step()
    for bad in (dict(t=0, **s), dict(t=k, **s), dict(t=k + 1, head=s["head"]), dict(t=-1, head=s["head"]), dict(t=1), dict(t=1, obs=s["obs"]["p1"]),
                dict(t=1, obs={"p1": s["obs"]["p1"]}), dict(t=1, head={a: torch.zeros(n) for a in agents}), dict(t=1, obs={a: torch.zeros(n, 36) for a in agents}),
                dict(t=1, rewards={a: torch.zeros(n) for a in agents}), dict(t=0, terminations=s["terminations"]), dict(t=1.0, head=s["head"])):
        with pytest.raises(ValueError):
            buf.store(**bad)
            pytest.fail(f"bad store {sorted(bad)} was accepted")
    with pytest.raises(ValueError, match="set_targets"):
        buf.minibatch()
    for bad in ({}, {"advantages": {a: torch.zeros(k, n) for a in agents}}, {"advantages": {a: torch.zeros(k, n) for a in agents}, "returns": {"p1": torch.zeros(k, n)}},
                {"advantages": {a: torch.zeros(k, n) for a in agents}, "returns": {a: torch.zeros(k + 1, n) for a in agents}}):
        with pytest.raises(ValueError):
            buf.set_targets(bad)
    buf.set_targets({"advantages": {a: torch.zeros(k, n) for a in agents}, "returns": {a: torch.zeros(k, n) for a in agents}})
    with pytest.raises(ValueError, match="GPU"):
        buf.minibatch(counter=3)
    for bad in (dict(example_step={}), dict(k=0), dict(n=0), dict(example_step={**step(), "obs": {a: torch.zeros(n + 1, 35) for a in agents}}),
                dict(example_step={**step(), "rewards": {"p1": torch.zeros(n)}})):
        with pytest.raises(ValueError):
            batch.RolloutBuffer(**{**dict(k=k, n=n, example_step=step()), **bad})


# ---- the judge --------------------------------------------------------------------------------------------------------------
def test_the_permutation_is_a_bijection():
    sizes = set(J.BIJECTION_M)
    for b in range(2, 14):
        sizes |= {(1 << b) - 1, 1 << b, (1 << b) + 1}
    for M in sorted(sizes):
        for epoch in range(3):
            walks = []
            r = J.perm(np.arange(M), M, 5, epoch, walks=walks)
            assert r.min() >= 0 and r.max() < M and np.array_equal(np.sort(r), np.arange(M)), (M, epoch)
            if M == 4097:
                assert 3.5 < walks[0].mean() < 4.0          # the domain is 16384: below 4 passes on average
            if M in (64, 1024, 4096):
                assert walks[0].max() == 1                   # a power of four: the domain is [0, M)


def test_a_scalar_formulation_agrees():
    for M, seed, epoch in ((1, 0, 0), (2, 1, 0), (5, 7, 3), (65, 7, 1), (241, 1 << 63, 9), (4097, 0xDEADBEEFCAFEF00D, (1 << 40) + 5), (1 << 31, 3, 2)):
        ps = np.unique(np.concatenate([np.arange(min(M, 40)), np.array([M - 1, M // 2])]))
        want = [J.perm_scalar(int(p), M, seed, epoch) for p in ps]
        assert J.perm(ps, M, seed, epoch).tolist() == want, (M, seed, epoch)


def test_epochs_seeds_and_the_env_key_give_other_permutations():
    from oracle.pz_oracle import philox4x32_10_numpy

    M = 4097
    base = J.perm(np.arange(M), M, 7, 0)
    for other in (J.perm(np.arange(M), M, 7, 1), J.perm(np.arange(M), M, 8, 0), J.perm(np.arange(M), M, 7 + (1 << 32), 0), J.perm(np.arange(M), M, 7, 1 << 32)):
        assert (other != base).mean() > 0.99
    # the round keys are not what the env's own key (the plain seed) gives at the same counters
    for seed in (0, 7, 0x123456789ABCDEF0):
        w = philox4x32_10_numpy((np.zeros(2), np.zeros(2), np.arange(2), np.zeros(2)), (seed & 0xFFFFFFFF, seed >> 32))
        plain = [int(w[i][0]) for i in range(4)] + [int(w[0][1]), int(w[1][1])]
        assert not set(plain) & set(J.round_keys(seed, 0))
    assert J.philox_key(0) == (0x53485546, 0x42415443)


def test_the_minibatches_of_an_epoch_partition_it():
    for k, n, mb in J.basic_shapes() + [(1, 1000, 7), (3, 4099, 5)]:
        M = k * n
        B = M // mb
        for epoch in (0, 3):
            rows = np.concatenate([J.minibatch_rows(M, mb, 11, epoch * mb + m) for m in range(mb)])
            assert len(rows) == B * mb and len(np.unique(rows)) == B * mb and rows.min() >= 0 and rows.max() < M
            # they are the permutation's first B * minibatches positions: the tail is dropped, not wrapped
            assert np.array_equal(rows, J.perm(np.arange(B * mb), M, 11, epoch))


def test_every_mutant_is_caught_by_the_gpu_tests_own_shapes():
    """what the GPU test compares -- the source offset of every output row of a float32 column, at every shape and counter it
    runs -- differs from the definition's under each of the six mutants"""
    col = J.SIMPLE[0]
    caught = {m: 0 for m in J.MUTANTS}
    for k, n, mb in J.basic_shapes():
        c = J.sized(col, k, n)
        for counter in J.counters(mb):
            want = J.source_offsets(J.minibatch_rows(k * n, mb, 3, counter), n, c["step_pitch"], c["game_pitch"])
            for m in J.MUTANTS:
                got = J.source_offsets(J.minibatch_rows(k * n, mb, 3, counter, mutant=m), n, c["step_pitch"], c["game_pitch"], mutant=m)
                caught[m] += not np.array_equal(got, want)
    print(caught)
    assert len(J.MUTANTS) == 6 and all(count > 0 for count in caught.values()), caught
