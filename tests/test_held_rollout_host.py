"""CPU tests of the k-step trajectory launches of a frame-skip env (``pz_step_many_held``, ``pz_rollout_random_held``,
the ``held_traj_kernel`` family; ``raw_env.step_many_held`` / ``rollout_random_held``): the C ABI without a device, the
code object, the Python surface, and -- on the judge alone -- that the cases of tests/test_gpu_held_rollout.py bite."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from frame_skip_judge import HeldOracle
from held_rollout_cases import BITING, held_traj_kernels, judge_counts, make_judge, policy

REPO = Path(__file__).resolve().parent.parent
NEW = {"pz_step_many_held": 16, "pz_rollout_random_held": 18}


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build as pz_build

    return pz_build.build()


def _declaration(name):
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_hip.h").read_text(), flags=re.S)
    decl = re.search(rf"int {name}\((.*?)\);", header, flags=re.S)
    assert decl, f"{name} is not declared in include/pikazoo_hip.h"
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_both_entry_points_are_declared_bound_and_exported(built_lib):
    from pikazoo_amd import _native

    many, roll = _declaration("pz_step_many_held"), _declaration("pz_rollout_random_held")
    assert len(many) == 16 and many[4:7] == ["const void *actions", "int32_t k", "int32_t hold"]
    assert many[13] == "int64_t *episodes_done"
    assert len(roll) == 18 and roll[4:9] == ["uint64_t action_seed", "uint64_t t0", "int32_t k", "int32_t hold",
                                             "int32_t *actions"]
    assert roll[15] == "int64_t *episodes_done"
    dll = C.CDLL(str(built_lib))
    for name, count in NEW.items():
        assert name in _native.exported_names()
        restype, argtypes = _native._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == count
        assert hasattr(dll, name)
    sig = _native._SIGNATURES
    assert sig["pz_step_many_held"][1][5:7] == [C.c_int32, C.c_int32]
    assert sig["pz_rollout_random_held"][1][4:8] == [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32]
    # one argument (`hold`, behind k) more than the sibling, everything else the sibling's
    for held, plain, at in (("pz_step_many_held", "pz_step_many", 6), ("pz_rollout_random_held", "pz_rollout_random", 7)):
        args = list(sig[held][1])
        assert args.pop(at) is C.c_int32 and args == list(sig[plain][1])
    lib = _native.load()
    assert lib.pz_abi_version() == 10 and lib.pz_config_bytes() == 120  # additive: same ABI, same configuration block


def test_the_entry_points_validate_their_arguments_without_a_gpu(built_lib):
    """Argument errors are reported before anything touches the device (no launch on these paths)."""
    from pikazoo_amd import _native

    lib = _native.load()
    cfg = _native.PzConfig()
    cfg.winning_score, cfg.serve_mode = 15, 0
    fake = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    ref = C.byref(cfg)

    def many(state=fake, n=0, stride=0, tape=fake, k=4, hold=4, o1=fake, o2=fake, r1=fake, r2=fake, term=fake, tables=None):
        return lib.pz_step_many_held(state, n, stride, ref, tape, k, hold, o1, o2, r1, r2, term, None, None, tables, None)

    def roll(state=fake, n=0, stride=0, tape=None, k=4, hold=4, o1=fake, o2=fake, r1=fake, r2=fake, term=fake, tables=None):
        return lib.pz_rollout_random_held(state, n, stride, ref, 1, 0, k, hold, tape, o1, o2, r1, r2, term, None, None,
                                          tables, None)

    for call in (many, roll):
        cfg.action_format = cfg.normalize_obs = cfg.packed_state = 0
        assert call() == 0                                      # empty batch: no-op
        assert call(k=1, hold=1) == 0
        assert call(k=0) == -2 and call(k=-3) == -2             # PZ_E_SIZE, as the siblings' k < 1
        assert call(hold=0) == -2 and call(hold=-1) == -2
        assert call(state=None) == -1                           # PZ_E_NULL
        for name in ("o1", "o2", "r1", "r2", "term"):
            assert call(**{name: None}) == -1, name
        assert call(n=-1) == -2 and call(n=8, stride=4) == -2   # PZ_E_SIZE
        assert call(o1=C.c_void_p(4100)) == -4 and call(o2=C.c_void_p(4104)) == -4  # PZ_E_ALIGN
        # every slab keeps the 16-byte alignment of the row stores: n % 4 == 0 when k > 1
        assert call(n=6, stride=8) == -4 and call(n=6, stride=8, hold=1) == -4
        for bad in (_native.PzFlightTables(None, 4104), _native.PzFlightTables(4098, 4096)):
            assert call(n=8, stride=8, tables=C.byref(bad)) == -4
        cfg.normalize_obs = 7
        assert call() == -3                                     # PZ_E_CONFIG
        for fmt in (2, 3, 4, 5, 6):                             # 2-byte rows: n % 8 == 0 when k > 1
            cfg.normalize_obs = fmt
            assert call(n=12, stride=16) == -4 and call() == 0
        cfg.normalize_obs = 1
        assert call(n=12, stride=16, state=None) == -1
        cfg.normalize_obs, cfg.packed_state = 0, 1
        assert call() == 0 and call(state=C.c_void_p(4100)) == -4  # a packed state is 16-byte aligned
        cfg.packed_state = 2
        assert call() == -3
    cfg.action_format = cfg.normalize_obs = cfg.packed_state = 0
    assert many(tape=None) == -1                                # the tape is required ...
    assert roll(tape=None) == 0 and roll(tape=fake) == 0        # ... the rollout's action output is not
    for fmt in (1, 2, 3):                                       # the tape is int32 alone
        cfg.action_format = fmt
        assert many() == -3
    cfg.action_format = 4
    assert many() == -3 and roll() == -3


def test_the_code_object_holds_exactly_the_reachable_held_trajectory_kernels(built_lib):
    sys.path.insert(0, str(REPO / "tools"))
    import kernel_digest
    import kernel_matrix
    import kernel_notes

    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    shipped = {name.replace("pz::", "", 1) for name in kernel_digest.kernels(built_lib)}
    want = held_traj_kernels()
    assert len(want) == 32
    assert {k for k in shipped if k.startswith("held_traj_kernel<")} == want
    # the pinned families and pz_step_held's gained and lost none
    assert {k for k in shipped if k.startswith(kernel_matrix.FAMILIES)} == kernel_matrix.KERNELS
    assert len(kernel_matrix.KERNELS) == 137
    tf = ("false", "true")
    assert {k for k in shipped if k.startswith("hold_kernel<")} == {f"hold_kernel<{a}, {b}, {p}>" for a in tf for b in tf
                                                                    for p in tf}
    # the standing code-object rules: no scratch, no VGPR spill
    notes = {name.split("(")[0].replace("void pz::", ""): r for name, r in kernel_notes.notes(Path(built_lib))}
    for k in want:
        assert notes[k][".private_segment_fixed_size"] == 0 and notes[k][".vgpr_spill_count"] == 0, (k, notes[k])


def test_env_source_threads_the_held_trajectories_through_the_api():
    """What can be said without a device: the two methods exist with their siblings' signatures and bind the new calls."""
    from pikazoo_amd import env as E

    for held, plain in (("step_many_held", "step_many"), ("rollout_random_held", "rollout_random")):
        assert inspect.signature(getattr(E.raw_env, held)) == inspect.signature(getattr(E.raw_env, plain))
    src = inspect.getsource(E.raw_env)
    assert "pz_step_many_held" in src and "pz_rollout_random_held" in src
    assert not hasattr(E.raw_env, "step_random_held")


@pytest.mark.parametrize("case", BITING, ids=lambda c: c.id)
def test_the_biting_cases_bite_on_the_judge_alone(oracle, case):
    """Every GPU case with hold > 1 and k >= 16 asserts that games ended inside a repeat, on a repeat's last frame and
    (auto_reset) were running again one slab later; here the same counts on the CPU judge, without a device."""
    judge = make_judge(oracle, case)
    assert isinstance(judge, HeldOracle)
    terms = [judge.step(*policy(oracle, case, t))[2].copy() for t in range(case.k)]
    inside, last, revived, twice = judge_counts(judge, np.stack(terms))
    assert inside > 0 and last > 0
    if case.auto_reset:
        assert revived > 0
    if case.ends_twice:
        assert twice > 0
