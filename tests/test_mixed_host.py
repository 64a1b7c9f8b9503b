"""Per-game computer players (pz_step_mixed) without a GPU: the export and its declaration, the family's census in the
code object -- exactly two instantiations, outside pz::, no scratch, no VGPR spill --, argument validation, what the GPU
cases of tests/mixed_judge.py cover, and, on the judge alone, that those cases bite."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import mixed_judge as mj

REPO = Path(__file__).resolve().parent.parent
KERNELS = {"pz_mixed::step_mixed_kernel<false>", "pz_mixed::step_mixed_kernel<true>"}


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    sys.path.insert(0, str(REPO / "tools"))
    import build as pz_build

    return pz_build.build()


def test_symbol_is_exported_declared_and_bound(built_lib):
    from pikazoo_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+pz_step_mixed\s*\(([^;]*)\)\s*;", header)
    assert decl, "pz_step_mixed is not declared in include/pikazoo_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 15 and params[4] == "const uint8_t *computer_mask"
    exported = subprocess.run(["nm", "-D", "--defined-only", str(built_lib)], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T pz_step_mixed$", exported, flags=re.M), "pz_step_mixed is not exported"
    assert "pz_step_mixed" in _native.exported_names()
    lib = _native.load()
    # additive: the ABI version and pz_config are the parent's
    assert lib.pz_abi_version() == _native.ABI_VERSION == 10
    assert lib.pz_config_bytes() == C.sizeof(_native.PzConfig) == 120
    assert len(lib.pz_step_mixed.argtypes) == len(lib.pz_step.argtypes) + 1
    assert "pz_step_mixed" in (REPO / "INTEGRATION.md").read_text()


def test_argument_validation_without_a_gpu(built_lib):
    from pikazoo_amd import _native

    lib = _native.load()
    cfg = _native.PzConfig()
    cfg.winning_score = 1
    fake = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    ok = (fake, fake, fake, fake, fake, fake, fake, fake)  # mask, actions, observations, rewards
    assert lib.pz_step_mixed(fake, 0, 0, C.byref(cfg), *ok, None, None, None) == 0       # empty batch: no launch
    assert lib.pz_step_mixed(fake, 0, 0, C.byref(cfg), None, *ok[1:], None, None, None) == -1   # NULL mask
    assert lib.pz_step_mixed(fake, 0, 0, C.byref(cfg), fake, None, *ok[2:], None, None, None) == -1
    assert lib.pz_step_mixed(None, 0, 0, C.byref(cfg), *ok, None, None, None) == -1
    assert lib.pz_step_mixed(fake, 8, 4, C.byref(cfg), *ok, None, None, None) == -2      # stride < n
    assert lib.pz_step_mixed(fake, 0, 0, C.byref(cfg), fake, fake, fake, C.c_void_p(4100), fake, fake, fake, fake, None,
                             None, None) == -4                                                 # observations: 16 bytes
    bad = _native.PzFlightTables(None, 4104)
    assert lib.pz_step_mixed(fake, 8, 8, C.byref(cfg), *ok, None, C.byref(bad), None) == -4
    cfg.action_format = 4
    assert lib.pz_step_mixed(fake, 0, 0, C.byref(cfg), *ok, None, None, None) == -3


def test_the_code_object_holds_exactly_the_two_instantiations_outside_pz(built_lib):
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    names = set(kernel_digest.kernels(built_lib))
    assert {n for n in names if "mixed" in n} == KERNELS
    assert not any(n.startswith("pz::") and "mixed" in n for n in names)
    rows = {name.split("(")[0].replace("void ", ""): r for name, r in kernel_notes.notes(Path(built_lib))}
    for k in KERNELS:
        r = rows[k]
        assert r[".private_segment_fixed_size"] == 0, f"{k} uses scratch memory"
        assert r[".vgpr_spill_count"] == 0, f"{k} spills VGPRs"
        assert r[".group_segment_fixed_size"] == 2 * 64 * 35 * 4  # the two staged observation tensors, nothing else


def test_the_gpu_cases_cover_the_family():
    cases = mj.cases()
    assert len({c.name for c in cases}) == len(cases) and 10 <= len(cases) <= 14
    plain = {(c.packed, c.tables) for c in cases if not (c.shaped or c.planted or c.obs_format or c.action_format != "i32"
                                                         or not c.auto_reset)}
    assert plain == {(p, t) for p in (False, True) for t in ("both", "power_hit", "none")}
    assert any(c.shaped and c.simplify_action and c.obs_format == 1 for c in cases)
    assert any(c.obs_format >= 2 for c in cases) and any(c.action_format == "i64" for c in cases)
    assert any(not c.auto_reset for c in cases) and any(c.planted for c in cases)
    # every action stream / start combination of the cases is one the non-vacuity probes below run
    assert {(c.simplify_action, c.planted) for c in cases} == {(p.simplify_action, p.planted) for p in PROBES.values()}
    codes = mj.role_codes()
    assert codes.shape == (mj.N,) and mj.N % 64 == 8 and mj.STRIDE > mj.N
    assert (codes[:64] == 0).all() and (codes[64:128] == 3).all()
    assert all(np.array_equal(np.bincount(codes[128:192], minlength=4), [16] * 4) for _ in (0,))
    assert np.array_equal(codes[128:136], [0, 1, 2, 3, 0, 1, 2, 3])
    for c in mj.CODES:  # every role code decides whole games, and the tail is not one code
        assert (codes == c).sum() >= 16
    assert len(set(codes[192:])) > 1


def _run(oracle, case, frames=mj.FRAMES):
    judge = mj.judge_for(oracle, case)
    n_act = 13 if case.simplify_action else 18
    for t in range(frames):
        judge.step(*mj.actions(oracle, t, n_act))
    return judge


# the three action / start combinations of the GPU cases: 18 actions from the constructor's state and from planted
# states, and the 13 actions of SimplifyAction (the wrapper-stack cases)
PROBES = {"constructed": mj.Case("probe"), "planted": mj.Case("probe", planted=True),
          "simplified-actions": mj.Case("probe", simplify_action=True)}


@pytest.mark.parametrize("probe", list(PROBES))
def test_every_lane_depends_on_its_role_code(oracle, probe):
    """Non-vacuity, on the judge alone: after the GPU cases' frames every lane's state under its own roles differs from
    its state under each of the three other role codes -- a kernel that misreads any lane's code is caught at the end."""
    judge = _run(oracle, PROBES[probe])
    mine = judge.state
    for other in mj.CODES:
        lanes = judge.codes != other
        same = (mine == judge.state_under(other)).all(axis=0) & lanes
        assert not same.any(), (other, np.flatnonzero(same))


def test_a_lane_without_a_computer_keeps_its_landing_point_word(oracle):
    """On the judge alone: some code-0 lane carries, at the end of a frame, a landing-point word that every
    computer-role run overwrote in that frame from the same state."""
    case = mj.Case("probe", planted=True)
    judge = mj.judge_for(oracle, case)
    start = judge.state
    judge.step(*mj.actions(oracle, 0, 18))
    zero = judge.codes == 0
    kept = zero & (judge.state[mj.EX_WORD] == start[mj.EX_WORD]) & (start[41] == 0)
    for code in (1, 2, 3):
        kept &= judge.state_under(code)[mj.EX_WORD] != start[mj.EX_WORD]
    assert kept.sum() >= 8, kept.sum()


def test_a_role_change_continues_from_the_lanes_own_state(oracle):
    """The judge's role change: a lane that moves to another run takes its state along, and from then on differs from
    the lane that never changed."""
    case = mj.Case("probe")
    judge, stay = mj.judge_for(oracle, case), mj.judge_for(oracle, case)
    for t in range(50):
        a = mj.actions(oracle, t, 18)
        judge.step(*a)
        stay.step(*a)
    assert np.array_equal(judge.state, stay.state)
    before = judge.state
    flipped = (judge.codes ^ 3).astype(np.uint8)
    judge.set_codes(flipped)
    assert np.array_equal(judge.state, before)
    for t in range(50, 120):
        a = mj.actions(oracle, t, 18)
        judge.step(*a)
        stay.step(*a)
    assert not (judge.state == stay.state).all(axis=0).any()
