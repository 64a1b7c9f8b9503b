"""CPU tests of frame skip (``pz_step_held``, ``frame_skip=``): the C ABI without a device, the code object, and the
judge of tests/test_gpu_frame_skip.py (tests/frame_skip_judge.py) against the reference itself."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from frame_skip_judge import HeldOracle

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build as pz_build

    return pz_build.build()


def test_pz_step_held_is_declared_bound_and_exported(built_lib):
    from pikazoo_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int pz_step_held\((.*?)\);", header, flags=re.S)
    assert decl, "pz_step_held is not declared in include/pikazoo_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 16 and params[6] == "int32_t k" and params[13] == "int64_t *episodes_done"
    assert "pz_step_held" in _native.exported_names()
    assert len(_native._SIGNATURES["pz_step_held"][1]) == 16 and _native._SIGNATURES["pz_step_held"][1][6] is C.c_int32
    assert hasattr(C.CDLL(str(built_lib)), "pz_step_held")
    lib = _native.load()
    assert lib.pz_abi_version() == 10 and lib.pz_config_bytes() == 120  # additive: same ABI, same configuration block


def test_pz_step_held_validates_its_arguments_without_a_gpu(built_lib):
    """Argument errors are reported before anything touches the device (no launch on these paths)."""
    from pikazoo_amd import _native

    lib = _native.load()
    cfg = _native.PzConfig()
    cfg.winning_score, cfg.serve_mode = 15, 0
    fake = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    ref = C.byref(cfg)

    def held(state=fake, n=0, stride=0, a1=fake, a2=fake, k=4, o1=fake, o2=fake, r1=fake, r2=fake, term=fake, tables=None):
        return lib.pz_step_held(state, n, stride, ref, a1, a2, k, o1, o2, r1, r2, term, None, None, tables, None)

    assert held() == 0                                   # empty batch: no-op
    assert held(k=1) == 0
    assert held(k=0) == -3 and held(k=-2) == -3          # PZ_E_CONFIG: at least one frame
    assert held(state=None) == -1                        # PZ_E_NULL
    for name in ("a1", "a2", "o1", "o2", "r1", "r2", "term"):
        assert held(**{name: None}) == -1, name
    assert held(n=-1) == -2 and held(n=8, stride=4) == -2  # PZ_E_SIZE
    assert held(o1=C.c_void_p(4100)) == -4 and held(o2=C.c_void_p(4104)) == -4  # PZ_E_ALIGN
    for bad in (_native.PzFlightTables(None, 4104), _native.PzFlightTables(4098, 4096)):
        assert held(n=8, stride=8, tables=C.byref(bad)) == -4
    cfg.action_format = 4
    assert held() == -3
    cfg.action_format, cfg.normalize_obs = 3, 7
    assert held() == -3
    cfg.normalize_obs, cfg.packed_state = 6, 1
    assert held() == 0 and held(state=C.c_void_p(4100)) == -4  # a packed state is 16-byte aligned


def test_the_hold_kernels_are_in_the_code_object_and_the_pinned_families_gained_none(built_lib):
    sys.path.insert(0, str(REPO / "tools"))
    import kernel_digest
    import kernel_matrix
    import kernel_notes

    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    shipped = {name.replace("pz::", "", 1) for name in kernel_digest.kernels(built_lib)}
    tf = ("false", "true")
    want = {f"hold_kernel<{a}, {b}, {p}>" for a in tf for b in tf for p in tf}
    assert {k for k in shipped if k.startswith("hold_kernel<")} == want
    assert {k for k in shipped if k.startswith(kernel_matrix.FAMILIES)} == kernel_matrix.KERNELS
    assert len(kernel_matrix.KERNELS) == 137
    # the standing code-object rules: no scratch, no VGPR spill
    notes = {name.split("(")[0].replace("void pz::", ""): r for name, r in kernel_notes.notes(Path(built_lib))}
    for k in want:
        assert notes[k][".private_segment_fixed_size"] == 0 and notes[k][".vgpr_spill_count"] == 0, (k, notes[k])


def test_env_source_threads_frame_skip_through_the_api():
    """What can be said without a device: the constructor argument, the binding call and the checkpoint key exist."""
    import inspect

    from pikazoo_amd import env as E

    sig = inspect.signature(E.raw_env.__init__)
    assert sig.parameters["frame_skip"].default == 1 and sig.parameters["frame_skip"].kind is inspect.Parameter.KEYWORD_ONLY
    src = inspect.getsource(E.raw_env)
    assert "pz_step_held" in src and 'd["frame_skip"]' in src


def test_the_judge_reproduces_the_reference_stepped_with_held_actions(oracle):
    """tests/golden/frame_skip_k4.npz (tests/capture_frame_skip.py): the unmodified reference, every action held for
    4 frames, a game's repeat cut at its terminal frame and the game reset before its next repeat -- what the judge's
    frozen frames and next-launch reset must amount to."""
    from conftest import GOLDEN

    d = dict(np.load(GOLDEN / "frame_skip_k4.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    assert meta["frame_skip"] == 4 and meta["ended_inside"] > 0 and meta["ended_last"] > 0
    kw = meta["env_kwargs"]
    cfg = oracle.make_config(winning_score=kw["winning_score"], is_player2_computer=kw["is_player2_computer"],
                             seed=meta["seed"], env_id_base=meta["env_id_base"], auto_reset=True)
    judge = HeldOracle(oracle, meta["lanes"], meta["frame_skip"], cfg, nthreads=1)
    judge.reset()
    assert np.array_equal(judge.state, d["state0"])
    for t in range(meta["steps"]):
        a = d["actions"][t].astype(np.int32)
        obs, rew, term = judge.step(a[0], a[1])
        st = d["states"][t].astype(np.int32)
        st[43] = d["rng_counter"][t]
        assert np.array_equal(judge.state, st), t
        assert np.array_equal(obs[0], d["obs"][t, 0]) and np.array_equal(obs[1], d["obs"][t, 1]), t
        assert np.array_equal(rew[0], d["rew"][t, 0]) and np.array_equal(rew[1], d["rew"][t, 1]), t
        assert np.array_equal(term, d["term"][t]), t
    assert (judge.ended_inside, judge.ended_last) == (meta["ended_inside"], meta["ended_last"])
