"""CPU tests (no GPU needed) of the V-trace library and of the judge its GPU tests compare with (tests/vtrace_judge.py).

The judge: ``judge32`` against exact rational arithmetic on dyadic inputs with planted weights; against ``judge64`` within the
derived tolerance, with the share of it that an honest float32 run uses recorded; on-policy equal to ``gae_judge.judge`` BIT
FOR BIT on all its flag patterns; off-policy different from GAE on every element; nothing crossing an episode end; a NaN
log-prob staying in its episode; every mutant caught by the GPU test's own cases.  The library: exports, build id, the new
build tuple, no shared symbol, lazy loading, the INTEGRATION entry, the kernel census, every return code that needs no launch
in the header's order, and the ``ValueError``s that need no device."""
import re
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import gae_judge as GJ
import vtrace_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_vtrace", "pz_vtrace_abi_version", "pz_vtrace_build_id"]
FAKE = 4096


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.vtrace, the judge's included: none of them runs without the module"""
    from pikazoo_amd import vtrace

    return vtrace


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import vtrace

    return vtrace.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the judge -------------------------------------------------------------------------------------------------------------------
def test_judge32_is_exact_on_dyadic_inputs_with_planted_weights():
    """integer rewards, values in quarters, gamma = lam = 1/2, weights and clips powers of two, k <= 6: every intermediate is a
    dyadic rational of few bits, float32 commits no rounding, and judge32 must equal exact rational arithmetic"""
    rng = np.random.default_rng(5)
    clips = (1.0, 0.5, 2.0)
    for k in (1, 2, 4, 6):
        n = 97
        r = rng.integers(-3, 4, size=(k, n)).astype(np.int32)
        v = (rng.integers(-40, 41, size=(k + 1, n)) / 4).astype(np.float32)
        d = GJ.flags("random50" if k > 2 else "random10", k, n, rng)
        w = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0, 8.0], np.float32), size=(k, n))
        lp = np.zeros((k, n), np.float32)
        for rew in (r, r.astype(np.float32)):
            pg, vs = J.judge32(rew, d, v, lp, lp, 0.5, 0.5, clips, w=w)
            fp, fv = J.judge_fraction(rew, d, v, w, 0.5, 0.5, clips)
            for t in range(k):
                assert [Fraction(float(x)) for x in pg[t]] == fp[t]
                assert [Fraction(float(x)) for x in vs[t]] == fv[t]
    # the three plants of the exact cases give exactly 1, 0 and a weight far beyond any clip of the cases
    lpb = np.array([-0.5, -1.25, -3.0], np.float32)
    w = J.weights(lpb, np.array([-0.5, -np.inf, np.float32(-3.0) + np.float32(8)], np.float32))
    assert w[0] == 1 and w[1] == 0 and 2900 < w[2] < 3000 and w[2] / 4 > 700


@pytest.mark.parametrize("s", J.TOLERANCE, ids=lambda s: f"k{s['k']}-{s['rf']}-{s['vf']}")
def test_judge32_is_within_the_derived_tolerance_of_judge64_and_the_mutants_are_not(s):
    """the float32 restatement (numpy's exp) uses a part of the tolerance -- recorded here, it must stay below 1 -- and every
    mutant that shows on random log-ratios misses it by far: the tolerance is neither too tight for honest float32 nor blind"""
    c = J.case_of(s, "random")
    for side in range(2):
        args = (c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side])
        pg64, vs64, tol_pg, tol_vs = J.judge64(*args)
        pg, vs = J.judge32(*args)
        used = max(J.worst_share(pg, pg64, tol_pg), J.worst_share(vs, vs64, tol_vs))
        print(f"k={s['k']} {s['rf']}/{s['vf']} side {side}: judge32 uses {used:.3f} of the tolerance; the largest tolerance "
              f"{max(tol_pg.max(), tol_vs.max()):.3g}, the largest |vs| {np.abs(vs64).max():.3g}")
        assert 0 < used < 1
        assert max(tol_pg.max(), tol_vs.max()) < 2e-3 * max(1.0, np.abs(vs64).max())     # (and it is a float32 tolerance, not a loose one)
        for m in J.MUTANTS[:5]:
            if s["k"] == 1 and m in ("trace_without_c", "pg_adv_from_v_only", "trace_mask_dropped"):
                continue                                  # (one row has no trace)
            mp, mv = J.judge32(*args, mutant=m)
            assert max(J.worst_share(mp, pg64, tol_pg), J.worst_share(mv, vs64, tol_vs)) > 100, m


def test_on_policy_judge32_is_gaes_judge_bit_for_bit():
    """target = behaviour (the same bits) and all three clips >= 1: vs is GAE's ret and pg_adv its adv, on every pattern of
    gae_judge.FLAG_PATTERNS, k in {1, 7, 8, 33, 130}, both reward dtypes, lam in {0, 0.95, 1}"""
    compared = 0
    for pattern in GJ.FLAG_PATTERNS:
        for k in (1, 7, 8, 33, 130):
            for rf, vf in (("int32", "float32"), ("float32", "bfloat16")):
                c = J.make_case(k, 65, pattern, rf, vf, seed=3, kind="on_policy")
                for lam in (0.0, 0.95, 1.0):
                    for clips in ((1.0, 1.0, 1.0), (1.0, 2.5, 4.0)):
                        for side in range(2):
                            adv, ret = GJ.judge(c["rew"][side], c["d"], c["val"][side], 0.99, lam)
                            pg, vs = J.judge32(c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side], 0.99, lam, clips)
                            assert np.array_equal(bits(pg), bits(adv)) and np.array_equal(bits(vs), bits(ret)), (pattern, k, rf, lam, clips)
                            compared += adv.size
    assert compared >= 100000
    # a clip below 1 breaks it, as it must
    c = J.make_case(8, 65, "random10", seed=3, kind="on_policy")
    adv, ret = GJ.judge(c["rew"][0], c["d"], c["val"][0], 0.99, 0.95)
    pg, vs = J.judge32(c["rew"][0], c["d"], c["val"][0], c["lpb"][0], c["lpt"][0], 0.99, 0.95, (0.5, 1.0, 1.0))
    assert not np.array_equal(bits(vs), bits(ret))


def test_off_policy_differs_from_gae_on_every_element():
    c = J.make_case(33, 200, "random10", seed=4, kind="random")
    for side in range(2):
        adv, ret = GJ.judge(c["rew"][side], c["d"], c["val"][side], J.GAMMA, J.LAM)
        pg, vs = J.judge32(c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side])
        assert (bits(pg) != bits(adv)).all() and (bits(vs) != bits(ret)).all()


def test_nothing_crosses_an_episode_end():
    """NaN, inf and 1e30 planted behind a flagged row -- in the values, the rewards' successors and the log-probs -- leave the rows
    in front of the flag at the bits they have without the plants"""
    c = J.make_case(9, 65, "none", seed=8)
    c["d"][4] = 1
    clean = [J.judge32(c["rew"][s], c["d"], c["val"][s], c["lpb"][s], c["lpt"][s]) for s in range(2)]
    for s in range(2):
        v, lpb, lpt = c["val"][s].copy(), c["lpb"][s].copy(), c["lpt"][s].copy()
        v[5, ::3], v[5, 1::3], v[5, 2::3] = np.nan, np.inf, 1e30
        v[6:] = 1e30
        lpt[5:, ::2], lpb[5:, 1::2] = np.nan, -1e30
        pg, vs = J.judge32(c["rew"][s], c["d"], v, lpb, lpt)
        assert np.array_equal(bits(pg[:5]), bits(clean[s][0][:5])) and np.array_equal(bits(vs[:5]), bits(clean[s][1][:5]))
        with np.errstate(invalid="ignore"):
            assert np.isfinite(pg[:5]).all() and (~np.isfinite(vs[5]) | (np.abs(vs[5]) > 1e20)).all()     # (the plants did reach row 5)


def test_a_nan_log_prob_surfaces_as_nan_in_its_own_episode_only():
    c, nan_rows = J.nan_case()
    for s in range(2):
        pg, vs = J.judge32(c["rew"][s], c["d"], c["val"][s], c["lpb"][s], c["lpt"][s])
        for t in range(9):
            assert np.isnan(vs[t]).all() == (t in nan_rows) and np.isnan(pg[t]).all() == (t in nan_rows), t
            assert np.isnan(vs[t]).any() == (t in nan_rows) and np.isnan(pg[t]).any() == (t in nan_rows), t
        # the mutant that writes the clip as a minimum hides it
        mp, mv = J.judge32(c["rew"][s], c["d"], c["val"][s], c["lpb"][s], c["lpt"][s], mutant="nan_weight_becomes_clip")
        assert np.isfinite(mv).all() and np.isfinite(mp).all()


def outputs(c, s, mutant=None):
    sides = 2 if s["both"] else 1
    return [J.judge32(c["rew"][i], c["d"], c["val"][i], c["lpb"][i], c["lpt"][i], s["gamma"], s["lam"], s["clips"], mutant=mutant) for i in range(sides)]


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


@pytest.mark.parametrize("mutant", J.MUTANTS)
def test_every_mutant_is_caught_by_the_gpu_tests_own_cases(mutant):
    """over the table of exact cases that tests/test_gpu_vtrace.py launches (and its NaN case): which tests tell the mutant from
    the judge by the bits they compare"""
    caught = {}
    for test, specs in J.EXACT.items():
        if test == "many_workgroups":
            continue                      # (the size is what that case is for)
        hits = 0
        for s in specs:
            c = J.case_of(s)
            hits += not same(outputs(c, s), outputs(c, s, mutant))
        caught[test] = (hits, len(specs))
    c, _ = J.nan_case()
    s = J.spec(9, 65)
    nan_hit = any(not np.array_equal(np.isnan(x), np.isnan(y)) for pa, pb in zip(outputs(c, s), outputs(c, s, mutant)) for x, y in zip(pa, pb))
    print(mutant, caught, "NaN case:", nan_hit)
    if mutant == "nan_weight_becomes_clip":
        assert nan_hit and not any(h for h, _ in caught.values())      # the exact plants hold no NaN: the NaN case is there for it
        return
    # every test of the table catches it in at least one of its cases, and most cases do
    assert all(h > 0 for h, _ in caught.values()), caught
    assert sum(h for h, _ in caught.values()) >= 0.6 * sum(n for _, n in caught.values()), caught
    assert caught["k_edges"][0] >= len(J.K_EDGES) - (1 if mutant in ("trace_without_c", "pg_adv_from_v_only", "trace_mask_dropped") else 0)


def test_the_case_table_holds_what_the_kernel_can_get_wrong():
    assert J.K_EDGES == GJ.K_EDGES and J.N_EDGES == GJ.N_EDGES and GJ.CHUNK == 8
    csrc = REPO / "pika-zoo_amd" / "csrc"
    source = (csrc / "pz_traj_scan.hpp").read_text()
    assert re.findall(r"^constexpr int kChunk = (\d+);", source, re.M) == ["8"], "the chunk moved: K_EDGES are the edges of 8"
    for unit in ("pz_learn.hip", "pz_vtrace.hip"):        # both kernels scan by that one definition: neither has a chunk of its own
        text = (csrc / unit).read_text()
        assert '#include "pz_traj_scan.hpp"' in text and not re.search(r"\bkChunk\s*=", text), unit
    assert {s["k"] for s in J.EXACT["k_edges"]} == set(GJ.K_EDGES) and {s["n"] for s in J.EXACT["n_edges"]} == set(GJ.N_EDGES)
    assert {s["pattern"] for s in J.EXACT["flag_patterns"]} == set(GJ.FLAG_PATTERNS)
    assert {(s["rf"], s["vf"]) for s in J.EXACT["formats"]} == {(r, v) for r in GJ.REWARD_DTYPES for v in GJ.VALUE_DTYPES}
    assert all(len(set(s["pitches"])) == 5 and min(s["pitches"]) > s["n"] for s in J.EXACT["five_pitches"])
    assert all(set(s["pitches"]) == {s["n"]} for s in J.EXACT["pitch_is_n"])
    assert {(s["gamma"], s["lam"]) for s in J.EXACT["gamma_lam_ends"]} >= {(0.99, 1.0), (0.99, 0.0), (0.0, 0.95), (1.0, 1.0)}
    ends = [s["clips"] for s in J.EXACT["clip_ends"]]
    assert all(any(cl[i] == x for cl in ends) for i in range(3) for x in (0.0, 4.0))
    assert len(set(J.CLIPS)) == 3 and max(J.CLIPS) <= 4 and all(max(cl) <= 4 for cl in ends)
    for s in J.EXACT["k_edges"][3:] + J.EXACT["formats"]:
        c = J.case_of(s)
        for lpb, lpt in zip(c["lpb"], c["lpt"]):
            kinds = [(lpt.view(np.uint32) == lpb.view(np.uint32)), np.isneginf(lpt), lpt > lpb + 7]
            assert (sum(kinds) == 1).all() and all(0.2 < kind.mean() < 0.5 for kind in kinds)
            w = J.weights(lpb, lpt)
            assert set(np.unique(w[~kinds[2]]).tolist()) == {0.0, 1.0} and (w[kinds[2]] > 2000).all()


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_vtrace_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, vtrace

    assert header_functions("pikazoo_vtrace.h") == NAMES == sorted(vtrace.SIGNATURES) == dynamic_pz_symbols(pz_build.VTRACE_LIB)
    assert pz_build.library_id(pz_build.VTRACE_LIB) == pz_build.source_id() == lib.pz_vtrace_build_id().decode()
    assert not pz_build.needs_build()
    # the fifteenth library, through a tuple of its own: the three older tuples are what they were
    assert len(pz_build.TARGETS) == 11 and len(pz_build.ALL_TARGETS) == 13 and len(pz_build.BUILD_TARGETS) == 14
    assert len(pz_build.LIBRARY_TARGETS) == 15 and pz_build.LIBRARY_TARGETS[:14] == pz_build.BUILD_TARGETS
    assert pz_build.LIBRARY_TARGETS[14] == (pz_build.VTRACE_LIB, pz_build.VTRACE_SOURCES)
    assert pz_build.VTRACE_LIB.name == "libpikazoo_vtrace.so" and pz_build.VTRACE_SOURCES == [pz_build.CSRC / "pz_vtrace.hip"]
    assert pz_build.VTRACE_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_vtrace.h") in pz_build.DEPS
    assert (pz_build.CSRC / "pz_traj_scan.hpp") in pz_build.DEPS
    for lib_path, _ in pz_build.LIBRARY_TARGETS:
        assert pz_build.library_id(lib_path) == pz_build.source_id(), lib_path
    assert lib.pz_vtrace_abi_version() == vtrace.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_vtrace.h").read_text()
    assert "#define PZ_VTRACE_ABI_VERSION 1" in header
    for other, _ in pz_build.BUILD_TARGETS:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_vtrace.h" in doc and "libpikazoo_vtrace.so" in doc and "pz_vtrace" in doc
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"int pz_vtrace\((.*?)\);", bare, flags=re.S).group(1)
    args = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert len(args) == 28 == len(vtrace.SIGNATURES["pz_vtrace"][1])
    shown = re.search(r"int pz_vtrace\((.*?)\);", doc, flags=re.S)
    assert shown and [a.split()[-1].lstrip("*") for a in shown.group(1).replace("\n", " ").split(",")] == args


def test_importing_the_older_modules_does_not_load_the_vtrace_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, wrappers, learn, policy, ppo, net, netgrad, optim, batch, pool, league, act, pool_act, ego; "
            "assert 'pikazoo_amd.vtrace' not in sys.modules; "
            "import pikazoo_amd as p; assert 'vtrace' in p.__all__; "
            "p.vtrace.targets; assert 'pikazoo_amd.vtrace' in sys.modules and p.vtrace._lib is None; "
            "assert not any('libpikazoo_vtrace' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_vtrace_library(pz_build):
    """2 reward formats x 3 value formats = 6 kernels, one family, and nothing else in the code object; none uses scratch, spills
    a register or holds LDS, and each stays within 128 VGPRs (4 waves per SIMD)"""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    want = sorted(f"pz_vt::vtrace_kernel<{rf}, {vf}>" for rf in (0, 1) for vf in (0, 1, 2))
    table = kernel_digest.kernels(pz_build.VTRACE_LIB)
    kernels = sorted(name for name in table if not name.endswith(".kd"))
    assert kernels == want, kernels
    assert all(count > 100 for name, (_, count) in table.items() if name in want)
    notes = kernel_notes.notes(pz_build.VTRACE_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == want
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0 and row[".vgpr_count"] <= 128, (name, row)
        print(name.split("(")[0], {k: row[k] for k in (".vgpr_count", ".sgpr_count")})


def call(lib, **over):
    """pz_vtrace on fake pointers (every check runs before the launch), both agents, k = 4, n = 8, pitch 8"""
    a = dict(rew_p1=FAKE, rew_p2=FAKE, reward_format=0, terminated=FAKE, val_p1=FAKE, val_p2=FAKE, value_format=0, lpb_p1=FAKE, lpb_p2=FAKE,
             lpt_p1=FAKE, lpt_p2=FAKE, k=4, n=8, rew_pitch=8, term_pitch=8, val_pitch=8, lp_pitch=8, out_pitch=8, gamma=0.99, lam=0.95,
             clip_rho=1.0, clip_c=1.0, clip_pg_rho=1.0, vs_p1=FAKE, vs_p2=FAKE, pg_p1=FAKE, pg_p2=FAKE, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.pz_vtrace(*a.values())


SECOND = ("rew_p2", "val_p2", "lpb_p2", "lpt_p2", "vs_p2", "pg_p2")
PITCHES = ("rew_pitch", "term_pitch", "val_pitch", "lp_pitch", "out_pitch")


def test_argument_validation(lib):
    # NULL: any pointer of agent 1 or the flags; agent 2 is all six or none
    for name in ("rew_p1", "terminated", "val_p1", "lpb_p1", "lpt_p1", "vs_p1", "pg_p1"):
        assert call(lib, **{name: None}) == -1, name
    for name in SECOND:
        assert call(lib, **{name: None}) == -1, name
        assert call(lib, **{other: None for other in SECOND if other != name}) == -1, name
    # sizes
    assert call(lib, k=0) == -2 and call(lib, k=-1) == -2 and call(lib, n=-1) == -2
    for name in PITCHES:
        assert call(lib, **{name: 7}) == -2, name
        assert call(lib, **{name: 1 << 61}) == -2, name                        # 5 rows of it: beyond int64 in bytes -- refused, never wrapped
        assert call(lib, **{name: ((2 ** 63 - 1) // 4) // 5 + 1}) == -2, name  # the first pitch that is too large
    big = {name: 1 << 31 for name in PITCHES}
    assert call(lib, n=(1 << 30) + 1, **big) == -2
    assert call(lib, k=2 ** 31 - 1, **big) == -2
    # formats, the two factors, the three clips
    assert call(lib, reward_format=2) == -3 and call(lib, reward_format=-1) == -3
    assert call(lib, value_format=3) == -3 and call(lib, value_format=-1) == -3
    for name in ("gamma", "lam"):
        for bad in (float("nan"), float("inf"), -float("inf"), -0.25, 1.0000001):
            assert call(lib, **{name: bad}) == -3, (name, bad)
    for name in ("clip_rho", "clip_c", "clip_pg_rho"):
        for bad in (float("nan"), float("inf"), -float("inf"), -0.25, -1e-30):
            assert call(lib, **{name: bad}) == -3, (name, bad)
        for good in (0.0, 1e-30, 1.0, 4.0, 3e38):
            assert call(lib, n=0, **{name: good}) == 0, (name, good)
    # alignment to the element: 4 bytes, 2 for the 16-bit value formats, none for the flags
    for name in ("rew_p1", "rew_p2", "val_p1", "val_p2", "lpb_p1", "lpb_p2", "lpt_p1", "lpt_p2", "vs_p1", "vs_p2", "pg_p1", "pg_p2"):
        assert call(lib, **{name: FAKE + 2}) == -4, name
        assert call(lib, value_format=1, **{name: FAKE + 1}) == -4, name
    assert call(lib, n=0, value_format=1, val_p1=FAKE + 2, val_p2=FAKE + 6, terminated=FAKE + 1) == 0
    # the order of the checks: NULL, size, config, alignment
    assert call(lib, rew_p1=None, k=0, clip_c=-1.0, vs_p1=FAKE + 1) == -1
    assert call(lib, k=0, clip_c=-1.0, vs_p1=FAKE + 1) == -2
    assert call(lib, clip_c=-1.0, vs_p1=FAKE + 1) == -3
    assert call(lib, n=0, vs_p1=FAKE + 1) == -4
    # n == 0: nothing to do, no launch (also on one side, on any format, at any legal scalar)
    assert call(lib, n=0) == 0 and call(lib, n=0, **{name: 0 for name in PITCHES}) == 0
    assert call(lib, n=0, reward_format=1, value_format=2, gamma=0.0, lam=1.0, clip_rho=0.0, **{name: None for name in SECOND}) == 0


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """on CPU tensors the device check is the last one standing, so everything in front of it is reachable here; the rest of
    the ``ValueError``s are the GPU test's"""
    import torch

    from pikazoo_amd import vtrace

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(vtrace, "load", refuse)
    r, v, d, lp = torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(4, 8, dtype=torch.bool), torch.zeros(4, 8)
    with pytest.raises(ValueError, match="GPU"):
        vtrace.targets(r, v, d, lp, lp)
    for bad in (lambda: vtrace.targets({"player_1": r}, {"player_2": v}, d, {"player_1": lp}, {"player_1": lp}),
                lambda: vtrace.targets({"player_1": r}, {"player_1": v}, d, {"player_2": lp}, {"player_1": lp}),
                lambda: vtrace.targets({"player_1": r}, {"player_1": v}, d, {"player_1": lp}, lp),
                lambda: vtrace.targets({"player_1": r, "player_2": r}, {"player_1": v, "player_2": v}, d, {"player_1": lp, "player_2": lp},
                                       {"player_2": lp, "player_1": lp})):
        with pytest.raises(ValueError, match="same agents"):
            bad()
    with pytest.raises(ValueError, match="k, N"):
        vtrace.targets(torch.zeros(4), v, d, lp, lp)
    with pytest.raises(ValueError, match="one or two"):
        vtrace.targets({}, {}, d, {}, {})
    with pytest.raises(ValueError, match="tensor"):
        vtrace.targets(r, v, d, lp, [1.0])
    with pytest.raises(ValueError, match="share one tensor"):
        vtrace.targets(r, v, {"player_1": d, "player_2": d.clone()}, lp, lp)
