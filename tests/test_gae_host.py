"""CPU tests (no GPU needed) of the GAE library: libpikazoo_learn.so exports its header's symbols and carries the tree's
build id, its code object holds exactly the ``pz_learn::gae_kernel`` family without scratch, spills or a fused
multiply-add, ``pz_gae`` refuses bad arguments before any launch, and the judge the GPU tests compare with
(tests/gae_judge.py) is the definition: exact on dyadic inputs, within a derived bound of the float64 formula, and
sharp enough that three mutants fail on its cases."""
import ctypes as C
import re
import shutil
import subprocess
import sys
import tempfile
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import gae_judge as J
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def learn_lib(pz_build):
    from pikazoo_amd import learn

    return learn.load()


def test_learn_library_exports_exactly_its_header(pz_build, learn_lib):
    from pikazoo_amd import _native, learn

    names = header_functions("pikazoo_learn.h")
    assert names == ["pz_gae", "pz_learn_abi_version", "pz_learn_build_id"]
    assert names == sorted(learn.SIGNATURES) == dynamic_pz_symbols(pz_build.LEARN_LIB)
    assert pz_build.library_id(pz_build.LEARN_LIB) == pz_build.source_id() == learn_lib.pz_learn_build_id().decode()
    assert not pz_build.needs_build()
    assert pz_build.LEARN_SOURCES[0] in pz_build.DEPS and (pz_build.CSRC / "pz_traj_scan.hpp") in pz_build.DEPS
    assert learn_lib.pz_learn_abi_version() == learn.ABI_VERSION == 1
    assert "#define PZ_LEARN_ABI_VERSION 1" in (REPO / "include" / "pikazoo_learn.h").read_text()
    # the product library did not move: its ABI, and none of the new names in it
    assert _native.load().pz_abi_version() == 10
    assert not set(names) & set(dynamic_pz_symbols(pz_build.LIB)) and not set(names) & set(_native.exported_names())
    # INTEGRATION.md shows the entry point as the header declares it (argument names in the header's order)
    doc = (REPO / "INTEGRATION.md").read_text()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_learn.h").read_text(), flags=re.S)
    decl = re.search(r"int pz_gae\((.*?)\);", header, flags=re.S).group(1)
    args = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert len(args) == 20 == len(learn.SIGNATURES["pz_gae"][1])
    shown = re.search(r"int pz_gae\((.*?)\);", doc, flags=re.S)
    assert shown, "INTEGRATION.md does not show pz_gae"
    assert [a.split()[-1].lstrip("*") for a in shown.group(1).replace("\n", " ").split(",")] == args
    assert "pikazoo_learn.h" in doc and "libpikazoo_learn.so" in doc


def test_importing_the_package_or_the_env_does_not_load_the_learn_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; from pikazoo_amd import env, pikazoo_v0; "
            "assert 'pikazoo_amd.learn' not in sys.modules; import pikazoo_amd as p; p.learn.gae; "
            "assert 'pikazoo_amd.learn' in sys.modules and p.learn._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_learn_library(pz_build):
    """The formats are COMPILE-TIME instantiations: 2 reward formats x 3 value formats = 6 kernels, one family, and
    nothing else in the code object.  None uses scratch, spills a register or touches LDS, and the family's disassembly
    holds no fused or chained float32 multiply-add (the translation unit switches contraction off)."""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    want = sorted(f"pz_learn::gae_kernel<{rf}, {vf}>" for rf in (0, 1) for vf in (0, 1, 2))
    table = kernel_digest.kernels(pz_build.LEARN_LIB)
    kernels = sorted(name for name in table if not name.endswith(".kd"))
    assert kernels == want, kernels
    assert all(count > 50 for name, (_, count) in table.items() if name in want)
    notes = kernel_notes.notes(pz_build.LEARN_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == want
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0 and row[".vgpr_count"] <= 128, (name, row)
    with tempfile.TemporaryDirectory() as t:
        copy = shutil.copy(pz_build.LEARN_LIB, Path(t) / "lib.so")
        subprocess.run([str(kernel_digest.LLVM / "llvm-objdump"), "--offloading", str(copy)], check=True, cwd=t, capture_output=True)
        obj = sorted(Path(t).glob("*gfx950*"))[0]
        asm = subprocess.run([str(kernel_digest.LLVM / "llvm-objdump"), "-d", str(obj)], check=True, capture_output=True,
                             text=True).stdout
    mnemonics = re.findall(r"^\s+([a-z][a-z_0-9]+) ", asm, flags=re.M)
    assert mnemonics.count("v_mul_f32_e32") + mnemonics.count("v_mul_f32_e64") >= 6 * 2  # (it is the arithmetic's code)
    fused = [m for m in mnemonics if re.match(r"v_(pk_)?(fma|fmac|mad|mac)\w*_f(32|16)|v_mad_\w*f32|v_fma_mix", m)]
    assert not fused, sorted(set(fused))
    assert "nt" in re.findall(r"global_store_dword .* (nt)\b", asm)  # the stores are non-temporal


FAKE = 4096


def call(lib, **over):
    """pz_gae on fake pointers (every check runs before the launch), both agents, k = 4, n = 8, pitch 8"""
    a = dict(rew_p1=FAKE, rew_p2=FAKE, reward_format=0, terminated=FAKE, val_p1=FAKE, val_p2=FAKE, value_format=0, k=4, n=8,
             rew_pitch=8, term_pitch=8, val_pitch=8, out_pitch=8, gamma=0.99, lam=0.95, adv_p1=FAKE, adv_p2=FAKE, ret_p1=FAKE,
             ret_p2=FAKE, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.pz_gae(*a.values())


def test_argument_validation(learn_lib):
    lib = learn_lib
    # NULL: any pointer of agent 1 or the flags; agent 2 is all four or none
    for name in ("rew_p1", "terminated", "val_p1", "adv_p1", "ret_p1"):
        assert call(lib, **{name: None}) == -1, name
    second = ("rew_p2", "val_p2", "adv_p2", "ret_p2")
    for name in second:
        assert call(lib, **{name: None}) == -1, name
        assert call(lib, **{other: None for other in second if other != name}) == -1, name
    # sizes
    assert call(lib, k=0) == -2 and call(lib, k=-1) == -2 and call(lib, n=-1) == -2
    for name in ("rew_pitch", "term_pitch", "val_pitch", "out_pitch"):
        assert call(lib, **{name: 7}) == -2, name
        assert call(lib, **{name: 1 << 61}) == -2, name  # 5 rows of it: beyond int64 in bytes -- refused, never wrapped
        assert call(lib, **{name: ((2 ** 63 - 1) // 4) // 5 + 1}) == -2, name  # the first pitch that is too large
    big = dict(rew_pitch=1 << 31, term_pitch=1 << 31, val_pitch=1 << 31, out_pitch=1 << 31)
    assert call(lib, n=(1 << 30) + 1, **big) == -2
    assert call(lib, k=2 ** 31 - 1, **{name: 1 << 31 for name in big}) == -2
    # formats and the two factors
    assert call(lib, reward_format=2) == -3 and call(lib, reward_format=-1) == -3
    assert call(lib, value_format=3) == -3 and call(lib, value_format=-1) == -3
    for name in ("gamma", "lam"):
        for bad in (float("nan"), float("inf"), -float("inf"), -0.25, 1.0000001):
            assert call(lib, **{name: bad}) == -3, (name, bad)
    # alignment to the element: 4 bytes, 2 for the 16-bit value formats, none for the flags
    for name in ("rew_p1", "rew_p2", "val_p1", "val_p2", "adv_p1", "adv_p2", "ret_p1", "ret_p2"):
        assert call(lib, **{name: FAKE + 2}) == -4, name
        assert call(lib, value_format=1, **{name: FAKE + 1}) == -4, name
    # the order of the checks: NULL, size, config, alignment
    assert call(lib, rew_p1=None, k=0, gamma=2.0, adv_p1=FAKE + 1) == -1
    assert call(lib, k=0, gamma=2.0, adv_p1=FAKE + 1) == -2
    assert call(lib, gamma=2.0, adv_p1=FAKE + 1) == -3
    # n == 0: nothing to do, no launch (also on one side, on any format, at any legal factor)
    assert call(lib, n=0) == 0 and call(lib, n=0, rew_pitch=0, term_pitch=0, val_pitch=0, out_pitch=0) == 0
    assert call(lib, n=0, rew_p2=None, val_p2=None, adv_p2=None, ret_p2=None, reward_format=1, value_format=2, gamma=0.0,
                lam=1.0, val_p1=FAKE + 2, terminated=FAKE + 1) == 0


def test_python_errors_come_before_any_launch():
    """shape, dtype, device and range errors of learn.gae raise ValueError -- on CPU tensors the device check is the last
    one standing, so everything before it is reachable here"""
    import torch

    from pikazoo_amd import learn

    r, v, d = torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(4, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="GPU"):
        learn.gae(r, v, d)
    with pytest.raises(ValueError, match="same agents"):
        learn.gae({"player_1": r}, {"player_2": v}, d)
    with pytest.raises(ValueError, match="same agents"):
        learn.gae({"player_1": r}, v, d)
    with pytest.raises(ValueError, match="k, N"):
        learn.gae(torch.zeros(4), v, d)
    with pytest.raises(ValueError, match="one or two"):
        learn.gae({}, {}, d)


# ---- the judge ------------------------------------------------------------------------------------------------------
def test_judge_is_exact_on_dyadic_inputs():
    """integer rewards, values in quarters, gamma = lam = 1/2, k <= 8: every intermediate is a dyadic rational of few bits,
    so float32 commits no rounding and the judge must equal exact rational arithmetic"""
    rng = np.random.default_rng(5)
    for k in (1, 2, 5, 8):
        n = 97
        r = rng.integers(-3, 4, size=(k, n)).astype(np.int32)
        v = (rng.integers(-40, 41, size=(k + 1, n)) / 4).astype(np.float32)
        d = J.flags("random50" if k > 2 else "random10", k, n, rng)
        for rew in (r, r.astype(np.float32)):
            adv, ret = J.judge(rew, d, v, 0.5, 0.5)
            fa, fr = J.judge_fraction(rew, d, v, 0.5, 0.5)
            for t in range(k):
                assert [Fraction(float(x)) for x in adv[t]] == fa[t]
                assert [Fraction(float(x)) for x in ret[t]] == fr[t]
    # a value behind an episode end never reaches the row in front of it: a select, not a multiply by zero
    v = np.array([[1.0], [np.inf], [np.nan]], np.float32)
    adv, ret = J.judge(np.array([[2], [3]], np.int32), np.array([[1], [1]], np.uint8), v, 0.5, 0.5)
    assert adv[0, 0] == 1.0 and ret[0, 0] == 2.0 and adv[1, 0] == -np.inf


@pytest.mark.parametrize("k", [1, 32, 128])
def test_judge_is_close_to_the_float64_formula(k):
    """|float32 - float64| <= 6 k 2^-24 M, M the largest magnitude of the float64 run: each row commits at most five
    roundings on the chain (gamma v, r + q, - v, gl a, the sum) and one more on the return, each at most 2^-24 of a
    magnitude <= M, and an error carried from row t + 1 is multiplied by gl <= 1"""
    c = J.make_case(k, 300, "random10", "float32", "float32", seed=k)
    for r, v in zip(c["rew"], c["val"]):
        adv, ret = J.judge(r, c["d"], v, 0.99, 0.95)
        a64, r64, most = J.judge_float64(r, c["d"], v, 0.99, 0.95)
        bound = 6 * k * 2.0 ** -24 * most
        err = max(np.abs(adv - a64).max(), np.abs(ret - r64).max())
        print(f"k={k}: error {err:.3g}, M {most:.3g}, bound {bound:.3g}")
        assert err <= bound


def bite_cases():
    return [(k, n, p, rf, vf) for k in J.K_EDGES for n in (1, 65) for p in J.FLAG_PATTERNS
            for rf, vf in (("int32", "float32"), ("float32", "bfloat16"))]


def test_every_mutant_differs_from_the_judge_on_every_case():
    """... that can tell it apart at all: dropping the mask changes nothing where no flag is set (pattern "none", or a
    random pattern that drew none on a tiny case), and reading another value row or swapping the factors changes nothing
    where every row is an episode end (pattern "all": neither v[t+1] nor gl is ever used) -- there the mutant must EQUAL
    the judge.  Everywhere else at least one output differs, for both agents."""
    told_apart = 0
    for k, n, p, rf, vf in bite_cases():
        c = J.make_case(k, n, p, rf, vf, seed=3)
        for r, v in zip(c["rew"], c["val"]):
            adv, ret = J.judge(r, c["d"], v, 0.99, 0.95)
            for m in J.MUTANTS:
                ma, mr = J.judge(r, c["d"], v, 0.99, 0.95, mutant=m)
                same = np.array_equal(ma.view(np.uint32), adv.view(np.uint32)) and np.array_equal(mr.view(np.uint32), ret.view(np.uint32))
                blind = not c["d"].any() if m == "mask_dropped" else bool(c["d"].all())
                assert same == blind, (k, n, p, rf, vf, m)
                told_apart += not same
    # (of the six patterns, "none" blinds one mutant and "all" two; the two random ones may blind one on a one-game case)
    assert told_apart >= 2 * len(bite_cases()) * 3 * 2 // 3


def test_env_recipe_has_episode_ends(oracle):
    """the recipe of the env tests in tests/test_gpu_gae.py, run on the CPU: most games end twice or more in its 128
    frames, some never, so the mask is exercised inside, at the end and not at all"""
    rc = J.RECIPE
    n = rc["n"]
    env = oracle.OracleEnv(n, oracle.make_config(winning_score=rc["winning_score"], seed=rc["seed"], env_id_base=rc["env_id_base"]))
    env.reset()
    term = np.zeros((rc["frames"], n), np.uint8)
    for t in range(rc["frames"]):
        a1, a2 = oracle.random_actions(n, rc["env_id_base"], rc["action_seed"], t)
        term[t] = env.step(a1, a2)[2]
    ends = term.astype(np.int64).sum(0)
    print(f"{int(ends.sum())} terminal frames, {int((ends >= 2).sum())} games with two or more, {int((ends == 0).sum())} with none, "
          f"first at frame {int(np.nonzero(term.any(1))[0][0])}, {int(term[-8:].sum())} in the last eight frames")
    assert (ends >= 2).sum() >= 200 and (ends == 0).sum() >= 1
    assert all(term[:, g:g + 64].any() for g in range(0, n, 64))
