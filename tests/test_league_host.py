"""CPU tests (no GPU needed) of the league library: the judge the GPU tests compare with (tests/league_judge.py) is the header's
draw and tally -- each equal to a second, scalar formulation on every case, the draw always below P, never a member of weight
0, the same in any sharding, another vector under another counter or seed, on a stream apart from the env's, the policy's and
the batch's, and distributed as its weights say -- and sharp enough that every mutant fails on the GPU tests' own cases;
``pfsp_weights`` is its numpy restatement; libpikazoo_league.so exports its header's four symbols and carries the tree's build
id, nothing loads it before its first use, its code object holds two kernels without scratch or spilled registers, the entry
points refuse bad arguments before any launch and in the documented order, and ``pikazoo_amd.league`` raises ``ValueError``
for malformed arguments before it needs the library.

No call here ever passes every check with games to run: a call that did would launch a kernel on fake pointers wherever a GPU
is present.  A check is shown to PASS by planting a failure of a later one."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import batch_judge as BJ
import league_judge as LJ
from test_cabi_and_host import dynamic_pz_symbols, header_functions
from test_net_host import declared_arguments

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_league_abi_version", "pz_league_build_id", "pz_league_draw", "pz_league_tally"]
KERNELS = ["pz_league::draw_kernel", "pz_league::tally_kernel"]


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.league, the judge's included: none of them runs without the module"""
    from pikazoo_amd import league

    return league


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import league

    return league.load()


def draw_of(case, mutant=None, scalar=False):
    weights = LJ.make_weights(case["weights"], case["P"])
    mask = LJ.make_mask(case["mask"], case["n"])
    if scalar:
        return LJ.draw_scalar(weights, case["n"], case["seed"], case["C"], case["first_game"], mask)
    return LJ.draw(weights, case["n"], case["seed"], case["C"], case["first_game"], mask, mutant=mutant)


# ---- the judge: the draw ------------------------------------------------------------------------------------------------------
def test_the_two_formulations_of_the_draw_agree_and_have_the_headers_properties():
    seen = set()
    for case in LJ.all_draw_cases():
        members, errors = draw_of(case)
        s_members, s_errors = draw_of(case, scalar=True)
        assert members.tolist() == s_members and errors == s_errors, case
        weights = LJ.make_weights(case["weights"], case["P"])
        mask = LJ.make_mask(case["mask"], case["n"])
        drawn = np.ones(case["n"], bool) if mask is None else mask != 0
        if case["weights"] in LJ.BAD_WEIGHT_KINDS:
            assert errors == 1 and (members == LJ.PLANTED).all(), case
        else:
            assert errors == 0 and (members[~drawn] == LJ.PLANTED).all()
            assert (members[drawn] >= 0).all() and (members[drawn] < case["P"]).all(), case         # always below P
            assert (weights[members[drawn]] > 0).all(), case                                          # never a member of weight 0
        seen.add((case["weights"], case["mask"], case["dtype"], case["first_game"], case["counter"]))
    for i, names in enumerate((LJ.WEIGHT_KINDS + LJ.BAD_WEIGHT_KINDS, LJ.MASK_KINDS, LJ.MEMBER_DTYPES, LJ.FIRST_GAMES, LJ.COUNTER_KINDS)):
        assert {s[i] for s in seen} == set(names)
    for wk in LJ.WEIGHT_KINDS:      # each weight kind meets every format, every first_game and every form of the counter
        for i, names in ((2, LJ.MEMBER_DTYPES), (3, LJ.FIRST_GAMES), (4, LJ.COUNTER_KINDS)):
            assert {s[i] for s in seen if s[0] == wk} == set(names), (wk, i)
    assert max(LJ.FIRST_GAMES) > 1 << 32 and sorted({c["n"] for c in LJ.all_draw_cases()}) == sorted(LJ.CASE_N)
    assert {c["P"] for c in LJ.all_draw_cases()} == set(LJ.CASE_P) == {1, 2, 3, 16}
    assert (LJ.make_weights("all_at_the_limit", 16) == (1 << 32) - 1).all() and (LJ.make_weights("one_at_the_limit", 16) == (1 << 32) - 1).sum() == 1
    for kind, C in ((k, c) for k in LJ.COUNTER_KINDS for c in (0, 5, (1 << 40) + 9)):
        by_value, on_device = LJ.split_counter(kind, C)
        assert by_value + (on_device or 0) == C and (on_device is None) == (kind == "by_value")


def test_a_shard_draws_what_the_batch_draws():
    w = np.array([3, 0, 5, 1], np.int64)
    for n, first in ((4099, 0), (300, (1 << 32) - 100), (257, (1 << 63) + 11)):
        whole, _ = LJ.draw(w, n, 21, 6, first)
        for g0 in (0, 1, 64, n - 1):
            tail, _ = LJ.draw(w, n - g0, 21, 6, first + g0)
            assert np.array_equal(tail, whole[g0:]), (n, first, g0)


def test_counters_seeds_and_the_other_streams_give_other_draws():
    from oracle.pz_oracle import philox4x32_10_numpy

    n, w = 4096, np.full(16, 1000, np.int64)
    base, _ = LJ.draw(w, n, 7, 0)
    for other in (LJ.draw(w, n, 7, 1), LJ.draw(w, n, 8, 0), LJ.draw(w, n, 7 + (1 << 32), 0), LJ.draw(w, n, 7, 1 << 32), LJ.draw(w, n, 7, 0, first_game=n)):
        assert (other[0] != base).mean() > 0.9                                        # 15 / 16 expected
    # the key is neither the plain seed (the env, the policy head, the random policy) nor the batch permutation's
    for seed in (0, 7, 0x123456789ABCDEF0):
        plain = (seed & 0xFFFFFFFF, seed >> 32)
        keys = {LJ.philox_key(seed), plain, BJ.philox_key(seed)}
        assert len(keys) == 3
        ctr = (np.arange(64), np.zeros(64), np.zeros(64), np.zeros(64))
        mine = philox4x32_10_numpy(ctr, LJ.philox_key(seed))
        for other in (plain, BJ.philox_key(seed)):
            theirs = philox4x32_10_numpy(ctr, other)
            assert not set(mine[0].tolist()) & set(theirs[0].tolist())
    assert LJ.philox_key(0) == LJ.KEY_XOR == (0x4C454147, 0x44524157)
    assert bytes.fromhex("%08X%08X" % LJ.KEY_XOR) == b"LEAGDRAW"


def test_the_draw_follows_its_weights():
    """one fixed seed, n = 65 536, weights (1, 2, 3, 0, 10): every member's count within 5 standard deviations of its mean.  A
    condition on the judge: a first seed that misses it (a few in a million) means the judge is wrong, not the seed."""
    n, w = 65536, np.array([1, 2, 3, 0, 10], np.int64)
    members, errors = LJ.draw(w, n, 2024, 0)
    assert errors == 0
    counts = np.bincount(members, minlength=5)
    q = w / w.sum()
    print(counts.tolist(), (n * q).tolist(), (5 * np.sqrt(n * q * (1 - q))).tolist())
    assert (np.abs(counts - n * q) <= 5 * np.sqrt(n * q * (1 - q))).all() and counts[3] == 0


def test_every_draw_mutant_is_caught_by_the_gpu_tests_own_cases():
    """the GPU test compares the member vector word for word: each mutant's differs from the definition's on some of its cases"""
    caught = {m: 0 for m in LJ.DRAW_MUTANTS}
    for case in LJ.all_draw_cases():
        want, _ = draw_of(case)
        for mutant in LJ.DRAW_MUTANTS:
            caught[mutant] += not np.array_equal(draw_of(case, mutant=mutant)[0], want)
    print(caught)
    assert len(LJ.DRAW_MUTANTS) == 6 and all(count > 0 for count in caught.values()), caught


# ---- the judge: the tally -----------------------------------------------------------------------------------------------------
def tally_of(case, x, mutant=None, scalar=False):
    args = (x["terminated"], x["buf1"], x["buf2"], case["stride"], x["members_p1"], x["members_p2"], case["P"], x["table"], x["errors"])
    return LJ.tally_scalar(*args) if scalar else LJ.tally(*args, mutant=mutant)


def test_the_two_formulations_of_the_tally_agree_and_every_mutant_is_caught():
    caught = {m: 0 for m in LJ.TALLY_MUTANTS}
    seen = set()
    for case in LJ.all_tally_cases():
        x = LJ.tally_inputs(case)
        table, errors = tally_of(case, x)
        s_table, s_errors = tally_of(case, x, scalar=True)
        assert np.array_equal(table, s_table) and errors == s_errors, case
        ended = x["terminated"] != 0
        added = table - x["table"]
        assert added[..., 0].sum() + (errors - x["errors"]) == ended.sum(), case          # every finished game counts exactly once
        assert (added[..., 1] <= added[..., 0]).all() and (added[..., 0] >= 0).all()
        if not case["invalid"]:
            assert errors == x["errors"]
        if not case["with_p1"]:
            assert (added[1:] == 0).all()
        for mutant in LJ.TALLY_MUTANTS:
            got = tally_of(case, x, mutant=mutant)
            caught[mutant] += not (np.array_equal(got[0], table) and got[1] == errors)
        seen.add((case["terminated"], case["stride"], case["score_dtype"], case["with_p1"], case["member_dtype"], case["invalid"]))
    print(caught)
    assert len(LJ.TALLY_MUTANTS) == 5 and all(count > 0 for count in caught.values()), caught
    for i, names in enumerate((LJ.TERMINATION_KINDS, LJ.SCORE_STRIDES, LJ.SCORE_DTYPES, (False, True), LJ.MEMBER_DTYPES, (False, True))):
        assert {s[i] for s in seen} == set(names)
    assert set(LJ.SCORE_STRIDES) == {1, 8, 3} and {"none", "all", "one_lane_per_wave", "last_row_only"} <= set(LJ.TERMINATION_KINDS)
    # a second call adds to the first
    case = LJ.tally_cases(257, 3)[7]
    x = LJ.tally_inputs(case)
    once = tally_of(case, x)
    twice = tally_of(case, {**x, "table": once[0], "errors": once[1]})
    assert np.array_equal(twice[0] - once[0], once[0] - x["table"]) and twice[1] - once[1] == once[1] - x["errors"]


# ---- pfsp_weights -------------------------------------------------------------------------------------------------------------
def test_pfsp_weights_equal_their_restatement_and_prefer_stronger_opponents():
    import torch

    from pikazoo_amd import league

    rng = np.random.default_rng(5)
    for P, active, power, prior, row in ((1, 1, 2.0, 8.0, 0), (4, 3, 2.0, 8.0, 0), (16, 16, 1.0, 2.0, 0), (16, 9, 3.5, 0.5, 2), (8, 8, 0, 8.0, 7)):
        table = np.zeros((P, P, 4), np.int64)
        table[..., 0] = rng.integers(0, 5000, (P, P))
        table[..., 1] = (table[..., 0] * rng.random((P, P))).astype(np.int64)
        table[0, 0] = 0                                                        # a member without games: an even match
        got = league.pfsp_weights(torch.from_numpy(table), active, power, prior, row)
        want = LJ.pfsp_weights(table, active, power, prior, row)
        assert got.dtype == torch.int64 and tuple(got.shape) == (P,)
        assert np.abs(got.numpy() - want).max() <= 1, (P, active, power)
        assert (got[active:] == 0).all() and (got[:active] >= 1).all() and (got < 1 << 32).all()
    # monotone: more losses, more weight; all games won still leaves weight 1 or more; none played is an even match
    table = np.zeros((16, 16, 4), np.int64)
    table[0, :, 0] = 100
    table[0, :, 1] = np.arange(16) * 100 // 15                                 # member 0 never beaten ... member 15 always
    w = league.pfsp_weights(torch.from_numpy(table), 16).numpy()
    assert (np.diff(w) < 0).all() and w[15] >= 1
    fresh = league.pfsp_weights(torch.zeros((3, 3, 4), dtype=torch.int64), 3)
    assert fresh.tolist() == [1 << 18] * 3                                     # (1 - 1/2)^2 * 2^20
    for bad in (dict(table=torch.zeros(3, 3, 4)), dict(table=torch.zeros((3, 4, 4), dtype=torch.int64)), dict(table=torch.zeros((3, 3, 3), dtype=torch.int64)),
                dict(table=torch.zeros((17, 17, 4), dtype=torch.int64)), dict(table=None), dict(active=0), dict(active=4), dict(active=2.0), dict(active=True),
                dict(row=3), dict(row=-1), dict(power=-1.0), dict(power="2"), dict(prior_games=0), dict(prior_games=-2.0)):
        with pytest.raises(ValueError):
            league.pfsp_weights(**{**dict(table=torch.zeros((3, 3, 4), dtype=torch.int64), active=3), **bad})
            pytest.fail(f"bad pfsp_weights {sorted(bad)} was accepted")


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_league_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, batch, league, net, pool

    assert header_functions("pikazoo_league.h") == NAMES == sorted(league.SIGNATURES) == dynamic_pz_symbols(pz_build.LEAGUE_LIB)
    assert pz_build.library_id(pz_build.LEAGUE_LIB) == pz_build.source_id() == lib.pz_league_build_id().decode()
    assert not pz_build.needs_build()
    assert len(pz_build.TARGETS) == 11 and pz_build.TARGETS[-1] == (pz_build.LEAGUE_LIB, pz_build.LEAGUE_SOURCES)
    assert pz_build.LEAGUE_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_league.h") in pz_build.DEPS
    assert lib.pz_league_abi_version() == league.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_league.h").read_text()
    assert "#define PZ_LEAGUE_ABI_VERSION 1" in header
    assert f"#define PZ_LEAGUE_MAX_MEMBERS {league.MAX_MEMBERS}\n" in header and league.MAX_MEMBERS == LJ.MAX_MEMBERS == pool.MAX_MEMBERS == 16
    assert f"#define PZ_LEAGUE_CELL_WORDS {league.CELL_WORDS}\n" in header and league.CELL_WORDS == LJ.CELL == 4
    for key, value in league.SCORE_FORMATS.items():
        assert re.search(r"PZ_LEAGUE_SCORE_%s = %d\b" % (str(key).split(".")[-1].upper(), value), header), key
    assert [str(d).split(".")[-1] for d in league.SCORE_FORMATS] == list(LJ.SCORE_DTYPES)
    # the member formats are the pool's values
    assert league.MEMBER_FORMATS == pool.MEMBER_FORMATS and [str(d).split(".")[-1] for d in league.MEMBER_FORMATS] == list(LJ.MEMBER_DTYPES)
    assert league.KEY_XOR == LJ.KEY_XOR and all("0x%08X" % k in header for k in LJ.KEY_XOR)
    # no other library holds any of the names, and the older libraries' ABI versions did not move
    others = [out for out, _ in pz_build.TARGETS[:-1]]
    assert len(others) == 10
    for other in others:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
        assert pz_build.library_id(other) == pz_build.source_id(), other
    assert not set(NAMES) & set(_native.exported_names())
    assert _native.load().pz_abi_version() == 10
    assert net.load().pz_net_abi_version() == net.ABI_VERSION == 1 and batch.load().pz_batch_abi_version() == batch.ABI_VERSION == 1
    assert pool.load().pz_pool_abi_version() == pool.ABI_VERSION == 1
    # both declarations stand in INTEGRATION.md as the header has them
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_league.h" in doc and "libpikazoo_league.so" in doc
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("pz_league_tally", 13), ("pz_league_draw", 12)):
        args = declared_arguments(bare, name)
        assert len(args) == count == len(league.SIGNATURES[name][1]) and declared_arguments(doc, name) == args, name


def test_importing_the_other_modules_does_not_load_the_league_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim, batch, pool; "
            "assert 'pikazoo_amd.league' not in sys.modules; import pikazoo_amd as p; assert 'league' in p.__all__; "
            "p.league.tally; p.league.draw; p.league.pfsp_weights; p.league.Matchmaker; "
            "assert 'pikazoo_amd.league' in sys.modules and p.league._lib is None; "
            "assert not any('libpikazoo_league' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    # ... and importing the league module alone imports neither the pool module nor any library
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from pikazoo_amd import league; "
            "assert 'pikazoo_amd.pool' not in sys.modules and 'pikazoo_amd.batch' not in sys.modules and league._lib is None; "
            "assert not any('libpikazoo_' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_league_library(pz_build):
    """TWO kernels.  Neither uses scratch or spills a register: the draw keeps its sixteen prefix sums in registers (its loops
    over the members are unrolled), the tally's only array is its [16][16][4] table of 64-bit words in LDS: 8 KiB, plus the
    errors word and the barrier's vote (at most 8.5 KiB).  Read from the code object's notes alone."""
    import kernel_notes

    notes = kernel_notes.notes(pz_build.LEAGUE_LIB)
    short = lambda name: name.replace("void ", "").split("(")[0]  # noqa: E731
    assert sorted(short(name) for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".vgpr_count"] <= 64, (name, row)
        if "tally" in name:
            assert 16 * 16 * 4 * 8 + 4 <= row[".group_segment_fixed_size"] <= 8704, (name, row)
        else:
            assert row[".group_segment_fixed_size"] == 0, (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})


# ---- argument checking --------------------------------------------------------------------------------------------------------
FAKE = 4096
# by default the LAST check fails: members_p2 is not aligned to its int32 elements
TALLY = dict(terminated=FAKE, score_p1=FAKE, score_p2=FAKE + 4, score_format=0, score_stride=1, members_p1=FAKE, members_p2=FAKE + 2, member_format=1,
             n=64, num_members=3, table=FAKE, errors=FAKE, stream=None)
# ... here: errors is not 4-byte aligned
DRAW = dict(weights=FAKE, num_members=3, seed=5, counter=0, counter_dev=FAKE, first_game=0, mask=FAKE + 1, members=FAKE, member_format=2, n=64,
            errors=FAKE + 2, stream=None)


def test_argument_validation_of_the_tally(lib):
    """Every return code in the documented order.  The LAST check (the alignment of a member vector) is planted in every
    call that is meant to pass the earlier ones: -4 then says that they all passed."""
    def call(**over):
        a = dict(TALLY)
        assert not set(over) - set(a)
        a.update(over)
        return lib.pz_league_tally(*a.values())

    passes = lambda **kw: call(**kw) == -4  # noqa: E731
    ok = dict(members_p2=FAKE)
    assert passes() and passes(n=1 << 30) and passes(num_members=1) and passes(num_members=16) and passes(members_p1=None)
    assert passes(score_stride=8, score_format=1) and passes(score_stride=(1 << 31) - 1) and passes(n=0)
    assert call(n=0, **ok) == 0 and call(n=0, terminated=None, score_p1=None, score_p2=None, members_p1=None, members_p2=None) == 0
    # NULL
    for name in ("terminated", "score_p1", "score_p2", "members_p2", "table", "errors"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, table=None) == -1 and call(n=0, errors=None) == -1
    # sizes
    for bad in (dict(n=-1), dict(n=(1 << 30) + 1), dict(num_members=0), dict(num_members=17), dict(num_members=-3), dict(score_stride=0),
                dict(score_stride=-8), dict(score_stride=1 << 60)):
        assert call(**bad) == -2, bad
    # formats
    for name, count in (("score_format", 2), ("member_format", 3)):
        assert call(**{name: count}) == -3 and call(**{name: -1}) == -3, name
        for value in range(count):
            assert call(n=0, **{name: value}, members_p1=None, members_p2=None) == 0, (name, value)
    # alignment: 8 bytes for the table and the errors word, the element for scores and members
    for name in ("table", "errors"):
        for off in (1, 2, 4):
            assert call(**{**ok, name: FAKE + off}) == -4, (name, off)
        assert call(n=0, **{**ok, name: FAKE + 8}) == 0
    for name in ("score_p1", "score_p2", "members_p1", "members_p2"):
        assert call(**{**ok, name: FAKE + 1}) == -4 and call(**{**ok, name: FAKE + 2}) == -4, name
        assert call(n=0, **{**ok, name: FAKE + 4}) == 0, name
    assert call(n=0, score_format=1, score_p1=FAKE + 2, score_p2=FAKE + 6, **ok) == 0 and call(score_format=1, score_p2=FAKE + 1, **ok) == -4
    assert call(n=0, member_format=0, members_p1=FAKE + 1, members_p2=FAKE + 3) == 0
    assert call(member_format=2, members_p2=FAKE + 4) == -4 and call(member_format=2, members_p1=FAKE + 4, **ok) == -4
    # the order of the checks: NULL, size, config, alignment
    assert call(table=None, n=-1, score_format=9) == -1 and call(n=-1, score_format=9) == -2 and call(score_stride=0, member_format=9) == -2
    assert call(score_format=9) == -3 and call(member_format=9) == -3 and call() == -4


def test_argument_validation_of_the_draw(lib):
    """pz_league_draw: its planted last failure is a misaligned `errors`"""
    def call(**over):
        a = dict(DRAW)
        assert not set(over) - set(a)
        a.update(over)
        return lib.pz_league_draw(*a.values())

    passes = lambda **kw: call(**kw) == -4  # noqa: E731
    ok = dict(errors=FAKE)
    assert passes() and passes(n=1 << 30) and passes(num_members=1) and passes(num_members=16) and passes(counter_dev=None) and passes(mask=None)
    assert passes(counter=(1 << 62) - 1) and passes(first_game=(1 << 63) - 1) and passes(first_game=-5) and passes(seed=(1 << 64) - 1) and passes(n=0)
    assert call(n=0, **ok) == 0 and call(n=0, members=None, **ok) == 0
    for name in ("weights", "members", "errors"):
        assert call(**{name: None}) == -1, name
    assert call(n=0, weights=None) == -1 and call(n=0, errors=None) == -1
    for bad in (dict(n=-1), dict(n=(1 << 30) + 1), dict(num_members=0), dict(num_members=17), dict(num_members=-1), dict(counter=1 << 62),
                dict(counter=(1 << 64) - 1)):
        assert call(**bad) == -2, bad
    assert call(member_format=3) == -3 and call(member_format=-1) == -3
    for value in range(3):
        assert call(n=0, member_format=value, **ok) == 0
    for name in ("weights", "counter_dev"):
        for off in (1, 2, 4):
            assert call(**{**ok, name: FAKE + off}) == -4, (name, off)
        assert call(n=0, **{**ok, name: FAKE + 8}) == 0
    for off in (1, 2, 3):
        assert call(errors=FAKE + off) == -4
    assert call(n=0, errors=FAKE + 4) == 0
    assert call(members=FAKE + 4, **ok) == -4 and call(n=0, members=FAKE + 8, **ok) == 0
    assert call(member_format=1, members=FAKE + 2, **ok) == -4 and call(n=0, member_format=1, members=FAKE + 4, **ok) == 0
    assert call(n=0, member_format=0, members=FAKE + 1, mask=FAKE + 3, **ok) == 0
    assert call(weights=None, n=-1, member_format=7) == -1 and call(n=-1, member_format=7) == -2 and call(counter=1 << 62, member_format=7) == -2
    assert call(member_format=7) == -3 and call() == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """shape, dtype, device, stride and range errors raise ValueError -- on CPU tensors the device check stands behind the
    others, so every one of them is reachable here, and none of them asks for the library"""
    import torch

    from pikazoo_amd import league, net, pool

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(league, "load", refuse)
    n, P = 8, 3
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)  # noqa: E731
    term = torch.zeros(n, dtype=torch.bool)
    state = torch.zeros((44, 16), dtype=torch.int32)
    scores32 = state[:, :n][36:38].t()                                         # the int32 state's view: strides (1, 16)
    scores16 = torch.zeros(16 * 16, dtype=torch.uint8).view(torch.int16).view(16, 8)[:n, 4:6]     # the packed state's: (8, 1)
    members = i64(n)
    for scores in (scores32, scores16, torch.zeros((n, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match="GPU"):
            league.tally(term, scores, members, P)
    with pytest.raises(ValueError, match="GPU"):
        league.tally(term.to(torch.uint8), scores16, members.to(torch.uint8), 16, table=i64(16, 16, 4), members_p1=members.to(torch.uint8), errors=i64(1))
    bad_tallies = [
        dict(terminations=[0] * n), dict(terminations=torch.zeros(n)), dict(terminations=torch.zeros((n, 1), dtype=torch.bool)),
        dict(terminations=torch.zeros(2 * n, dtype=torch.bool)[::2]), dict(terminations=torch.zeros(n + 1, dtype=torch.bool)),
        dict(scores=None), dict(scores=torch.zeros((n, 2))), dict(scores=torch.zeros((n, 2), dtype=torch.int64)), dict(scores=torch.zeros((n, 3), dtype=torch.int32)),
        dict(scores=torch.zeros((2, n), dtype=torch.int32)), dict(scores=torch.zeros(n, dtype=torch.int32)), dict(scores=torch.zeros((n + 1, 2), dtype=torch.int16)),
        dict(scores=torch.zeros((1, 2), dtype=torch.int32).expand(n, 2)),                                           # stride 0: every game the same scores
        dict(members=[0] * n), dict(members=torch.zeros(n, dtype=torch.int16)), dict(members=torch.zeros(n)), dict(members=i64(n + 1)), dict(members=i64(n, 1)),
        dict(members=i64(2 * n)[::2]), dict(members_p1=i64(n + 1)), dict(members_p1=torch.zeros(n, dtype=torch.int32)), dict(members_p1="zero"),
        dict(num_members=0), dict(num_members=17), dict(num_members=3.0), dict(num_members=True),
        dict(table=i64(P, P, 3)), dict(table=i64(P + 1, P + 1, 4)), dict(table=torch.zeros((P, P, 4), dtype=torch.int32)), dict(table=i64(P, P, 8)[:, :, ::2]),
        dict(table="table"), dict(errors=i64(2)), dict(errors=torch.zeros(1, dtype=torch.int32)), dict(errors=7),
        dict(table=torch.zeros((P, P, 4), dtype=torch.int64, device="meta")), dict(members=torch.zeros(n, dtype=torch.int64, device="meta")),
    ]
    for i, bad in enumerate(bad_tallies):
        args = dict(terminations=term, scores=scores32, members=members, num_members=P)
        args.update(bad)
        with pytest.raises(ValueError):
            league.tally(**args)
            pytest.fail(f"bad tally {i} was accepted: {sorted(bad)}")
    shared = i64(P * P * 4 + n)
    with pytest.raises(ValueError, match="overlaps"):
        league.tally(term, scores32, shared[:n], P, table=shared[4:4 + P * P * 4].view(P, P, 4))
    # the draw
    weights = torch.tensor([1, 2, 3], dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        league.draw(weights, n, seed=0)
    with pytest.raises(ValueError, match="GPU"):
        league.draw(weights, n, seed=-1, counter=i64(1), first_game=1 << 40, mask=term, out=torch.zeros(n, dtype=torch.uint8),
                    errors=torch.zeros(1, dtype=torch.int32))
    bad_draws = [
        dict(weights=[1, 2]), dict(weights=torch.ones(3)), dict(weights=torch.ones(3, dtype=torch.int32)), dict(weights=i64(0)), dict(weights=i64(17)),
        dict(weights=i64(3, 1)), dict(weights=i64(6)[::2]), dict(n=-1), dict(n=(1 << 30) + 1), dict(n=8.0), dict(n=True), dict(seed=1.5), dict(seed=None),
        dict(counter=-1), dict(counter=1 << 62), dict(counter=0.0), dict(counter=i64(2)), dict(counter=torch.zeros(1, dtype=torch.int32)),
        dict(first_game=1 << 63), dict(first_game=2.0), dict(mask=torch.zeros(n)), dict(mask=torch.zeros(n + 1, dtype=torch.bool)),
        dict(mask=torch.zeros(2 * n, dtype=torch.uint8)[::2]), dict(out=i64(n + 1)), dict(out=torch.zeros(n, dtype=torch.int16)), dict(out=i64(2 * n)[::2]),
        dict(out=[0] * n), dict(dtype=torch.int16), dict(dtype=torch.float32), dict(errors=i64(1)), dict(errors=torch.zeros(2, dtype=torch.int32)),
        dict(out=torch.zeros(n, dtype=torch.int64, device="meta")), dict(mask=torch.zeros(n, dtype=torch.bool, device="meta")),
    ]
    for i, bad in enumerate(bad_draws):
        args = dict(weights=weights, n=n, seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            league.draw(**args)
            pytest.fail(f"bad draw {i} was accepted: {sorted(bad)}")
    with pytest.raises(ValueError, match="overlaps"):
        league.draw(shared[:3], n, seed=0, out=shared[2:2 + n])
    # the matchmaker: everything it owns, before any launch
    model = net.ActorCritic()
    snapshots = pool.Snapshots(model, 4)
    mm = league.Matchmaker(snapshots, n, seed=3, first_game=100)
    assert tuple(mm.table.shape) == (4, 4, 4) and mm.table.dtype == torch.int64 and not mm.table.any()
    assert tuple(mm.members.shape) == (n,) and mm.members.dtype == torch.int64 and not mm.members.any()
    assert mm.counter.dtype == torch.int64 and mm.counter.tolist() == [0] and mm.tally_errors.dtype == torch.int64 and mm.draw_errors.dtype == torch.int32
    assert mm.plans == {} and mm.check() is mm
    assert mm.weights().tolist() == [1 << 18, 0, 0, 0]
    mm.table[:] = 5
    assert mm.push() == 1 and len(snapshots) == 2
    assert not mm.table[1].any() and not mm.table[:, 1].any() and (mm.table[0, 0] == 5).all() and (mm.table[2:, 2:] == 5).all()
    assert mm.weights().tolist()[2:] == [0, 0] and mm.weights().tolist()[1] == 1 << 18
    rates = mm.win_rates()
    assert rates.dtype == torch.float64 and float(rates[0]) == 1.0 and bool(torch.isnan(rates[1]))
    for call in (lambda: mm.record(term, scores32), lambda: mm.rematch(), lambda: mm.rematch(mask=term)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    mm.tally_errors[0] = 2
    with pytest.raises(ValueError, match="2 finished games"):
        mm.check()
    mm.tally_errors[0] = 0
    mm.draw_errors[0] = 1
    with pytest.raises(ValueError, match="weights"):
        mm.check()
    for bad in (dict(snapshots=model), dict(num_envs=0), dict(num_envs=2.0), dict(seed="s"), dict(first_game=-1), dict(power=-1), dict(prior_games=0)):
        with pytest.raises(ValueError):
            league.Matchmaker(**{**dict(snapshots=snapshots, num_envs=n, seed=0), **bad})
            pytest.fail(f"bad Matchmaker {sorted(bad)} was accepted")
    assert "README" in league.Matchmaker.__doc__ and "rematch(mask=terminations)" in league.Matchmaker.__doc__
