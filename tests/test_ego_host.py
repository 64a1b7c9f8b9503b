"""CPU tests (no GPU needed) of the egocentric rows: the judge of the GPU test (tests/ego_judge.py) against a second, scalar
formulation and against torch's CPU bfloat16; the involutions; the header's five bounds on the distance from "normalise the
mirrored integer", exhaustively over each mirrored column's bounds; the MEANING of the mirror through the oracle's observe on
planted states; ``PI`` derived from the key table and from SimplifyAction's tuples; every mutant of the judge caught by the GPU
test's own cases; a numpy model of the kernels' three index walks, with the grid cap read from the source, which holds that no
case of the first table takes a thread round its loop, that every large case takes every thread round twice and some a third
time, and that four mutants of the walks and an actions loop of one trip are caught by the large cases alone (the
element-by-element ones only in place: out of place an element done twice is stored twice with the same value); and the
library: exports, build id, lazy loading, the new build tuple, the kernel census, every return code
that needs no launch in the header's order, and every ValueError of the binding and the wrapper.

No call here ever passes every check with rows to run: a call that passes them all has rows = 0 and launches nothing (so the
overlap code, which stands behind that return, is the GPU test's)."""
import re
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ego_judge as EJ
from test_cabi_and_host import dynamic_pz_symbols, header_functions

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_ego_abi_version", "pz_ego_actions", "pz_ego_build_id", "pz_ego_error_string", "pz_ego_rows"]
FAKE = 4096
MIRRORED = EJ.COURT + EJ.SIGN


@pytest.fixture(autouse=True)
def the_binding():
    """every test of this file is about pikazoo_amd.ego, the judge's included: none of them runs without the module"""
    from pikazoo_amd import ego

    return ego


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import ego

    return ego.load()


# ---- the judge in a second formulation -------------------------------------------------------------------------------------------
def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def scalar_mirror(word, col, fmt):
    """one element as its unsigned word, in pure Python: floats through struct, bfloat16 through integer arithmetic"""
    if col not in MIRRORED:
        return word
    M = EJ.WIDTH if col in EJ.COURT else 0
    if fmt == 0:
        v = word - (1 << 32) if word >> 31 else word
        return (M - v) & 0xFFFFFFFF
    if fmt == 2:
        v = word - (1 << 16) if word >> 15 else word
        return (M - v) & 0xFFFF
    c = (392 / 412 if col == 26 else 1.0) if fmt in EJ.NORMALISED else float(M)
    c = f32(c)
    if fmt == 1:
        s = struct.unpack("<f", struct.pack("<I", word))[0]
        return struct.unpack("<I", struct.pack("<f", c - s))[0]   # (c - s is exact in double: one rounding)
    if fmt in (3, 5):
        s = struct.unpack("<e", struct.pack("<H", word))[0]
        return struct.unpack("<H", struct.pack("<e", f32(c - s)))[0]
    s = struct.unpack("<f", struct.pack("<I", word << 16))[0]
    u = struct.unpack("<I", struct.pack("<f", c - s))[0]
    low, keep = u & 0xFFFF, u >> 16
    if low > 0x8000 or (low == 0x8000 and keep & 1):
        keep += 1
    return keep & 0xFFFF


@pytest.mark.parametrize("fmt", list(EJ.FORMATS))
def test_the_judge_agrees_with_a_scalar_formulation(fmt):
    assert f32(392 / 412) == float(EJ.C26) == float.fromhex("0x1.e72548p-1")
    stored = EJ.encode(EJ.content(24, 3), fmt)
    got = EJ.bits(EJ.mirror(stored, fmt))
    words = EJ.bits(stored)
    for r in range(stored.shape[0]):
        for j in range(EJ.DIM):
            assert int(got[r, j]) == scalar_mirror(int(words[r, j]), j, fmt), (fmt, r, j)
    copied = [j for j in range(EJ.DIM) if j not in MIRRORED]
    assert len(copied) == 27 and np.array_equal(got[:, copied], words[:, copied])


def test_the_bfloat16_of_the_judge_is_torchs():
    import torch

    x = np.concatenate([np.arange(-500, 500, dtype=np.float32), np.random.default_rng(0).random(50000, dtype=np.float32) * 2 - 0.5,
                        np.array([0.0, 1.0, 256.0, 257.0, 258.0, 259.0, 431.0, 432.0, 3.0e38, -3.0e38], np.float32)])
    ours = EJ.f32_to_bf16(x)
    theirs = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(ours.view(np.int16), theirs.view(torch.int16).numpy())
    assert np.array_equal(EJ.bf16_to_f32(ours), theirs.to(torch.float32).numpy())
    for fmt in (4, 6):   # the whole mirror, in torch's own bfloat16 arithmetic on the CPU
        stored = EJ.encode(EJ.content(64, 1), fmt)
        t = torch.from_numpy(stored.view(np.int16)).view(torch.bfloat16).to(torch.float32)
        want = t.clone()
        for j in MIRRORED:
            c = (float(EJ.C26) if j == 26 else 1.0) if fmt == 6 else float(EJ.WIDTH if j in EJ.COURT else 0)
            want[:, j] = torch.tensor(c, dtype=torch.float32) - t[:, j]
        want = want.to(torch.bfloat16).view(torch.int16).numpy()
        assert np.array_equal(EJ.mirror(stored, fmt).view(np.int16), want), fmt


def test_involutions():
    for fmt in (0, 2, 3):   # exact arithmetic: twice is the identity
        stored = EJ.encode(EJ.content(64, 2), fmt)
        assert np.array_equal(EJ.bits(EJ.mirror(EJ.mirror(stored, fmt), fmt)), EJ.bits(stored)), fmt
    assert sorted(EJ.PI) == list(range(18)) and all(EJ.PI[EJ.PI[a]] == a for a in range(18))
    assert [a for a in range(18) if EJ.PI[a] != a] == [3, 4, 6, 7, 8, 9, 11, 12, 14, 15, 16, 17]
    from pikazoo_amd import ego

    assert ego.PI == EJ.PI and ego.COURT_COLUMNS == EJ.COURT and ego.SIGN_COLUMNS == EJ.SIGN and ego.COURT_WIDTH == EJ.WIDTH
    header = (REPO / "include" / "pikazoo_ego.h").read_text()
    assert "pi = (" + ", ".join(map(str, EJ.PI)) + ")" in header and "0x1.e72548p-1" in header


def test_the_bounds_of_the_header_hold_for_every_value_inside_the_columns_bounds():
    """distance from "normalise the mirrored integer": float32 <= 2^-24, float16 <= 2^-11, bfloat16 <= 2^-8 (normalised); none
    in the raw exact formats; raw bfloat16 within 2 of the mirrored integer"""
    worst = {}
    for j in MIRRORED:
        M = EJ.WIDTH if j in EJ.COURT else 0
        v = np.arange(EJ.LOW[j], EJ.HIGH[j] + 1)
        rows = np.tile(EJ.LOW, (len(v), 1))
        rows[:, j] = v
        mirrored = rows.copy()
        mirrored[:, j] = M - v
        ideal = (mirrored[:, j] - EJ.LOW[j]) / (EJ.HIGH[j] - EJ.LOW[j])            # float64
        for fmt in EJ.FORMATS:
            got = EJ.mirror(EJ.encode(rows, fmt), fmt)[:, j]
            if fmt in (0, 2):
                err = np.abs(got.astype(np.int64) - mirrored[:, j])
            elif fmt == 3:
                err = np.abs(got.astype(np.float64) - mirrored[:, j])
            elif fmt == 4:
                err = np.abs(EJ.bf16_to_f32(got).astype(np.float64) - mirrored[:, j])
            else:
                # against the fused form: the float32 quotient of the mirrored integer, rounded into the format
                fused = EJ.widen(EJ.encode(mirrored, fmt)[:, j], fmt).astype(np.float64)
                err = np.maximum(np.abs(EJ.widen(got, fmt).astype(np.float64) - fused), 0)
                assert np.abs(EJ.widen(got, fmt).astype(np.float64) - ideal).max() <= {1: 2.0 ** -23, 5: 2.0 ** -10, 6: 2.0 ** -7}[fmt]
            worst[fmt] = max(worst.get(fmt, 0), float(err.max()))
    print({EJ.FORMATS[f]: w for f, w in worst.items()})
    assert worst[0] == worst[2] == worst[3] == 0
    assert worst[4] <= 2
    assert worst[1] <= 2.0 ** -24 and worst[5] <= 2.0 ** -11 and worst[6] <= 2.0 ** -8


# ---- what the mirror MEANS ---------------------------------------------------------------------------------------------------------
def planted_states(n, seed):
    """int32 states [44, n] with every observed field somewhere inside its bounds"""
    rng = np.random.default_rng(seed)
    st = np.zeros((44, n), np.int32)
    for base in (0, 13):
        st[base + 0] = rng.integers(32, 401, n)       # x
        st[base + 1] = rng.integers(108, 245, n)      # y
        st[base + 2] = rng.integers(-15, 17, n)       # y velocity
        st[base + 3] = rng.integers(0, 7, n)          # state
        st[base + 4] = rng.integers(0, 5, n)          # frame number
        st[base + 5] = rng.integers(0, 2, n)          # arm swing direction
        st[base + 6] = rng.integers(-2, 4, n)         # delay before next frame
        st[base + 7] = rng.integers(-1, 2, n)         # diving direction
        st[base + 8] = rng.integers(-2, 4, n)         # lying down duration left
        st[base + 9] = rng.integers(0, 2, n)          # collision with ball happened
        st[base + 12] = rng.integers(0, 2, n)         # power hit key is down previous
    for at, (lo, hi) in {26: (20, 432), 27: (0, 252), 28: (-20, 20), 29: (-124, 124), 30: (0, 1), 31: (0, 432), 32: (0, 252), 33: (0, 432),
                         34: (0, 252)}.items():
        st[at] = rng.integers(lo, hi + 1, n)
    st[40] = rng.integers(0, 2, n)
    return st


def mirrored_state(st):
    """the mirrored game: the players swapped, x -> 432 - x, the diving directions and the ball's x velocity negated"""
    out = st.copy()
    out[0:13], out[13:26] = st[13:26], st[0:13]
    for x in (0, 13, 26, 31, 33):
        out[x] = EJ.WIDTH - out[x]
    for d in (7, 20, 28):
        out[d] = -out[d]
    return out


def test_the_mirrored_row_of_player_2_is_player_1s_row_in_the_mirrored_game(oracle):
    n = 512
    S = planted_states(n, 11)
    S2 = mirrored_state(S)
    assert np.array_equal(mirrored_state(S2), S)

    def observe(state, normalize):
        env = oracle.OracleEnv(n, oracle.make_config(normalize_obs=normalize))
        env.state[:] = state
        return env.observe()

    p1, p2 = observe(S, False)
    q1, q2 = observe(S2, False)
    assert not np.array_equal(p2, q1) and (p1 != q2).any(axis=0).sum() >= 8          # (the mirror is not the identity here)
    touched = sorted(np.nonzero((EJ.mirror(p2, 0) != p2).any(axis=0))[0])
    assert touched == sorted(MIRRORED), touched
    assert np.array_equal(EJ.mirror(p2, 0), q1) and np.array_equal(EJ.mirror(q2, 0), p1)
    assert np.array_equal(EJ.mirror(p1, 0), q2) and np.array_equal(EJ.mirror(q1, 0), p2)   # (either side)
    # the normalised rows: within the header's 2^-24 of the mirrored game's
    n1, n2 = observe(S, True)
    m1, m2 = observe(S2, True)
    assert np.array_equal(n2, EJ.encode(p2, 1))
    assert np.abs(EJ.mirror(n2, 1).astype(np.float64) - m1).max() <= 2.0 ** -24
    assert np.abs(EJ.mirror(m2, 1).astype(np.float64) - n1).max() <= 2.0 ** -24


def test_pi_is_the_key_table_with_left_and_right_swapped():
    """derived here from the oracle's key table (pikazoo_env.py:121-138: left right up down power_hit), from the kernel's
    packed one, and from SimplifyAction's two tuples"""
    text = (REPO / "oracle" / "pz_oracle.c").read_text()
    body = text[text.index("ACTION_KEY_MAP[18][5]"):]
    body = body[:body.index("};")]
    keys = [tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{(\d, \d, \d, \d, \d)\}", body)]
    assert len(keys) == 18 == len(set(keys))
    swapped = [(k[1], k[0]) + k[2:] for k in keys]
    assert tuple(keys.index(k) for k in swapped) == EJ.PI
    packed = re.search(r"kKeys\[18\] = \{([^}]*)\}", (REPO / "pika-zoo_amd" / "csrc" / "pz_physics.hpp").read_text()).group(1)
    packed = [int(v, 16) for v in packed.replace("\n", " ").split(",")]
    flip = [(k & ~3) | ((k & 1) << 1) | ((k >> 1) & 1) for k in packed]
    assert tuple(packed.index(k) for k in flip) == EJ.PI
    from pikazoo_amd.wrappers.simplify_action import ACTION_MAP

    assert tuple(EJ.PI[a] for a in ACTION_MAP["player_1"]) == ACTION_MAP["player_2"]
    a = np.array(list(range(18)) + [-1, 18, 255, (1 << 32) + 3], np.int64)
    assert EJ.mirror_actions(a).tolist() == list(EJ.PI) + [-1, 18, 255, (1 << 32) + 3]


# ---- the cases of the GPU test and the mutants ------------------------------------------------------------------------------------
CASES = EJ.row_cases()
LARGE = EJ.LARGE_CASES
SOURCE = (REPO / "pika-zoo_amd" / "csrc" / "pz_ego.hip").read_text()


def source_constant(name):
    """a ``constexpr int`` of pz_ego.hip, read from its text: a change of the cap must move the model below with it"""
    found = re.findall(rf"^constexpr int {name} = (\d+);", SOURCE, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


K_THREADS, K_MAX_BLOCKS = source_constant("kThreads"), source_constant("kMaxBlocks")
STRIDE = K_THREADS * K_MAX_BLOCKS            # threads of a capped grid


def test_the_case_table_holds_what_the_kernel_can_get_wrong():
    assert {c["rows"] for c in CASES} == set(EJ.ROWS) | {195} and set(EJ.ROWS) == {1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257}
    for fmt in EJ.FORMATS:
        mine = [c for c in CASES if c["fmt"] == fmt]
        assert {c["rows"] for c in mine} >= set(EJ.ROWS)
        assert {(c["in_pitch"], c["out_pitch"]) for c in mine} >= {(35, 35), (36, 35), (35, 36), (35, 40), (40, 35), (36, 40), (40, 36)}
        assert {(c["in_offset"], c["out_offset"]) for c in mine if (c["in_pitch"], c["out_pitch"]) == (35, 35)} >= {(0, 0), (35, 35), (1, 1), (1, 0)}
        assert {c["inplace"] for c in mine} == {True, False} and any(c["inplace"] and c["in_pitch"] > 35 for c in mine)
    for c in CASES:
        assert not c["inplace"] or (c["in_pitch"], c["in_offset"]) == (c["out_pitch"], c["out_offset"])
    values = EJ.content(8, 0)
    assert (values[0] == EJ.LOW).all() and (values[1] == EJ.HIGH).all() and len(set(values[3] - EJ.LOW)) >= 16
    assert ((values[2] >= EJ.LOW) & (values[2] <= EJ.HIGH)).all()
    above = EJ.bf16_to_f32(EJ.encode(values, 4))
    assert (above > 256).sum() >= 5
    for dtype in EJ.ACTION_DTYPES:
        seen = set(EJ.action_case(dtype, 257).tolist())
        assert seen == set(EJ.action_values(dtype).tolist()) >= set(range(18)) | {18}
    assert (1 << 32) + 3 in EJ.action_values(np.int64) and 255 in EJ.action_values(np.uint8) and -1 in EJ.action_values(np.int16)
    # the second table: the same formats past one grid stride (what it reaches that the first cannot: the walks below)
    assert EJ.row_cases() == CASES and not any(c.get("large") for c in CASES) and all(c["large"] for c in LARGE)
    assert max(c["rows"] for c in CASES) * EJ.DIM < STRIDE
    for fmt in EJ.FORMATS:
        mine = [c for c in LARGE if c["fmt"] == fmt]
        size = EJ.STORAGE[fmt]().itemsize
        flat, pitched = [c for c in mine if is_flat(c)], [c for c in mine if not is_flat(c)]
        assert len(flat) == 4 and len(pitched) == 5 and {c["rows"] for c in flat} == {EJ.LARGE_ROWS[size]}
        assert {c["rows"] for c in pitched} == {EJ.LARGE_ROWS["pitched"]}
        assert {(c["in_offset"], c["inplace"]) for c in flat} == {(0, False), (0, True), (1, False), (35, True)}
        assert {flat_split(c)[0] for c in flat} == ({0, 3, 1} if size == 4 else {0, 7, 5})
        assert all(flat_split(c)[2] - flat_split(c)[0] - flat_split(c)[1] * (16 // size) > 0 for c in flat if c["in_offset"] == 1)   # (a tail)
        assert {(c["in_pitch"], c["out_pitch"], c["inplace"]) for c in pitched} == {(35, 35, False), (36, 35, False), (35, 40, False), (40, 40, True),
                                                                                     (36, 36, True)}
    for c in LARGE:
        assert not c["inplace"] or (c["in_pitch"], c["in_offset"]) == (c["out_pitch"], c["out_offset"])
    values = EJ.large_content(4001, 1)
    kind = (np.arange(4001) + 1) % 4
    assert (values[kind == 0] == EJ.LOW).all() and (values[kind == 1] == EJ.HIGH).all() and ((values >= EJ.LOW) & (values <= EJ.HIGH)).all()
    assert not (values[kind >= 2][:, list(EJ.COURT)] == EJ.WIDTH // 2).any()
    assert all(len(set(row - EJ.LOW)) >= 12 for row in values[kind >= 2][:64])              # (a row's columns differ)
    assert (EJ.bf16_to_f32(EJ.encode(values, 4)) > 256).sum() >= 5 * 1000
    assert EJ.LARGE_ACTION_COUNT % 2 == 1 and 2 * STRIDE < EJ.LARGE_ACTION_COUNT < 3 * STRIDE
    for dtype in EJ.ACTION_DTYPES:
        behind = EJ.action_case(dtype, EJ.LARGE_ACTION_COUNT)[2 * STRIDE:]
        assert set(behind.tolist()) == set(EJ.action_values(dtype).tolist())               # (every value on the third trip too)


@pytest.mark.parametrize("mutant", EJ.MUTANTS)
def test_every_mutant_is_caught_by_the_gpu_tests_cases(mutant):
    caught = [i for i, case in enumerate(CASES) if case["rows"] <= 9
              and not np.array_equal(EJ.expected_buffer(case), EJ.expected_buffer(case, mutant))]
    formats = sorted({CASES[i]["fmt"] for i in caught})
    print(mutant, "caught by", len(caught), "cases of formats", formats)
    assert caught, mutant
    if mutant == "truncation for RNE":
        assert formats == [4, 5, 6]       # (float16 raw is exact; bfloat16 raw rounds 432 - v above 256)
    elif mutant == "c_26 = 1":
        assert formats == [1, 5, 6]
    else:
        assert formats == list(EJ.FORMATS)


# ---- the three index walks of pz_ego.hip past one grid stride ----------------------------------------------------------------------
# WHY A SECOND TABLE.  Every case of row_cases() and every count of ACTION_COUNTS is done in ONE trip of the kernels' grid-stride
# loops (held below), so `col = wrap(col + step)`, the (row_step, col_step, carry) walk and the stride itself run in none of
# them.  The model below restates blocks_for and the three walks over whole thread arrays, with the cap read from the source, and
# holds LARGE_CASES to what they are there for: two trips for every thread, a third for some, the last trip partial.
WALK_MUTANTS = ("flat: col not advanced", "flat: step from the stride without V", "pitched: carry dropped", "pitched: col_step dropped")


def is_flat(case):
    """launch_rows' choice: rows back to back and both bases of one phase within 16 bytes (the GPU test's buffers are 256-byte
    aligned and the guard is a multiple of 16 bytes)"""
    size = EJ.STORAGE[case["fmt"]]().itemsize
    assert (EJ.GUARD * size) % 16 == 0
    return case["in_pitch"] == case["out_pitch"] == EJ.DIM and ((case["in_offset"] - case["out_offset"]) * size) % 16 == 0


def blocks_for(threads):
    return min(max(-(-threads // K_THREADS), 1), K_MAX_BLOCKS)


def flat_split(case):
    """launch_rows: (head, vectors, total)"""
    size = EJ.STORAGE[case["fmt"]]().itemsize
    total = case["rows"] * EJ.DIM
    head = min(((16 - (case["in_offset"] * size) % 16) & 15) // size, total)
    return head, (total - head) // (16 // size), total


def wrap(col):
    return np.where(col >= EJ.DIM, col - EJ.DIM, col)


def flat_walk(case, mutant=None):
    """rows_flat_kernel: (the column the walk holds for every element, how often the element is done, the trips of every thread)"""
    V = 16 // EJ.STORAGE[case["fmt"]]().itemsize
    head, vectors, total = flat_split(case)
    stride = blocks_for(max(vectors, 2 * V)) * K_THREADS
    gid = np.arange(stride, dtype=np.int64)
    body_end = head + vectors * V
    cols, times, trips = np.full(total, -1, np.int64), np.zeros(total, np.int64), np.zeros(stride, np.int64)
    edge = gid[gid < head + (total - body_end)]
    e = np.where(edge < head, edge, body_end + (edge - head))
    cols[e] = e % EJ.DIM
    times[e] += 1
    v = gid[gid < vectors]
    mine = v.copy()
    col = (head + v * V) % EJ.DIM
    step = (stride % EJ.DIM) if mutant == "flat: step from the stride without V" else (stride * V) % EJ.DIM
    while (v < vectors).any():
        on = v < vectors
        for i in range(V):
            at = head + v[on] * V + i
            cols[at] = wrap(col[on] + i)
            times[at] += 1                     # (a trip's elements are distinct)
        trips[mine[on]] += 1
        v = v + stride
        if mutant != "flat: col not advanced":
            col = wrap(col + step)
    return cols, times, trips


def pitched_walk(case, mutant=None):
    """rows_pitched_kernel: the same three"""
    rows, total = case["rows"], case["rows"] * EJ.DIM
    stride = blocks_for(total) * K_THREADS
    gid = np.arange(stride, dtype=np.int64)
    row = gid // EJ.DIM
    col = gid - row * EJ.DIM
    row_step = stride // EJ.DIM
    col_step = stride - row_step * EJ.DIM
    cols, times, trips = np.full(total, -1, np.int64), np.zeros(total, np.int64), np.zeros(stride, np.int64)
    while (row < rows).any():
        on = row < rows
        at = row[on] * EJ.DIM + col[on]
        assert len(np.unique(at)) == len(at)
        cols[at] = col[on]
        times[at] += 1
        trips[on] += 1
        row = row + row_step
        if mutant != "pitched: col_step dropped":
            col = col + col_step
        carry = col >= EJ.DIM
        col = np.where(carry, col - EJ.DIM, col)
        if mutant != "pitched: carry dropped":
            row = row + carry
    return cols, times, trips


_walks, _large_walks = {}, {}


def walk_key(case, mutant=None):
    """what a walk depends on: the kernel, and for the flat one the element size and the head"""
    flat = is_flat(case)
    if mutant is not None and mutant.startswith("flat") != flat:
        mutant = None                          # (a mutant of the other kernel)
    return (flat, EJ.STORAGE[case["fmt"]]().itemsize if flat else 0, case["rows"], flat_split(case)[0] if flat else 0, mutant)


def walk(case, mutant=None):
    """the walk of a case's launch under `mutant`, made once per key (of the large ones the last six are kept)"""
    key = walk_key(case, mutant)
    held = _large_walks if case.get("large") else _walks
    if key not in held:
        if case.get("large") and len(held) >= 6:
            del held[next(iter(held))]
        cols, times, trips = (flat_walk if key[0] else pitched_walk)(case, key[4])
        held[key] = (cols.astype(np.int8), times.astype(np.int8), trips)
    return held[key]


def by_size(cases):
    """the cases in an order that makes every large row set once"""
    return sorted(cases, key=lambda c: (c["fmt"], c["rows"], c["seed"]))


def test_the_constants_of_the_walk_are_the_sources():
    assert (K_THREADS, K_MAX_BLOCKS, STRIDE) == (256, 2048, 524288), "the cap moved: check that LARGE_CASES still pass two trips (the tests below say)"
    assert "blocks > kMaxBlocks ? kMaxBlocks : blocks" in SOURCE and "(threads + kThreads - 1) / kThreads" in SOURCE
    assert "const int step = (int)((stride * V) % kDim);" in SOURCE and "const int64_t row_step = stride / kDim;" in SOURCE


def test_the_element_by_element_mirror_is_the_judges():
    for fmt in EJ.FORMATS:
        stored = EJ.encode(EJ.large_content(403, 3), fmt)
        cols = np.tile(np.arange(EJ.DIM), (403, 1))
        assert np.array_equal(EJ.bits(EJ.mirror_elements(stored, cols, fmt)), EJ.bits(EJ.mirror(stored, fmt))), fmt
        assert np.array_equal(EJ.bits(EJ.mirror_elements(stored, np.full_like(cols, 1), fmt)), EJ.bits(stored)), fmt
        moved = EJ.bits(EJ.mirror_elements(stored, (cols + 22) % EJ.DIM, fmt)) != EJ.bits(EJ.mirror(stored, fmt))
        kind = np.array([(3 if j == 26 and fmt in EJ.NORMALISED else 1) if j in EJ.COURT else 2 if j in EJ.SIGN else 0 for j in range(EJ.DIM)])
        differs = kind != kind[(np.arange(EJ.DIM) + 22) % EJ.DIM]
        assert np.array_equal(moved.any(axis=0), differs) and differs.sum() >= 10, fmt   # a mirror in a column of another kind shows


def test_every_walk_does_every_element_once_in_its_column_and_only_the_large_cases_stride():
    seen = set()
    for case in CASES + by_size(LARGE):
        if walk_key(case) in seen:
            continue
        seen.add(walk_key(case))
        cols, times, trips = walk(case)
        assert (times == 1).all() and np.array_equal(cols, np.arange(len(cols)) % EJ.DIM), case
        if case.get("large"):
            assert len(trips) == STRIDE and trips.min() >= 2 and trips.max() >= 3, (case, trips.min(), trips.max())
            assert 0 < (trips == trips.max()).sum() < STRIDE, case                     # the last trip is partial
        else:
            # no case of the first table takes a thread round its loop: the reason the second table exists
            assert trips.max() == 1 and len(trips) < STRIDE, (case, trips.max())
    print({("flat" if is_flat(c) else "pitched", c["rows"]): np.bincount(walk(c)[2]).tolist() for c in LARGE if c["fmt"] in (0, 2)})
    for n in EJ.ACTION_COUNTS:
        assert n <= blocks_for(n) * K_THREADS < STRIDE
    assert blocks_for(EJ.LARGE_ACTION_COUNT) * K_THREADS == STRIDE and 2 * STRIDE < EJ.LARGE_ACTION_COUNT < 3 * STRIDE


@pytest.mark.parametrize("mutant", WALK_MUTANTS)
def test_every_mutant_of_the_walks_is_caught_by_the_large_cases_and_by_no_other(mutant):
    """each mutant as the buffer it would leave: the flat ones mirror in wrong columns from the second trip on; the pitched ones
    do elements twice -- they skip none: trip t of either does rows [t * row_step, (t + 1) * row_step) whole and a part of row
    (t + 1) * row_step, which trip t + 1 does again"""
    for case in CASES:
        for got, want in zip(walk(case, mutant), walk(case)):
            assert np.array_equal(got, want), (mutant, case)                           # one trip: the walk is the unmutated one
    for case in [c for c in CASES if c["fmt"] in (1, 6) and c["rows"] in (9, 257)]:
        cols, times, _ = walk(case, mutant)
        assert np.array_equal(EJ.walked_buffer(case, cols, times), EJ.expected_buffer(case)), (mutant, case)
    caught, missed = [], []
    for case in by_size(LARGE):
        if mutant.startswith("flat") != is_flat(case):
            continue
        cols, times, _ = walk(case, mutant)
        buffers = EJ.case_buffers(case)
        same = np.array_equal(EJ.walked_buffer(case, cols, times, buffers), EJ.expected_buffer(case, buffers=buffers))
        (missed if same else caught).append(case)
    print(mutant, "caught by", len(caught), "large cases, missed by", len(missed))
    if mutant.startswith("flat"):
        assert len(caught) == 4 * len(EJ.FORMATS) and not missed            # every flat case of every format
        return
    # Out of place an element done twice is stored twice with the same value: nothing shows.  In place the second visit reads
    # what the first one stored, and the element is mirrored back (exactly in the integer formats and raw float16; elsewhere
    # the mirror of the mirror, which differs from the mirror all the same).  So ONLY the in-place cases can catch a pitched
    # mutant -- and they do so on the device only where the second visit comes after the first one's store: the two visits are
    # by different workgroups (the grid's first and its last), which this model runs one after the other (on the MI355X both
    # mutants, built locally, failed the (40, 40) in-place case in every format, in the doubled elements of both rows).
    assert caught and all(c["inplace"] for c in caught) and all(not c["inplace"] for c in missed)
    assert {c["fmt"] for c in caught} == set(EJ.FORMATS) and len(caught) == 2 * len(EJ.FORMATS)
    assert (walk(caught[0], mutant)[1] >= 1).all() and (walk(caught[0], mutant)[1] == 2).sum() >= 2 * 23   # none skipped; 23 per later trip


def test_an_actions_loop_of_one_trip_is_caught_by_the_large_count_and_by_no_other():
    for dtype in EJ.ACTION_DTYPES:
        for n in EJ.ACTION_COUNTS + (EJ.LARGE_ACTION_COUNT,):
            a = EJ.action_case(dtype, n)
            done = np.arange(n) < blocks_for(n) * K_THREADS
            for before in (a, np.full(n, 99, dtype)):                   # in place; out of place
                left = np.where(done, EJ.mirror_actions(a), before)
                assert np.array_equal(left, EJ.mirror_actions(a)) == (n != EJ.LARGE_ACTION_COUNT), (dtype, n)


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_ego_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, ego

    assert header_functions("pikazoo_ego.h") == NAMES == sorted(ego.SIGNATURES) == dynamic_pz_symbols(pz_build.EGO_LIB)
    assert pz_build.library_id(pz_build.EGO_LIB) == pz_build.source_id() == lib.pz_ego_build_id().decode()
    assert not pz_build.needs_build()
    # the fourteenth library, through a tuple of its own: TARGETS and ALL_TARGETS are what they were
    assert len(pz_build.TARGETS) == 11 and len(pz_build.ALL_TARGETS) == 13 and pz_build.ALL_TARGETS[:11] == pz_build.TARGETS
    assert pz_build.BUILD_TARGETS[:13] == pz_build.ALL_TARGETS and len(pz_build.BUILD_TARGETS) == 14
    assert pz_build.BUILD_TARGETS[13] == (pz_build.EGO_LIB, pz_build.EGO_SOURCES)
    assert pz_build.EGO_LIB.name == "libpikazoo_ego.so" and pz_build.EGO_SOURCES == [pz_build.CSRC / "pz_ego.hip"]
    assert pz_build.EGO_SOURCES[0] in pz_build.DEPS and (pz_build.INCLUDE / "pikazoo_ego.h") in pz_build.DEPS
    for lib_path, _ in pz_build.BUILD_TARGETS:
        assert pz_build.library_id(lib_path) == pz_build.source_id(), lib_path
    assert lib.pz_ego_abi_version() == ego.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_ego.h").read_text()
    assert "#define PZ_EGO_ABI_VERSION 1" in header and "#define PZ_E_EGO_OVERLAP (-5)" in header
    for other, _ in pz_build.ALL_TARGETS:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names())
    doc = (REPO / "INTEGRATION.md").read_text()
    assert "pikazoo_ego.h" in doc and "libpikazoo_ego.so" in doc and "pz_ego_rows" in doc and "pz_ego_actions" in doc
    assert lib.pz_ego_error_string(0) is None and lib.pz_ego_error_string(700) == b"HIP error"
    texts = {lib.pz_ego_error_string(code) for code in (-1, -2, -3, -4, -5)}
    assert len(texts) == 5 and None not in texts and b"overlap" in lib.pz_ego_error_string(-5)
    assert set(ego._ERRORS) == {-1, -2, -3, -4, -5}


def test_importing_the_older_modules_does_not_load_the_ego_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, wrappers, learn, policy, ppo, net, netgrad, optim, batch, pool, league, act, pool_act; "
            "assert 'pikazoo_amd.ego' not in sys.modules; wrappers.EgocentricObservation; assert 'pikazoo_amd.ego' not in sys.modules; "
            "import pikazoo_amd as p; assert 'ego' in p.__all__ and 'EgocentricObservation' in wrappers.__all__; "
            "p.ego.mirror; assert 'pikazoo_amd.ego' in sys.modules and p.ego._lib is None; "
            "assert not any('libpikazoo_ego' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_ego_library(pz_build):
    """a flat and a pitched kernel per row format and an action kernel per action type: 18 kernels and nothing else; none uses
    scratch, spills a register or holds LDS; the flat kernels move 16 bytes per access"""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.EGO_LIB)
    names = sorted(name for name in table if not name.endswith(".kd"))
    want = sorted([f"pz_ego::rows_{kind}_kernel<{f}>" for kind in ("flat", "pitched") for f in range(7)]
                  + [f"pz_ego::actions_kernel<{t}>" for t in ("int", "long", "unsigned char", "short")])
    assert [n.replace("void ", "") for n in names] == want, names
    notes = kernel_notes.notes(pz_build.EGO_LIB)
    assert len(notes) == 18
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0 and row[".sgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0 and row[".vgpr_count"] <= 64, (name, row)
        print(name.split("(")[0], {k: row[k] for k in (".vgpr_count", ".sgpr_count")})


def test_argument_validation(lib):
    """every return code that needs no launch, on fake pointers, in the header's order: NULL, size, config, alignment; a call
    that passes them all has rows = 0 and launches nothing"""
    def rows(in_=FAKE, out=2 * FAKE, fmt=0, n=0, ip=35, op=35):
        return lib.pz_ego_rows(in_, out, fmt, n, ip, op, None)

    assert rows() == 0 and rows(None, None) == 0 and rows(ip=36, op=1 << 40) == 0
    assert all(rows(fmt=f) == 0 for f in range(7))
    assert rows(None, n=1) == -1 and rows(out=None, n=1) == -1
    assert rows(n=-1) == -2 and rows(ip=34) == -2 and rows(op=34) == -2 and rows(op=0) == -2 and rows(ip=-35) == -2
    assert rows(n=1 << 40, ip=1 << 22) == -2 and rows(n=1 << 40, op=1 << 22) == -2 and rows(n=1 << 61) == -2
    assert rows(fmt=7) == -3 and rows(fmt=-1) == -3
    for f, step in ((0, 2), (1, 2), (0, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1)):
        assert rows(FAKE + step, fmt=f) == -4 and rows(out=FAKE + step, fmt=f) == -4, (f, step)
    for f in (2, 3, 4, 5, 6):
        assert rows(FAKE + 2, 2 * FAKE + 6, fmt=f) == 0
    assert rows(FAKE + 4, 2 * FAKE + 12, fmt=1) == 0
    # the order
    assert rows(None, FAKE + 1, fmt=9, n=1, ip=3) == -1
    assert rows(FAKE + 1, FAKE + 1, fmt=9, n=1, ip=3) == -2
    assert rows(FAKE + 1, FAKE + 1, fmt=9) == -3
    assert rows(FAKE + 1, FAKE + 1) == -4

    def actions(in_=FAKE, out=2 * FAKE, fmt=0, n=0):
        return lib.pz_ego_actions(in_, out, fmt, n, None)

    assert actions() == 0 and actions(None, None) == 0 and all(actions(fmt=f) == 0 for f in range(4))
    assert actions(None, n=1) == -1 and actions(out=None, n=1) == -1
    assert actions(n=-1) == -2 and actions(n=1 << 61) == -2
    assert actions(fmt=4) == -3 and actions(fmt=-1) == -3
    assert actions(FAKE + 2) == -4 and actions(FAKE + 4, fmt=1) == -4 and actions(FAKE + 1, fmt=3) == -4 and actions(out=FAKE + 1, fmt=3) == -4
    assert actions(FAKE + 1, FAKE + 3, fmt=2) == 0 and actions(FAKE + 2, fmt=3) == 0 and actions(FAKE + 4) == 0
    assert actions(None, FAKE + 1, fmt=9, n=-1) == -2 and actions(None, FAKE + 1, fmt=9, n=1) == -1
    assert actions(FAKE + 1, FAKE + 1, fmt=9, n=-1) == -2 and actions(FAKE + 1, FAKE + 1, fmt=9) == -3 and actions(FAKE + 1, FAKE + 1) == -4


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    import torch

    from pikazoo_amd import ego

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(ego, "load", refuse)
    x = torch.zeros(8, 35)
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror(x)
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror(torch.zeros(3, 8, 35, dtype=torch.float16), normalized=True, out=torch.zeros(4, 8, 40, dtype=torch.float16)[1:, :, :35])
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror(x, out=x)
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror(torch.zeros(8, 35, dtype=torch.int16)[1:], normalized=False, out=torch.zeros(2, 7, 35, dtype=torch.int16)[1])
    wide = torch.zeros(8, 70)
    slab = torch.zeros(3, 8, 35)
    bad = [
        dict(rows=torch.zeros(8, 34)), dict(rows=torch.zeros(35, 8).t()), dict(rows=torch.zeros(8, 35, dtype=torch.float64)),
        dict(rows=torch.zeros(8, 35, dtype=torch.int64)), dict(rows=np.zeros((8, 35), np.float32)), dict(rows=torch.zeros(())),
        dict(rows=slab[:, ::2]), dict(rows=slab.transpose(0, 1)), dict(rows=wide[:, ::2]), dict(rows=torch.zeros(35).expand(8, 35)),
        dict(normalized=False), dict(normalized=1), dict(rows=torch.zeros(8, 35, dtype=torch.int32), normalized=True),
        dict(rows=torch.zeros(8, 35, dtype=torch.float16)), dict(rows=torch.zeros(8, 35, dtype=torch.bfloat16)),
        dict(out=torch.zeros(8, 35, dtype=torch.float16)), dict(out=torch.zeros(9, 35)), dict(out=torch.zeros(8, 36)), dict(out=slab.transpose(0, 1)[:, 0]),
        dict(out="rows"), dict(rows=wide[:, :35], out=wide[:, 35:]), dict(rows=wide[:, :35], out=wide[:, 1:36]), dict(rows=slab[0], out=slab[:2].view(-1)[35:35 * 9].view(8, 35)),
        dict(rows=wide[:, :35], out=wide.view(-1)[:8 * 35].view(8, 35)),
    ]
    for i, over in enumerate(bad):
        args = dict(rows=x)
        args.update(over)
        with pytest.raises(ValueError):
            ego.mirror(**args)
            pytest.fail(f"bad call {i} was accepted: {sorted(over)}")
    a = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror_actions(a)
    with pytest.raises(ValueError, match="GPU"):
        ego.mirror_actions(a, out=a)
    two = torch.zeros(16, dtype=torch.int64)
    for i, over in enumerate([dict(actions=torch.zeros(8)), dict(actions=torch.zeros(8, dtype=torch.int8)), dict(actions=two[::2]), dict(actions=[1, 2]),
                              dict(out=torch.zeros(8, dtype=torch.int32)), dict(out=torch.zeros(9, dtype=torch.int64)), dict(out=two[::2]),
                              dict(actions=two[:8], out=two[4:12]), dict(out=3)]):
        args = dict(actions=a)
        args.update(over)
        with pytest.raises(ValueError):
            ego.mirror_actions(**args)
            pytest.fail(f"bad action call {i} was accepted: {sorted(over)}")
    assert ego.row_format(torch.float32) == 1 == ego.row_format(torch.float32, True) and ego.row_format(torch.int16) == 2
    assert [ego.row_format(torch.float16, n) for n in (False, True)] == [3, 5] and [ego.row_format(torch.bfloat16, n) for n in (False, True)] == [4, 6]
