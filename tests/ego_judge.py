"""The judge of the egocentric rows: include/pikazoo_ego.h's definition in numpy, bit for bit in all seven row formats, the
involution ``PI`` of the 18 actions, the mutants of the definition that the tests must tell from it, and the case lists of the
GPU test (tests/test_gpu_ego.py), which the host test (tests/test_ego_host.py) plays the mutants on.

Two case tables.  ``row_cases()`` holds what a launch can get wrong within ONE trip of the kernels' grid-stride loops: its
largest case is 257 rows, 8 995 elements, and a thread takes a second trip only above 524 288.  ``LARGE_CASES`` (and
``LARGE_ACTION_COUNT``) are about 2.5 strides each, so that the advance of the column, the (row, column) walk with its carry
and the stride itself run; ``mirror_elements`` and ``walked_buffer`` say what a walk that holds wrong columns, or does
elements twice or not at all, would leave.

Rows are numpy arrays ``[..., 35]`` in the storage type of their format: int32 (0), float32 (1), int16 (2), float16 (3, 5) and,
numpy having no bfloat16, uint16 holding the bfloat16 bits (4, 6).  bfloat16 is done in uint16 / uint32 bit arithmetic with
round to nearest even."""
import numpy as np

DIM = 35
FORMATS = {0: "int32", 1: "float32 normalised", 2: "int16", 3: "float16", 4: "bfloat16", 5: "float16 normalised", 6: "bfloat16 normalised"}
STORAGE = {0: np.int32, 1: np.float32, 2: np.int16, 3: np.float16, 4: np.uint16, 5: np.float16, 6: np.uint16}
NORMALISED = (1, 5, 6)
COURT = (0, 13, 26, 28, 30)   # M = 432
SIGN = (3, 16, 32)            # M = 0
WIDTH = 432
C26 = np.float32(float.fromhex("0x1.e72548p-1"))
PI = (0, 1, 2, 4, 3, 5, 7, 6, 9, 8, 10, 12, 11, 13, 15, 14, 17, 16)

# the bounds of a row (pikazoo_env.py:485-562): player, opponent, ball
_PLAYER_LOW = [32, 108, -15, -1, -2, 0, 0, 0, 0, 0, 0, 0, 0]
_PLAYER_HIGH = [400, 244, 16, 1, 3, 4, 4, 1, 1, 1, 1, 1, 1]
LOW = np.array(_PLAYER_LOW * 2 + [20, 0, 0, 0, 0, 0, -20, -124, 0], np.int64)
HIGH = np.array(_PLAYER_HIGH * 2 + [432, 252, 432, 252, 432, 252, 20, 124, 1], np.int64)

MUTANTS = ("column 27 for 26", "opponent block at 12", "M = 431", "c_26 = 1", "x velocity not negated", "truncation for RNE",
           "mirror applied twice", "padding written")


# ---- the number formats ------------------------------------------------------------------------------------------------------------
def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x, truncate=False):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if truncate:
        return (u >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rounded = (u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32)).astype(np.uint16)


def f32_to_f16(x, truncate=False):
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    if truncate:  # toward zero: step back where the rounding went away from zero
        away = np.abs(h.astype(np.float32)) > np.abs(x)
        h = np.where(away, np.nextafter(h, np.float16(0)), h)
    return h


def widen(stored, fmt):
    """the stored elements as float32 (exact)"""
    if fmt == 1:
        return np.asarray(stored, np.float32)
    if fmt in (3, 5):
        return np.asarray(stored, np.float16).astype(np.float32)
    return bf16_to_f32(stored)


def narrow(x, fmt, truncate=False):
    if fmt == 1:
        return np.asarray(x, np.float32)
    if fmt in (3, 5):
        return f32_to_f16(x, truncate)
    return f32_to_bf16(x, truncate)


def bits(a):
    """any row array as unsigned integers of its element size: what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def mirror(rows, fmt, mutant=None):
    """include/pikazoo_ego.h on ``[..., 35]`` rows of format `fmt` in their storage type; `mutant`: one of MUTANTS (``padding
    written`` is a mutant of the buffer, see :func:`expected_buffer`)"""
    rows = np.asarray(rows)
    assert rows.dtype == STORAGE[fmt] and rows.shape[-1] == DIM, (rows.dtype, rows.shape, fmt)
    if mutant == "mirror applied twice":
        return mirror(mirror(rows, fmt), fmt)
    court, sign = list(COURT), list(SIGN)
    if mutant == "column 27 for 26":
        court[2] = 27
    if mutant == "opponent block at 12":
        court[1], sign[1] = 12, 15
    if mutant == "x velocity not negated":
        sign.remove(32)
    M = 431 if mutant == "M = 431" else WIDTH
    out = rows.copy()
    if fmt in (0, 2):
        wide = rows.astype(np.int64)
        for j in court:
            out[..., j] = (M - wide[..., j]).astype(rows.dtype)
        for j in sign:
            out[..., j] = (0 - wide[..., j]).astype(rows.dtype)
        return out
    wide = widen(rows, fmt)
    cut = mutant == "truncation for RNE"
    for j in court + sign:
        if fmt in NORMALISED:
            c = C26 if (j == 26 and mutant != "c_26 = 1") else np.float32(1.0)
            if mutant == "M = 431" and j in court:  # c_j = (431 - 2 low) / (high - low)
                c = np.float32((431 - 2 * LOW[j]) / (HIGH[j] - LOW[j]))
        else:
            c = np.float32(M if j in court else 0)
        out[..., j] = narrow(c - wide[..., j], fmt, cut)   # one float32 subtraction
    return out


def mirror_actions(a):
    a = np.asarray(a)
    table = np.array(PI, np.int64)
    inside = (a >= 0) & (a < 18)
    return np.where(inside, table[np.where(inside, a, 0).astype(np.int64)], a).astype(a.dtype)


# ---- rows of the env's making ----------------------------------------------------------------------------------------------------
def encode(values, fmt):
    """integer rows (inside or outside the bounds) as the env stores them in format `fmt`"""
    v = np.asarray(values, np.int64)
    if fmt == 0:
        return v.astype(np.int32)
    if fmt == 2:
        return v.astype(np.int16)
    if fmt == 3:
        return v.astype(np.float32).astype(np.float16)
    if fmt == 4:
        return f32_to_bf16(v.astype(np.float32))
    s = (v - LOW).astype(np.float32) / (HIGH - LOW).astype(np.float32)   # the IEEE float32 quotient
    return narrow(s, fmt)


def content(rows, seed):
    """integer rows for a case: by turns every column at its low bound, at its high bound, at an interior value and at a value
    of its own per column; the high rows put 400 and 432 -- above 256 -- into the bfloat16 formats"""
    rng = np.random.default_rng([rows, seed])
    out = np.empty((rows, DIM), np.int64)
    for r in range(rows):
        kind = (r + seed) % 4
        if kind == 0:
            out[r] = LOW
        elif kind == 1:
            out[r] = HIGH
        elif kind == 2:
            out[r] = rng.integers(LOW, HIGH + 1)
        else:
            out[r] = LOW + (np.arange(DIM) * 7 + 3 + r) % (HIGH - LOW + 1)
    return out


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------------
ROWS = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257)
GUARD = 64          # sentinel elements in front of and behind each buffer
SENTINEL = 0x7B7B   # (finite in float16 and bfloat16; no value of a row)
# (in_pitch, out_pitch, in_offset, out_offset, in place): offsets in elements from a 256-byte aligned base
LAYOUTS = (
    (35, 35, 0, 0, False), (35, 35, 0, 0, True),          # the flat path, aligned
    (35, 35, 35, 35, False), (35, 35, 35, 35, True),      # a view from row 1: 140 / 70 bytes in, a head and a tail
    (35, 35, 1, 1, False), (35, 35, 1, 1, True),          # one element in: aligned to the element only
    (35, 35, 1, 0, False), (35, 35, 0, 35, False), (35, 35, 2, 1, False),   # bases of different phase: element by element
    (36, 35, 0, 0, False), (35, 36, 0, 0, False), (35, 40, 0, 0, False), (40, 35, 0, 0, False), (36, 40, 0, 0, False), (40, 36, 1, 35, False),
    (36, 36, 0, 0, True), (40, 40, 35, 35, True), (40, 40, 1, 1, False),
)


def row_cases():
    """every case of pz_ego_rows in the GPU test: 7 formats x 11 row counts x 18 layouts, and a [3, 65, 35] slab per format"""
    cases = []
    for fmt in FORMATS:
        for rows in ROWS:
            for index, (ip, op, ioff, ooff, inplace) in enumerate(LAYOUTS):
                cases.append(dict(fmt=fmt, rows=rows, in_pitch=ip, out_pitch=op, in_offset=ioff, out_offset=ooff, inplace=inplace, seed=index))
        cases.append(dict(fmt=fmt, rows=3 * 65, in_pitch=35, out_pitch=35, in_offset=0, out_offset=0, inplace=False, seed=1))
    return cases


def _sentinel(count, fmt):
    word = SENTINEL | (SENTINEL << 16) if STORAGE[fmt]().itemsize == 4 else SENTINEL
    return np.full(count, word, bits(np.zeros(1, STORAGE[fmt])).dtype)


def _rows_of(buffer, at, rows, pitch):
    """the [rows, pitch] view of a buffer's rows from element `at` (every buffer ends GUARD elements behind rows * pitch)"""
    return buffer[at:at + rows * pitch].reshape(rows, pitch)


def case_rows(case):
    """the rows of a case in their storage type (a large case: shared and read-only, see :func:`large_rows`)"""
    if case.get("large"):
        return large_rows(case["fmt"], case["rows"], case["seed"])[0]
    return encode(content(case["rows"], case["seed"]), case["fmt"])


def case_buffers(case):
    """(input buffer, output buffer or None when in place, the rows) as unsigned words: sentinels everywhere but in the rows'
    35 columns of the input"""
    fmt, rows = case["fmt"], case["rows"]
    stored = case_rows(case)
    src = _sentinel(GUARD + case["in_offset"] + rows * case["in_pitch"] + GUARD, fmt)
    _rows_of(src, GUARD + case["in_offset"], rows, case["in_pitch"])[:, :DIM] = bits(stored)
    dst = None if case["inplace"] else _sentinel(GUARD + case["out_offset"] + rows * case["out_pitch"] + GUARD, fmt)
    return src, dst, stored


def expected_buffer(case, mutant=None, buffers=None):
    """the output buffer (the input buffer, in place) after the call: the judge's rows in the 35 columns, everything else as it
    was; `buffers`: what :func:`case_buffers` returned for the case, where the caller holds it already (it is not written)"""
    src, dst, stored = case_buffers(case) if buffers is None else buffers
    if case.get("large") and mutant in (None, "padding written"):
        want = large_rows(case["fmt"], case["rows"], case["seed"])[1]
    else:
        want = mirror(stored, case["fmt"], None if mutant == "padding written" else mutant)
    out = src.copy() if dst is None else dst.copy()
    pitch = case["in_pitch"] if dst is None else case["out_pitch"]
    view = _rows_of(out, GUARD + (case["in_offset"] if dst is None else case["out_offset"]), case["rows"], pitch)
    view[:, :DIM] = bits(want)
    if mutant == "padding written":
        view[:-1, DIM:] = 0
    return out


# ---- the cases past one grid stride ----------------------------------------------------------------------------------------------
# pz_ego.hip caps a launch at 2 048 workgroups of 256 threads and strides: a thread takes a second trip of its loop only above
# 524 288 elements (element by element) or 524 288 16-byte pieces (flat).  No case above comes near (257 rows are 8 995
# elements), so the advance of the column, the (row, column) walk with its carry and the stride itself run in no case of
# row_cases().  These do: about 2.5 strides each, so every thread takes two trips and about half of them a third
# (tests/test_ego_host.py proves that on a numpy model of the three walks, with the cap read from the source).
# by path; the flat path by the format's element size (150 003 and not 150 001: behind a head of 3 elements the latter's rest
# is a whole number of 16-byte pieces, and the layout that is one element in would have no tail)
LARGE_ROWS = {"pitched": 37501, 4: 150003, 2: 300001}
LARGE_FLAT = (
    (35, 35, 0, 0, False), (35, 35, 0, 0, True),          # aligned
    (35, 35, 1, 1, False),                                # one element in: a head of 3 or 7 elements, the column starts from it
    (35, 35, 35, 35, True),                               # a view from row 1
)
LARGE_PITCHED = (
    (35, 35, 1, 0, False),                                # back to back, bases of different phase
    (36, 35, 0, 0, False), (35, 40, 0, 0, False),
    (40, 40, 1, 1, True), (36, 36, 0, 0, True),           # in place: the only calls in which an element done twice can show
)
LARGE_ACTION_COUNT = 1312537                              # odd; about 2.5 strides of one element


def large_content(rows, seed):
    """:func:`content` without its loop over the rows: by turns a row at the low bounds, at the high bounds, at random and at a
    value of its own per column -- and no court column of the last two kinds at 216, the value the mirror leaves where it is
    (432 - 216; in the normalised formats c_j - s = s there too), so that a mirror done in the wrong column or not at all shows"""
    rng = np.random.default_rng([rows, seed, 1])
    r = np.arange(rows)[:, None]
    kind = (r + seed) % 4
    own = LOW + (np.arange(DIM)[None, :] * 7 + 3 + r) % (HIGH - LOW + 1)
    out = np.where(kind == 0, LOW, np.where(kind == 1, HIGH, np.where(kind == 2, rng.integers(LOW, HIGH + 1, (rows, DIM)), own)))
    court = list(COURT)
    out[:, court] = np.where(out[:, court] == WIDTH // 2, WIDTH // 2 + 1, out[:, court])
    return out


_large, _large_values = {}, {}


def large_rows(fmt, rows, seed):
    """(the rows of a large case in format `fmt`, the judge's mirror of them): computed once per (format, rows, seed), shared by
    the cases and the tests that need them, read-only; the rows of one (format, rows) are held at a time"""
    key = (fmt, rows, seed)
    if key not in _large:
        _large.clear()
        if (rows, seed) not in _large_values:            # (the integer rows are those of every format)
            if len(_large_values) >= 3:
                _large_values.clear()
            _large_values[rows, seed] = large_content(rows, seed)
        stored = encode(_large_values[rows, seed], fmt)
        want = mirror(stored, fmt)
        stored.setflags(write=False)
        want.setflags(write=False)
        _large[key] = (stored, want)
    return _large[key]


def large_cases():
    """the cases of pz_ego_rows past one grid stride: 7 formats x (4 flat + 5 element-by-element layouts); one content per path"""
    cases = []
    for fmt in FORMATS:
        size = STORAGE[fmt]().itemsize
        for layouts, rows, seed in ((LARGE_FLAT, LARGE_ROWS[size], 1), (LARGE_PITCHED, LARGE_ROWS["pitched"], 2)):
            for ip, op, ioff, ooff, inplace in layouts:
                cases.append(dict(fmt=fmt, rows=rows, in_pitch=ip, out_pitch=op, in_offset=ioff, out_offset=ooff, inplace=inplace, seed=seed,
                                  large=True))
    return cases


LARGE_CASES = large_cases()


def mirror_elements(values, cols, fmt):
    """the mirror element by element: `values` (any shape, the format's storage type) each done as an element of column
    `cols` (same shape).  With ``cols = index mod 35`` this is :func:`mirror` (tests/test_ego_host.py holds the two to each
    other); with the column a mutated walk holds, what that walk stores."""
    values, cols = np.asarray(values), np.asarray(cols)
    assert values.dtype == STORAGE[fmt] and values.shape == cols.shape
    is_court, is_sign = np.isin(np.arange(DIM), COURT), np.isin(np.arange(DIM), SIGN)
    shape, values, cols = values.shape, np.ascontiguousarray(values).reshape(-1), np.ascontiguousarray(cols).reshape(-1)
    out = values.copy()
    at = np.flatnonzero((is_court | is_sign)[cols])          # (8 columns of 35: the others are copied)
    v, j = values[at], cols[at]
    if fmt in (0, 2):
        out[at] = (np.where(is_court[j], WIDTH, 0) - v.astype(np.int64)).astype(values.dtype)
        return out.reshape(shape)
    if fmt in NORMALISED:
        c = np.where(j == 26, C26, np.float32(1.0)).astype(np.float32)
    else:
        c = np.where(is_court[j], np.float32(WIDTH), np.float32(0)).astype(np.float32)
    out[at] = narrow(c - widen(v, fmt), fmt)
    return out.reshape(shape)


def walked_buffer(case, cols, times, buffers=None):
    """the output buffer after a walk that does element e of the rows (row-major, 35 to a row) `times[e]` times, each time as an
    element of column `cols[e]`: an element never done keeps what the buffer held (the sentinel; in place the input), one done
    twice is, in place, the mirror of the mirror -- provided the second visit reads what the first one stored"""
    src, dst, stored = case_buffers(case) if buffers is None else buffers
    fmt, rows = case["fmt"], case["rows"]
    cols, times = np.asarray(cols).reshape(rows, DIM), np.asarray(times).reshape(rows, DIM)
    out = src.copy() if dst is None else dst.copy()
    pitch = case["in_pitch"] if dst is None else case["out_pitch"]
    view = _rows_of(out, GUARD + (case["in_offset"] if dst is None else case["out_offset"]), rows, pitch)
    once = mirror_elements(stored, cols, fmt)
    result = np.where(times >= 2, mirror_elements(once, cols, fmt), once) if dst is None else once
    view[:, :DIM] = np.where(times == 0, view[:, :DIM], bits(result))
    return out


ACTION_DTYPES = (np.int32, np.int64, np.uint8, np.int16)
ACTION_COUNTS = (1, 63, 64, 65, 257)


def action_values(dtype):
    """all 18 actions and the values outside them that `dtype` can hold"""
    extra = [v for v in (-1, 18, 255, (1 << 32) + 3) if np.iinfo(dtype).min <= v <= np.iinfo(dtype).max]
    return np.array(list(range(18)) + extra, dtype)


def action_case(dtype, n):
    values = action_values(dtype)
    return values[(np.arange(n) * 13 + n) % len(values)]
