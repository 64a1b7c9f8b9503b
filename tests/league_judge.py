"""The judge of the league library (include/pikazoo_league.h): the header's two definitions in numpy / Python integers -- the
weighted draw (Philox block, 64 x 36-bit product, prefix sums) and the tally of finished games -- so that every comparison is
bit for bit.  Each has a second, scalar formulation (``draw_scalar`` with a Philox of its own, ``tally_scalar`` as a plain
loop) that tests/test_league_host.py holds it to.  Also the case lists of tests/test_gpu_league.py and the mutants that the
host test shows those cases to catch.
"""
import itertools

import numpy as np

from oracle.pz_oracle import philox4x32_10_numpy

KEY_XOR = (0x4C454147, 0x44524157)
MAX_MEMBERS = 16
CELL = 4
M64 = (1 << 64) - 1
WEIGHT_LIMIT = 1 << 32
DRAW_MUTANTS = ("key_words_swapped", "key_not_xored", "cum_below_r", "u_from_word0_shifted", "mask_inverted", "no_first_game")
TALLY_MUTANTS = ("ties_won", "table_transposed", "invalid_clamped", "unterminated_counted", "stride_one")
CASE_N = (1, 63, 64, 65, 257, 4099)
CASE_P = (1, 2, 3, 16)
MEMBER_DTYPES = ("uint8", "int32", "int64")         # index = the value of pz_pool_member_format
SCORE_DTYPES = ("int32", "int16")                   # index = the value of pz_league_score_format
PLANTED = 77                                        # what a member vector holds before a draw


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def philox_key(seed, mutant=None):
    seed = int(seed) & M64
    if mutant == "key_not_xored":
        return (seed & 0xFFFFFFFF, seed >> 32)
    key = ((seed & 0xFFFFFFFF) ^ KEY_XOR[0], (seed >> 32) ^ KEY_XOR[1])
    return key[::-1] if mutant == "key_words_swapped" else key


def weights_usable(weights):
    w = [int(x) for x in weights]
    return all(0 <= x < WEIGHT_LIMIT for x in w) and sum(w) > 0


def draw(weights, n, seed, C, first_game=0, mask=None, prior=None, mutant=None):
    """(members as int64 [n], errors): `prior` is what the vector held before (PLANTED without it); games that are not drawn
    keep it, and so does every game when the weights are unusable (errors == 1 then)"""
    n, C = int(n), int(C) & M64
    members = np.full(n, PLANTED, np.int64) if prior is None else np.asarray(prior, np.int64).copy()
    if not weights_usable(weights):
        return members, 1
    cum = np.cumsum([int(x) for x in weights], dtype=np.int64)       # below 2^36
    W = int(cum[-1])
    g = np.arange(n, dtype=np.uint64)
    G = g if mutant == "no_first_game" else g + np.uint64(int(first_game) & M64)       # (uint64 arithmetic wraps)
    m32 = np.uint64(0xFFFFFFFF)
    words = philox4x32_10_numpy((G & m32, G >> np.uint64(32), np.full(n, C & 0xFFFFFFFF), np.full(n, C >> 32)), philox_key(seed, mutant))
    if mutant == "u_from_word0_shifted":
        u = [int(w0) << 32 for w0 in words[0]]
    else:
        u = [(int(w1) << 32) | int(w0) for w0, w1 in zip(words[0], words[1])]
    r = np.array([(x * W) >> 64 for x in u], dtype=np.int64)         # the 64 x 36-bit product in Python integers
    picked = np.searchsorted(cum, r, side="left" if mutant == "cum_below_r" else "right")   # #{p: cum[p] <= r}
    chosen = np.ones(n, bool) if mask is None else (np.asarray(mask) != 0)
    if mutant == "mask_inverted" and mask is not None:
        chosen = ~chosen
    members[chosen] = picked[chosen]
    return members, 0


def draw_scalar(weights, n, seed, C, first_game=0, mask=None, prior=None):
    """the same in pure Python integers, one game at a time, with a Philox of its own"""
    seed &= M64
    key = ((seed & 0xFFFFFFFF) ^ 0x4C454147, (seed >> 32) ^ 0x44524157)

    def philox(c):
        k0, k1 = key
        c = list(c)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        return c

    members = [PLANTED] * n if prior is None else [int(x) for x in prior]
    w = [int(x) for x in weights]
    if any(x < 0 or x >= 1 << 32 for x in w) or sum(w) == 0:
        return members, 1
    W = sum(w)
    for g in range(n):
        if mask is not None and not mask[g]:
            continue
        G = (first_game + g) & M64
        block = philox([G & 0xFFFFFFFF, G >> 32, C & 0xFFFFFFFF, (C >> 32) & 0xFFFFFFFF])
        r = (((block[1] << 32) | block[0]) * W) >> 64
        p, running = 0, 0
        for x in w:
            running += x
            p += running <= r
        members[g] = p
    return members, 0


# ---- the tally -----------------------------------------------------------------------------------------------------------------
def tally(terminated, buf1, buf2, stride, members_p1, members_p2, P, table=None, errors=0, mutant=None):
    """(table int64 [P, P, 4], errors): the header's sums with ``np.add.at``.  `buf1` / `buf2` are the score buffers as the
    kernel sees them: game g's scores at element g * stride."""
    n = len(terminated)
    table = np.zeros((P, P, CELL), np.int64) if table is None else np.asarray(table, np.int64).copy()
    at = np.arange(n, dtype=np.int64) * (1 if mutant == "stride_one" else int(stride))
    s1, s2 = np.asarray(buf1)[at].astype(np.int64), np.asarray(buf2)[at].astype(np.int64)
    ended = np.ones(n, bool) if mutant == "unterminated_counted" else np.asarray(terminated) != 0
    a = np.zeros(n, np.int64) if members_p1 is None else np.asarray(members_p1).astype(np.int64)
    b = np.asarray(members_p2).astype(np.int64)
    if mutant == "invalid_clamped":
        a, b = np.clip(a, 0, P - 1), np.clip(b, 0, P - 1)
    valid = (a >= 0) & (a < P) & (b >= 0) & (b < P)
    errors = int(errors) + int((ended & ~valid).sum())
    hit = ended & valid
    a, b, s1, s2 = a[hit], b[hit], s1[hit], s2[hit]
    if mutant == "table_transposed":
        a, b = b, a
    won = (s1 >= s2) if mutant == "ties_won" else (s1 > s2)
    with np.errstate(over="ignore"):
        np.add.at(table, (a, b, 0), 1)
        np.add.at(table, (a, b, 1), won.astype(np.int64))
        np.add.at(table, (a, b, 2), s1)
        np.add.at(table, (a, b, 3), s2)
    return table, errors


def tally_scalar(terminated, buf1, buf2, stride, members_p1, members_p2, P, table=None, errors=0):
    """the same as a loop over the games in Python integers, wrapped to int64 at the end"""
    cells = [[[0] * CELL for _ in range(P)] for _ in range(P)] if table is None else [[[int(x) for x in cell] for cell in row] for row in table]
    errors = int(errors)
    for g in range(len(terminated)):
        if not terminated[g]:
            continue
        a = 0 if members_p1 is None else int(members_p1[g])
        b = int(members_p2[g])
        if not (0 <= a < P and 0 <= b < P):
            errors += 1
            continue
        s1, s2 = int(buf1[g * stride]), int(buf2[g * stride])
        cell = cells[a][b]
        cell[0] += 1
        cell[1] += s1 > s2
        cell[2] += s1
        cell[3] += s2
    wrap = lambda x: ((x + (1 << 63)) & M64) - (1 << 63)  # noqa: E731
    return np.array([[[wrap(x) for x in cell] for cell in row] for row in cells], dtype=np.int64).reshape(P, P, CELL), errors


# ---- prioritised fictitious self-play (the binding's one policy choice), restated --------------------------------------------
def pfsp_weights(table, active, power=2.0, prior_games=8.0, row=0):
    table = np.asarray(table, np.int64)
    games, wins = table[row, :, 0].astype(np.float64), table[row, :, 1].astype(np.float64)
    rate = (wins + prior_games / 2) / (games + prior_games)
    w = np.maximum(1, np.round(np.clip(1.0 - rate, 0.0, 1.0) ** power * (1 << 20))).astype(np.int64)
    w[active:] = 0
    return w


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------
WEIGHT_KINDS = ("small", "with_zeros", "one_at_the_limit", "all_at_the_limit")
BAD_WEIGHT_KINDS = ("negative", "two_pow_32", "all_zero")
MASK_KINDS = ("absent", "all_zero", "all_one", "every_third")
FIRST_GAMES = (0, (1 << 32) + 5, (1 << 33) - 40)     # the last one crosses a multiple of 2^32 inside the larger batches
COUNTER_KINDS = ("by_value", "on_the_device", "both")


def make_weights(kind, P):
    """int64 [P].  "small": 1, 2, 3, 1, ... -- sums so small that r meets a prefix sum exactly in many games, which is where
    `<=` and `<` part."""
    w = np.array([1 + p % 3 for p in range(P)], np.int64)
    if kind == "with_zeros":
        w[::2] = 0
        if P == 1:
            w[0] = 5
        elif P > 2:
            w[P - 1] = 0 if P % 2 == 0 else w[P - 1]         # a zero at the end as well, where P allows one
            w[1] = 4
    elif kind == "one_at_the_limit":
        w[P // 2] = WEIGHT_LIMIT - 1
    elif kind == "all_at_the_limit":
        w[:] = WEIGHT_LIMIT - 1
    elif kind == "negative":
        w[P - 1] = -1
    elif kind == "two_pow_32":
        w[0] = WEIGHT_LIMIT
    elif kind == "all_zero":
        w[:] = 0
    elif kind != "small":
        raise ValueError(kind)
    return w


def make_mask(kind, n):
    if kind == "absent":
        return None
    if kind == "all_zero":
        return np.zeros(n, np.uint8)
    if kind == "all_one":
        return np.full(n, 3, np.uint8)                        # any non-zero byte selects
    mask = np.zeros(n, np.uint8)
    mask[::3] = 1
    return mask


def split_counter(kind, C):
    """(by value, on the device or None) with the sum C"""
    if kind == "by_value":
        return C, None
    if kind == "on_the_device":
        return 0, C
    return C - C // 3, C // 3


def draw_cases(n, P):
    """every weight kind x every mask kind, with the member format, first_game and the counter's form cycling through them so
    that each occurs with each weight kind; then the three unusable weight vectors"""
    cases = []
    for i, (wk, mk) in enumerate(itertools.product(WEIGHT_KINDS, MASK_KINDS)):
        wi, mi = divmod(i, len(MASK_KINDS))               # (three values over the four masks of a weight kind: each occurs)
        cases.append(dict(n=n, P=P, weights=wk, mask=mk, dtype=MEMBER_DTYPES[(mi + wi) % 3], first_game=FIRST_GAMES[(mi + 2 * wi + 1) % 3],
                          counter=COUNTER_KINDS[(2 * mi + wi) % 3], C=(5 + i) if i % 2 else (1 << 40) + 3 * i, seed=0x9E3779B97F4A7C15 ^ (n * 131 + P)))
    for i, wk in enumerate(BAD_WEIGHT_KINDS):
        cases.append(dict(n=n, P=P, weights=wk, mask=MASK_KINDS[i], dtype=MEMBER_DTYPES[i], first_game=0, counter=COUNTER_KINDS[i], C=9, seed=3))
    return cases


def all_draw_cases():
    return [c for n in CASE_N for P in CASE_P for c in draw_cases(n, P)]


TERMINATION_KINDS = ("none", "all", "one_lane_per_wave", "last_row_only", "one_in_four")
SCORE_STRIDES = (1, 8, 3)


def make_terminated(kind, n, rng):
    t = np.zeros(n, np.uint8)
    if kind == "all":
        t[:] = rng.integers(1, 256, n)                        # any non-zero byte counts
    elif kind == "one_lane_per_wave":
        t[(17 if n > 17 else 0)::64] = 1
    elif kind == "last_row_only":
        t[n - 1] = 200
    elif kind == "one_in_four":
        t[rng.random(n) < 0.25] = 1
    elif kind != "none":
        raise ValueError(kind)
    return t


def invalid_members(dtype, P, count, rng):
    pool = {"uint8": [P, 255, 128], "int32": [-1, P, (1 << 31) - 1, -(1 << 31)], "int64": [-1, P, 1 << 32, (1 << 40) + 1, -(1 << 63)]}[dtype]
    return rng.choice(np.array(pool, dtype=np.int64), count)


def tally_cases(n, P):
    """every termination pattern x score stride x score format; members_p1 absent / given, the member format and invalid
    members cycle through them"""
    cases = []
    for i, (tk, stride, sd) in enumerate(itertools.product(TERMINATION_KINDS, SCORE_STRIDES, SCORE_DTYPES)):
        cases.append(dict(n=n, P=P, terminated=tk, stride=stride, score_dtype=sd, with_p1=bool(i % 2), member_dtype=MEMBER_DTYPES[(i // 2) % 3],
                          invalid=bool((i // 3) % 2), seed=n * 1000 + P * 50 + i))
    return cases


def all_tally_cases():
    return [c for n in CASE_N for P in CASE_P for c in tally_cases(n, P)]


def tally_inputs(case):
    """dict of numpy arrays for a tally case: terminated, buf1, buf2 (scores at the case's stride, random everywhere else),
    members_p1 (or None), members_p2, table (preloaded near 2^40) and errors (preloaded).  A quarter of the games are ties.
    Games that did not end hold members outside [0, P): they must count nowhere."""
    n, P, stride = case["n"], case["P"], case["stride"]
    rng = np.random.default_rng(case["seed"])
    sd = np.dtype(case["score_dtype"])
    info = np.iinfo(sd)
    size = (n - 1) * stride + 1
    buf1 = rng.integers(info.min, info.max + 1, size, dtype=np.int64)
    buf2 = rng.integers(info.min, info.max + 1, size, dtype=np.int64)
    ties = np.arange(n)[rng.random(n) < 0.25] * stride
    buf2[ties] = buf1[ties]
    terminated = make_terminated(case["terminated"], n, rng)
    md = case["member_dtype"]

    def member_vector():
        m = rng.integers(0, P, n).astype(np.int64)
        if case["invalid"]:
            bad = rng.random(n) < 0.2
            m[bad] = invalid_members(md, P, int(bad.sum()), rng)
        idle = terminated == 0
        m[idle] = invalid_members(md, P, int(idle.sum()), rng)
        return m.astype(md)

    members_p2 = member_vector()
    members_p1 = member_vector() if case["with_p1"] else None
    table = (1 << 40) - 3 + rng.integers(-5, 6, (P, P, CELL)).astype(np.int64)
    return dict(terminated=terminated, buf1=buf1.astype(sd), buf2=buf2.astype(sd), members_p1=members_p1, members_p2=members_p2, table=table,
                errors=11)
