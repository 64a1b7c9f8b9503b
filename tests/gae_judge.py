"""The judge of ``pz_gae`` (include/pikazoo_learn.h): the definition in numpy float32, the cases, and three mutants.

``judge`` is the header's arithmetic operation by operation on float32 arrays -- one numpy ufunc per rounding, so nothing
is fused and nothing is reordered; tests/test_gae_host.py holds it to exact rational arithmetic on dyadic inputs and to the
float64 textbook formula on random ones.  The GPU tests compare the kernel with it bit for bit (uint32 views).  No GPU
result is ever the expected value.
"""
from fractions import Fraction

import numpy as np

F = np.float32
REWARD_DTYPES = ("int32", "float32")
VALUE_DTYPES = ("float32", "float16", "bfloat16")
FLAG_PATTERNS = ("none", "all", "first_row", "last_row", "random10", "random50")
MUTANTS = ("mask_dropped", "v_next_is_v", "gamma_lam_swapped")


def bf16_round(x):
    """float32 array -> the float32 array of its bfloat16 roundings (nearest even), by bit arithmetic"""
    b = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F)


def as_value_dtype(v, dtype):
    """float32 values made representable in `dtype`, still as float32 (the judge's input; float() of them is exact)"""
    v = np.ascontiguousarray(v, F)
    return {"float32": lambda: v, "float16": lambda: v.astype(np.float16).astype(F), "bfloat16": lambda: bf16_round(v)}[dtype]()


def value_bits(v, dtype):
    """the array a device tensor of `dtype` is made of: float32 itself, float16 itself, bfloat16 as its uint16 patterns"""
    if dtype == "float32":
        return np.ascontiguousarray(v, F)
    if dtype == "float16":
        return v.astype(np.float16)
    return (np.ascontiguousarray(v, F).view(np.uint32) >> 16).astype(np.uint16)


def judge(r, d, v, gamma, lam, mutant=None):
    """(adv, ret), float32 [k, n], of rewards r [k, n] (int32 or float32), flags d [k, n] (anything == 0 is "goes on")
    and float32 values v [k + 1, n] -- the header's definition, in its order."""
    r, d, v = np.asarray(r), np.asarray(d), np.asarray(v)
    assert v.dtype == F and r.shape == d.shape and v.shape == (r.shape[0] + 1, r.shape[1])
    k, n = r.shape
    gamma, lam = F(gamma), F(lam)
    gl = F(gamma * lam)
    if mutant == "gamma_lam_swapped":
        gamma, gl = gl, gamma
    zero = np.zeros(n, F)
    a_next = zero.copy()
    adv, ret = np.empty((k, n), F), np.empty((k, n), F)
    for t in range(k - 1, -1, -1):
        nt = np.ones(n, bool) if mutant == "mask_dropped" else d[t] == 0
        rt = r[t].astype(F)
        v_next = v[t] if mutant == "v_next_is_v" else v[t + 1]
        with np.errstate(all="ignore"):
            q = np.where(nt, gamma * v_next, zero)
            delta = (rt + q) - v[t]
            a = delta + np.where(nt, gl * a_next, zero)
            adv[t], ret[t] = a, a + v[t]
        a_next = a
    return adv, ret


def judge_fraction(r, d, v, gamma, lam):
    """the same recurrence in exact rational arithmetic (lists of Fractions [k][n]); inputs must be finite"""
    k, n = np.asarray(r).shape
    g, gl = Fraction(float(gamma)), Fraction(float(gamma)) * Fraction(float(lam))
    a_next = [Fraction(0)] * n
    adv, ret = [None] * k, [None] * k
    for t in range(k - 1, -1, -1):
        row_a, row_r = [], []
        for i in range(n):
            nt = d[t][i] == 0
            vt = Fraction(float(v[t][i]))
            a = Fraction(float(r[t][i])) + (g * Fraction(float(v[t + 1][i])) if nt else 0) - vt + (gl * a_next[i] if nt else 0)
            row_a.append(a)
            row_r.append(a + vt)
        adv[t], ret[t], a_next = row_a, row_r, row_a
    return adv, ret


def judge_float64(r, d, v, gamma, lam):
    """the textbook formula in float64 with 0 / 1 masks: (adv, ret, largest magnitude met)"""
    r, v = np.asarray(r, np.float64), np.asarray(v, np.float64)
    g, gl = float(F(gamma)), float(F(gamma)) * float(F(lam))
    k, n = r.shape
    a_next = np.zeros(n)
    adv, ret = np.empty((k, n)), np.empty((k, n))
    most = float(np.abs(v).max(initial=0.0))
    for t in range(k - 1, -1, -1):
        m = (np.asarray(d[t]) == 0).astype(np.float64)
        delta = r[t] + g * v[t + 1] * m - v[t]
        a = delta + gl * m * a_next
        adv[t], ret[t], a_next = a, a + v[t], a
        most = max(most, float(np.abs(r[t]).max(initial=0.0)), float(np.abs(g * v[t + 1]).max(initial=0.0)),
                   float(np.abs(delta).max(initial=0.0)), float(np.abs(a).max(initial=0.0)), float(np.abs(ret[t]).max(initial=0.0)))
    return adv, ret, most


def flags(pattern, k, n, rng):
    d = np.zeros((k, n), np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "first_row":
        d[0] = 1
    elif pattern == "last_row":
        d[k - 1] = 1
    elif pattern.startswith("random"):
        d[:] = rng.random((k, n)) < int(pattern[6:]) / 100.0
    else:
        assert pattern == "none"
    return d


def make_case(k, n, pattern="random10", reward_dtype="float32", value_dtype="float32", seed=0, agents=2):
    """Seeded inputs of one case: per agent rewards [k, n] and values [k + 1, n] (float32, representable in the value
    dtype), the shared flags.  Rewards are the env's kind: -1 / 0 / 1 as int32, those plus small shaping terms as float32;
    values are of the size of returns.  Every game has a nonzero reward somewhere and values that differ from row to row,
    so that each mutant shows on every case (tests/test_gae_host.py proves it)."""
    rng = np.random.default_rng([seed, k, n, FLAG_PATTERNS.index(pattern)])
    d = flags(pattern, k, n, rng)
    rew, val = [], []
    for _ in range(agents):
        r = rng.integers(-1, 2, size=(k, n)).astype(np.int32)
        if reward_dtype == "float32":
            r = (r + rng.choice(np.array([0.0, 0.01, -0.01, 0.05], F), size=(k, n))).astype(F)
        v = as_value_dtype(rng.uniform(0.5, 3.0, size=(k + 1, n)).astype(F) * rng.choice(np.array([-1.0, 1.0], F), size=(k + 1, n)),
                           value_dtype)
        rew.append(r)
        val.append(v)
    return {"k": k, "n": n, "rew": rew, "val": val, "d": d}


# ---- the cases of the C-ABI tests ------------------------------------------------------------------------------------
# the kernel loads kChunk = 8 rows ahead and scans two chunks per trip of its main loop: below 8 rows only the row-by-row
# head runs; 8 and 16 rows end in each of the two tails without a trip; 24 and 32 rows take one trip into each tail; both
# sides of each of these multiples, with and without head rows
CHUNK = 8
K_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 130)
N_EDGES = (1, 63, 64, 65, 200)
PITCH = 256

# the recipe of the env tests: enough episode ends that nearly every game has two or more
RECIPE = dict(n=256, winning_score=1, seed=7, env_id_base=0, action_seed=11, frames=128)
