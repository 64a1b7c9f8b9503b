"""The judge of the policy-head launches (include/pikazoo_policy.h): the header's definition in numpy float64.  No GPU
result is ever an expected value; tests/test_policy_host.py holds this file to a second, independent formulation, to
central differences, to a float32 restatement and to six mutants.

WHAT IS EXACT.  The logits are float32 (or 16-bit) values and enter as float64 without error; u = (w >> 8) * 2^-24 is
exact; the Philox block is integer arithmetic.  So the float64 run is, for the purposes below, the real-number value of
the definition, and every tolerance bounds |float32 kernel - real value|.

THE TOLERANCES ARE DERIVED, not tuned.  Inputs: U = 2^-24, the float32 unit roundoff (one ulp <= 2 U relative); A; the
ulp bounds EXP_ULP and LOG_ULP of exp and log that the header names (3 and 3); and, per row, from the float64 run:
d_i = l_i - m <= 0, p_i = e_i / S, q = sum p_i |d_i| (<= max |l - m|, and = H - log S <= log A), r = sum p_i d_i^2,
log S (0 <= log S <= log A, because the largest term of S is exp(0) = 1).
  * d_i is one rounded subtraction: |err d_i| <= |d_i| U.
  * e_i: exp's own error <= 2 EXP_ULP U e_i, plus e_i |err d_i|: relative error <= (2 EXP_ULP + |d_i|) U.
  * c_i, a sum of i + 1 <= A positive terms added in order: <= (A - 1) U c_i from the adds, plus the terms' own errors,
    sum_{j<=i} e_j (2 EXP_ULP + |d_j|) U <= 2 EXP_ULP U c_i + q U S.  In particular the relative error of S is
        s_S = (2 EXP_ULP + (A - 1) + q) U.
  * THE DRAW compares c_i with thr = u * S (one more rounding, <= U thr <= U S).  Dividing by S: the float32 decision
    "c_i <= thr" can differ from the real one only if
        |c_i / S - u| <= [ (2 EXP_ULP + A - 1) + q ] U   (numerator)  +  s_S  (denominator, times c_i / S <= 1)  +  U
                       = (2 (2 EXP_ULP + A - 1 + q) + 1) U  =  (2 EXP_ULP + A - 1 + q + 1/2) 2^-23  =: tau.
    With A = 18 and q <= log 18 that is at most 26.4 * 2^-23 (the round figure (A + 8) 2^-23 = 26 * 2^-23).  A row with
    such an i is AMBIGUOUS: the kernel may return either neighbour of that boundary (the last live action <= i or the
    first live one > i; where several boundaries lie within tau of u -- actions of probability below tau -- any live action
    between the outermost two neighbours).  Only boundaries in front of the last live action count: c_i = S from there on
    and the threshold stays below S in the real run (u < 1) and in float32 alike (u * S rounds to a float below S for
    every u <= 1 - 2^-24: tests/test_policy_host.py, test_the_largest_u_and_the_clamp), so the header's clamp to the last
    live action is a guard that never binds, and the mutant that drops it cannot be told apart.
  * logp = (d_a) - log S: |err| <= |d_a| U  +  s_S (log's argument, d log S = dS / S)  +  2 LOG_ULP U log S  +
    U |logp| (the subtraction).
  * T = sum e_i d_i accumulated by fused multiply-adds (one rounding per term): relative to |T| = sum e_i |d_i|:
    terms (2 EXP_ULP + |d_i| + 1) U each and (A - 1) U from the accumulation; sum e_i d_i^2 U / S = r U.  Then T / S:
        |err (T / S)| <= [ q (2 EXP_ULP + 1 + (A - 1)) + r ] U + q s_S + q U.
    entropy = log S - T / S: |err| <= s_S + 2 LOG_ULP U log S + |err (T / S)| + U max(log S, q).
  * the gradient, grad_i = glogp ([i == a] - p_i) + gent (-p_i w_i), w_i = (d_i - log S) + H:
        rel err p_i <= (2 EXP_ULP + |d_i|) U + s_S + U =: rp_i
        |err w_i| <= |d_i| U + s_S + 2 LOG_ULP U log S + U |d_i - log S| + tol_H + U |w_i|
        |err grad_i| <= |glogp| (p_i rp_i + 2 U) + |gent| p_i (|err w_i| + |w_i| (rp_i + 2 U)) + 2 U |grad_i|.
    A 16-bit gradient is compared with the judge's value rounded to the format (nearest even), and may sit one unit of
    the format's last place away from it (its own rounding starts from a value up to the tolerance away).
Subnormal e_i (d_i < -87) carry an absolute error of at most 2^-149 each, against S >= 1: 32 * 2^-149 is added to
nothing below; it is 2^-120 of the smallest tolerance.  An e_i that float32 flushes to zero (d_i < -103.97) is "not live"
for the clamp; the float64 run decides that by float32(e_i) > 0, and the test rows keep every d_i out of (-110, -95).
"""
import numpy as np

from oracle.pz_oracle import philox4x32_10_numpy

U = 2.0 ** -24     # float32 unit roundoff
EXP_ULP = 3.0      # include/pikazoo_policy.h: the bound assumed for expf
LOG_ULP = 3.0      # ... and for logf
LOGIT_DTYPES = ("float32", "float16", "bfloat16")   # the values of pz_policy_logit_format
ACTION_DTYPES = ("int32", "int64")                  # ... of pz_policy_action_format
MUTANTS = ("words_swapped", "first_game_ignored", "step_dev_ignored", "max_not_subtracted", "clamp_dropped",
           "entropy_sign_flipped")
MASK = (1 << 64) - 1


def uniforms(seed, first_game, step, step_dev, n, mutant=None):
    """u[2, n] float64 (exact): step 3 of the header for games first_game .. first_game + n - 1 and both agents"""
    T = (int(step) + (0 if (step_dev is None or mutant == "step_dev_ignored") else int(step_dev))) & MASK
    G = (np.arange(n, dtype=np.uint64) + np.uint64(0 if mutant == "first_game_ignored" else first_game))
    t_lo, t_hi = T & 0xFFFFFFFF, T >> 32
    ctr = (G & np.uint64(0xFFFFFFFF), G >> np.uint64(32), np.full(n, t_lo, np.uint64), np.full(n, (2 + 4 * t_hi) & 0xFFFFFFFF, np.uint64))
    w = philox4x32_10_numpy(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w0, w1 = (w[1], w[0]) if mutant == "words_swapped" else (w[0], w[1])
    return np.stack([(x >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for x in (w0, w1)])


def stats(logits, mutant=None):
    """steps 1, 2, 5 (entropy) and 6 of the header over the rows of `logits` [n, A], in float64"""
    l = np.asarray(logits, np.float64)
    n, A = l.shape
    bad = np.isnan(l).any(1) | (l == np.inf).any(1) | ~np.isfinite(l).any(1)
    safe = np.where(bad[:, None], 0.0, l)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = np.zeros(n) if mutant == "max_not_subtracted" else safe.max(1)
        d = safe - m[:, None]
        e = np.exp(d)
        if mutant == "max_not_subtracted":
            e = e.astype(np.float32).astype(np.float64)  # (what the missing max costs: float32's range)
        c = np.cumsum(e, axis=1)
        S = c[:, -1]
        logS = np.log(S)
        live = e.astype(np.float32) > 0
        p = e / S[:, None]
        dz = np.where(live, d, 0.0)
        q = -(p * dz).sum(1)
        H = logS + (-q if mutant == "entropy_sign_flipped" else q)
        r = (p * dz * dz).sum(1)
    last = A - 1 - np.argmax(live[:, ::-1], axis=1)
    return dict(n=n, A=A, bad=bad, m=m, d=d, e=e, c=c, S=S, logS=logS, live=live, p=p, q=q, r=r, H=np.where(bad, np.nan, H),
                last=last, s_S=(2 * EXP_ULP + (A - 1) + q) * U)


def tau(st):
    """per row: the width around a boundary c_i / S inside which the float32 decision may differ (docstring)"""
    return (2 * EXP_ULP + st["A"] - 1 + st["q"] + 0.5) * 2.0 ** -23


def sample(logits, u, mutant=None):
    """step 4: (action [n], ambiguous [n] bool, neighbours [n, 2], the row statistics) -- an ambiguous row may return
    any LIVE action a with neighbours[0] <= a <= neighbours[1] (the two actions adjacent to its near boundary; with
    several near boundaries, the two outermost)"""
    st = stats(logits, mutant)
    n, A = st["n"], st["A"]
    thr = u * st["S"]
    with np.errstate(invalid="ignore"):
        a = (st["c"][:, :A - 1] <= thr[:, None]).sum(1)
    if mutant != "clamp_dropped":
        a = np.minimum(a, st["last"])
    a = np.where(st["bad"], 0, a)
    with np.errstate(invalid="ignore"):
        near = np.abs(st["c"][:, :A - 1] / st["S"][:, None] - u[:, None]) <= tau(st)[:, None]
    # (a boundary at or behind the last live action never decides: the real draw lies below it, and the clamp undoes it)
    near &= ~st["bad"][:, None] & (np.arange(A - 1)[None, :] < st["last"][:, None])
    ambiguous = near.any(1)
    # the actions adjacent to the near boundaries: the last live action <= the first of them, the first live one > the
    # last of them (small probabilities put several boundaries inside one tau: every live action in between may come out)
    lo, hi = a.copy(), a.copy()
    for g in np.nonzero(ambiguous)[0]:
        first, final = int(np.argmax(near[g])), A - 2 - int(np.argmax(near[g, ::-1]))
        below = [j for j in range(first + 1) if st["live"][g, j]]
        above = [j for j in range(final + 1, A) if st["live"][g, j]]
        lo[g] = below[-1] if below else above[0]
        hi[g] = above[0]  # (there is one: the boundaries counted lie in front of the last live action)
    return a, ambiguous, np.stack([lo, hi], axis=1), st


def log_prob(st, actions):
    """(logp [n], tolerance [n]) at the given actions; NaN for a bad row or an action outside [0, A)"""
    a = np.asarray(actions, np.int64)
    ok = (a >= 0) & (a < st["A"]) & ~st["bad"]
    da = st["d"][np.arange(st["n"]), np.where(ok, a, 0)]
    logp = np.where(ok, da - st["logS"], np.nan)
    with np.errstate(invalid="ignore"):
        mag = np.where(np.isfinite(da), np.abs(da), 0.0)
        tol = (mag + 2 * LOG_ULP * st["logS"] + np.abs(np.where(np.isfinite(logp), logp, 0.0))) * U + st["s_S"]
    return logp, tol


def entropy_tolerance(st):
    A, q, r, logS = st["A"], st["q"], st["r"], st["logS"]
    err_ts = (q * (2 * EXP_ULP + 1 + (A - 1)) + r) * U + q * st["s_S"] + q * U
    return st["s_S"] + 2 * LOG_ULP * U * logS + err_ts + U * np.maximum(logS, q)


def gradient(st, actions, glogp, gent):
    """(grad [n, A], tolerance [n, A]) of glogp * logp + gent * entropy with respect to the logits"""
    a = np.asarray(actions, np.int64)
    n, A = st["n"], st["A"]
    hot = (np.arange(A)[None, :] == a[:, None]).astype(np.float64)
    p, d, live = st["p"], st["d"], st["live"]
    logS, H = st["logS"][:, None], st["H"][:, None]
    glogp, gent = np.asarray(glogp, np.float64)[:, None], np.asarray(gent, np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        dz = np.where(live, d, 0.0)
        w = np.where(live, (dz - logS) + H, 0.0)
        grad = glogp * (hot - p) + np.where(live, gent * (-p * w), 0.0)
        rp = (2 * EXP_ULP + np.abs(dz)) * U + st["s_S"][:, None] + U
        err_w = (np.abs(dz) + 2 * LOG_ULP * logS + np.abs(dz - logS) + np.abs(w)) * U + st["s_S"][:, None] + entropy_tolerance(st)[:, None]
        tol = np.abs(glogp) * (p * rp + 2 * U) + np.abs(gent) * p * (err_w + np.abs(w) * (rp + 2 * U)) + 2 * U * np.abs(grad)
    grad = np.where(st["bad"][:, None], np.nan, grad)
    return grad, tol


# ---- the formats ---------------------------------------------------------------------------------------------------------
def to_bfloat16_bits(x):
    """float -> bfloat16 bit patterns (uint16), round to nearest even, NaN kept"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, np.float32)), ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def from_bfloat16_bits(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def as_logit_dtype(x, dtype):
    """float32 values exactly representable in `dtype` (rounded to it), as float32"""
    x = np.asarray(x, np.float32)
    if dtype == "float32":
        return x
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    return from_bfloat16_bits(to_bfloat16_bits(x))


def logit_bits(x, dtype):
    """the element patterns a device buffer of `dtype` holds for the (representable) float32 values x"""
    x = np.asarray(x, np.float32)
    if dtype == "float32":
        return x.copy()
    if dtype == "float16":
        return x.astype(np.float16)
    return to_bfloat16_bits(x)


def bits_to_float(bits, dtype):
    if dtype == "float32":
        return np.asarray(bits).view(np.float32)
    if dtype == "float16":
        return np.asarray(bits).view(np.float16).astype(np.float32)
    return from_bfloat16_bits(np.asarray(bits).view(np.uint16))


def round_to(x64, dtype):
    """the judge's own rounding of a float64 value to the format (nearest even), and one unit of its last place there"""
    x64 = np.asarray(x64, np.float64)
    mant, emin = {"float32": (23, -126), "float16": (10, -14), "bfloat16": (7, -126)}[dtype]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if dtype == "float16":
            rounded = x64.astype(np.float16).astype(np.float64)
        elif dtype == "bfloat16":
            rounded = from_bfloat16_bits(to_bfloat16_bits(x64.astype(np.float32))).astype(np.float64)
        else:
            rounded = x64.astype(np.float32).astype(np.float64)
        mag = np.where(np.isfinite(x64) & (x64 != 0), np.abs(x64), 2.0 ** emin)
        ulp = 2.0 ** (np.maximum(np.floor(np.log2(mag)), emin) - mant)
    return rounded, ulp


# ---- the rows of the tests -----------------------------------------------------------------------------------------------
# (exp(80) = 5.5e34 still fits float32; "plus100" is the kind that overflows float32's exp unless the max is subtracted, and
# "minus100" the one whose unshifted sum would be subnormal)
ROW_KINDS = ("random0.5", "random2", "random6", "equal", "one_hot", "masked_tail", "plus80", "minus80", "plus100", "minus100", "nan",
             "plus_inf", "all_minus_inf")


def make_rows(n, A, dtype, seed, kinds=ROW_KINDS):
    """[n, A] float32 logits representable in `dtype`, the row kinds cycling, and the kind of every row"""
    rng = np.random.default_rng([seed, n, A])
    l = np.zeros((n, A), np.float32)
    kind = [kinds[g % len(kinds)] for g in range(n)]
    for g, k in enumerate(kind):
        if k.startswith("random"):
            l[g] = rng.normal(0.0, float(k[6:]), A)
        elif k == "equal":
            l[g] = rng.normal(0.0, 3.0)
        elif k == "one_hot":
            l[g] = -np.inf
            l[g, rng.integers(A)] = rng.normal(0.0, 3.0)
        elif k == "masked_tail":  # the last actions masked: with u near 1 the threshold rounds up to S
            l[g] = rng.normal(0.0, 1.0, A)
            l[g, rng.integers(1, A):] = -np.inf
        elif k in ("plus80", "minus80", "plus100", "minus100"):
            l[g] = (1.0 if k[0] == "p" else -1.0) * float(k.lstrip("plusmin")) + rng.normal(0.0, 1.0, A)
        elif k == "nan":
            l[g] = rng.normal(0.0, 1.0, A)
            l[g, rng.integers(A)] = np.nan
        elif k == "plus_inf":
            l[g] = rng.normal(0.0, 1.0, A)
            l[g, rng.integers(A)] = np.inf
        elif k == "all_minus_inf":
            l[g] = -np.inf
        else:
            raise ValueError(k)
    return as_logit_dtype(l, dtype), kind


# ---- the header's steps once more, in numpy float32 (numpy's exp and log, not the device's) --------------------------------
def restate_float32(logits, u, actions=None, mutant=None):
    """(action, logp, entropy) as float32 arithmetic in the header's order gives them; `actions`: given ones (the sampled
    ones otherwise).  tests/test_policy_host.py holds it to the tolerances above: they are neither too tight for honest
    float32 nor blind to a wrong formula.  It takes the mutants too."""
    l = np.asarray(logits, np.float32)
    n, A = l.shape
    f = np.float32
    bad = np.isnan(l).any(1) | (l == np.inf).any(1) | ~np.isfinite(l).any(1)
    l = np.where(bad[:, None], f(0), l)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        m = np.zeros(n, f) if mutant == "max_not_subtracted" else l.max(1)
        d = l - m[:, None]
        e = np.exp(d)
        c = np.zeros((n, A), f)
        run, t, last = np.zeros(n, f), np.zeros(n, f), np.zeros(n, np.int64)
        for i in range(A):
            run = run + e[:, i]
            c[:, i] = run
            live = e[:, i] > 0
            fused = (e[:, i].astype(np.float64) * np.where(live, d[:, i], f(0)).astype(np.float64) + t.astype(np.float64)).astype(f)
            t = np.where(live, fused, t)
            last = np.where(live, i, last)
        S = run
        logS = np.log(S)
        H = logS + t / S if mutant == "entropy_sign_flipped" else logS - t / S
        thr = np.asarray(u, f) * S
        a = (c[:, :A - 1] <= thr[:, None]).sum(1)
        if mutant != "clamp_dropped":
            a = np.minimum(a, last)
        a = np.where(bad, 0, a)
        given = a if actions is None else np.asarray(actions, np.int64)
        ok = (given >= 0) & (given < A) & ~bad
        logp = (d[np.arange(n), np.where(ok, given, 0)]) - logS
    return a, np.where(ok, logp, f(np.nan)), np.where(bad, f(np.nan), H)


# ---- the cases the GPU tests run (tests/test_gpu_policy.py) and the host tests hold to their conditions ---------------------
N_EDGES = (1, 63, 64, 65, 191, 4133)      # below, at and above one wave; three waves less one row; 65 waves less 27 rows
A_EDGES = (2, 13, 18, 32)                 # the ends of the range and the env's two action counts
# (seed, first_game, step, step_dev): the plain one, game ids and steps beyond 2^32, and a device part that carries the step
DRAWS = ((7, 0, 0, None), (7, (1 << 32) + 5, (1 << 33) + 1, None), (0x9E3779B97F4A7C15, 3, 1, (1 << 40) + 9))
# the largest u there is, 1 - 2^-24 (the threshold closest to S: the clamp's case, if it had one): with seed 7 at step 0, word 0
# of game 1 991 157 and word 1 of game 619 726 are 0xFFFFFFxx (found by a search over 2^21 .. 2^28 game ids)
LARGEST_U = {"seed": 7, "step": 0, "game": (1991157, 619726)}


def case_logits(n, A, dtype, draw_index):
    """both agents' [n, A] logits (float32 values representable in `dtype`) of the sampling case, and the rows' kinds"""
    return [make_rows(n, A, dtype, seed=100 * draw_index + side) for side in (0, 1)]


def largest_u_case(A, dtype, side):
    """64 rows whose tail is masked, row 5 of which draws u = 1 - 2^-24 as agent `side`: (logits, first_game)"""
    rows, _ = make_rows(64, A, dtype, seed=900 + side, kinds=("masked_tail",))
    return rows, LARGEST_U["game"][side] - 5
