"""The judge of ``pz_vtrace`` (include/pikazoo_vtrace.h): the definition twice, the derived tolerance, the cases, the mutants.

``judge32`` is the header's arithmetic operation by operation on float32 arrays -- one numpy ufunc per rounding, nothing fused,
nothing reordered -- with the importance weight either passed in or computed as the float64 ``exp`` of the float32 log-ratio,
rounded to float32.  ``judge64`` is the textbook formula in float64 with 0 / 1 masks, and with it the tolerance of every
element.  No GPU result is ever the expected value; tests/test_vtrace_host.py holds this file to exact rational arithmetic, the
two formulations to each other, the on-policy case to ``gae_judge.judge`` bit for bit, and the cases to the mutants.

TWO KINDS OF CASES.
  * EXACT: every weight is known to the bit, whatever the device's expf does.  Per element the target log-prob is one of three
    plants: the behaviour log-prob's own bits (d == 0: w = 1, no expf), -inf (d = -inf: w = expf(-inf) = 0), or lpb + 8 with
    every clip <= 4 (w is about 2981 -- any expf within a factor of 700 of the truth leaves w > clip, so the weight IS the
    clip).  ``judge32`` computes exactly these weights, and the GPU is compared with it through uint32 views.
  * TOLERANCE: random log-ratios N(0, 0.5).  The GPU is compared with ``judge64`` within ``tol``, DERIVED below.

THE TOLERANCE IS DERIVED, not tuned.  U = 2^-24 is float32's unit roundoff (a rounded operation's result x carries at most
|x| U), EXP_ULP = 3 the bound on expf that include/pikazoo_policy.h names for this toolchain and tests/policy_judge.py uses
(one ulp <= 2 U relative).  judge64 carries, beside every real quantity, a bound on |float32 quantity - real quantity|:
  * d = lpt - lpb, one rounding: |err d| <= |d| U.  w = expf(d): relative error <= 2 EXP_ULP U from expf and e^{|err d|} - 1 from
    its argument; d == 0 and d == -inf are exact (w = 1 and 0).
  * x = min(clip, w) for the three clips: the minimum is 1-Lipschitz, so |err x| <= |err w|, and 0 where w (1 - rel) > clip.
  * gl = gamma * lam: the real product of the two float32 factors; float32 rounds it once: |err gl| <= gl U.
  * a product a b of quantities with errors ea, eb: |a| eb + |b| ea + ea eb, plus U (|a b| + that) for its rounding; a sum
    likewise ea + eb plus U (|a + b| + ea + eb).  No term is dropped as "second order".
  * these rules are applied, in the header's order, to q, r + q, delta, rho delta, gl c, (gl c) acc_next, acc, vs, gl acc_next,
    the inner sum and pg_adv -- per ELEMENT, the error of acc carried down the rows by the recurrence itself (multiplied by
    gl c <= gl clip_c per row, cut by every episode end).  Rewards and values enter without error (float() of a small int32 and
    of a 16-bit value is exact).
The bound is loose by design where errors cancel; tests/test_vtrace_host.py records how much of it an honest float32 run
(``judge32``, numpy's exp) uses, and checks that every mutant exceeds it.
"""
from fractions import Fraction

import numpy as np

import gae_judge as GJ

F = np.float32
U = 2.0 ** -24       # float32 unit roundoff
EXP_ULP = 3.0        # tests/policy_judge.py, include/pikazoo_policy.h: the bound assumed for expf
REWARD_DTYPES, VALUE_DTYPES, FLAG_PATTERNS = GJ.REWARD_DTYPES, GJ.VALUE_DTYPES, GJ.FLAG_PATTERNS
K_EDGES, N_EDGES, PITCH = GJ.K_EDGES, GJ.N_EDGES, GJ.PITCH
CLIPS = (1.5, 0.75, 3.0)                 # clip_rho != clip_c != clip_pg_rho, all <= 4, on both sides of w = 1
GAMMA, LAM = 0.99, 0.95
MUTANTS = ("rho_c_clips_swapped", "trace_without_c", "pg_adv_from_v_only", "trace_mask_dropped", "ratio_inverted", "nan_weight_becomes_clip")


def weights(lpb, lpt):
    """float32 importance weights as the header defines them, with the float64 exp rounded once in place of expf"""
    with np.errstate(all="ignore"):
        d = np.asarray(lpt, F) - np.asarray(lpb, F)
        return np.where(d == 0, F(1), np.exp(d.astype(np.float64)).astype(F))


def clip(w, c, nan_to_clip=False):
    """(w > c) ? c : w -- a NaN weight stays; the mutant's min(w, c) makes it the clip"""
    with np.errstate(invalid="ignore"):
        return np.where(w < c, w, F(c)) if nan_to_clip else np.where(w > c, F(c), w)


def judge32(r, d, v, lpb, lpt, gamma=GAMMA, lam=LAM, clips=CLIPS, w=None, mutant=None):
    """(pg_adv, vs), float32 [k, n] -- the order of ``gae_judge.judge``'s (adv, ret) -- of rewards r [k, n], flags d [k, n],
    float32 values v [k + 1, n] and float32 log-probs lpb, lpt [k, n]; `w`: the weights, where they are known."""
    r, d, v = np.asarray(r), np.asarray(d), np.asarray(v)
    assert v.dtype == F and r.shape == d.shape == np.shape(lpb) == np.shape(lpt) and v.shape == (r.shape[0] + 1, r.shape[1])
    k, n = r.shape
    gamma, lam = F(gamma), F(lam)
    gl = F(gamma * lam)
    clip_rho, clip_c, clip_pg = (F(x) for x in clips)
    if mutant == "rho_c_clips_swapped":
        clip_rho, clip_c = clip_c, clip_rho
    if w is None:
        w = weights(lpt, lpb) if mutant == "ratio_inverted" else weights(lpb, lpt)
    w = np.asarray(w, F)
    soft = mutant == "nan_weight_becomes_clip"
    zero = np.zeros(n, F)
    acc_next, v_next = zero.copy(), v[k]
    pg_adv, vs = np.empty((k, n), F), np.empty((k, n), F)
    for t in range(k - 1, -1, -1):
        nt = d[t] == 0
        rho, c, pg = clip(w[t], clip_rho, soft), clip(w[t], clip_c, soft), clip(w[t], clip_pg, soft)
        with np.errstate(all="ignore"):
            q = np.where(nt, gamma * v_next, zero)
            delta = (r[t].astype(F) + q) - v[t]
            glc = gl if mutant == "trace_without_c" else gl * c
            trace = glc * acc_next
            acc = rho * delta + (trace if mutant == "trace_mask_dropped" else np.where(nt, trace, zero))
            vs[t] = v[t] + acc
            pg_adv[t] = pg * (delta if mutant == "pg_adv_from_v_only" else delta + np.where(nt, gl * acc_next, zero))
        acc_next, v_next = acc, v[t]
    return pg_adv, vs


def judge_fraction(r, d, v, w, gamma, lam, clips):
    """the recurrence in exact rational arithmetic for given finite weights w [k][n]: (pg_adv, vs) as lists of Fractions"""
    k, n = np.asarray(r).shape
    g, gl = Fraction(float(F(gamma))), Fraction(float(F(gamma))) * Fraction(float(F(lam)))
    cr, cc, cp = (Fraction(float(F(x))) for x in clips)
    acc_next = [Fraction(0)] * n
    pg_adv, vs = [None] * k, [None] * k
    for t in range(k - 1, -1, -1):
        row_p, row_v, row_a = [], [], []
        for i in range(n):
            nt = d[t][i] == 0
            wt, vt = Fraction(float(w[t][i])), Fraction(float(v[t][i]))
            delta = Fraction(float(r[t][i])) + (g * Fraction(float(v[t + 1][i])) if nt else 0) - vt
            acc = min(wt, cr) * delta + (gl * min(wt, cc) * acc_next[i] if nt else 0)
            row_a.append(acc)
            row_v.append(vt + acc)
            row_p.append(min(wt, cp) * (delta + (gl * acc_next[i] if nt else 0)))
        pg_adv[t], vs[t], acc_next = row_p, row_v, row_a
    return pg_adv, vs


# ---- float64, and the error a float32 run may carry ------------------------------------------------------------------------------
def _mul(a, ea, b, eb):
    """a rounded float32 product of quantities known to ea, eb: (real value, bound on the float32 result's distance from it)"""
    e = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return a * b, e + U * (np.abs(a * b) + e)


def _add(a, ea, b, eb):
    e = ea + eb
    return a + b, e + U * (np.abs(a + b) + e)


def judge64(r, d, v, lpb, lpt, gamma=GAMMA, lam=LAM, clips=CLIPS):
    """the textbook formula in float64 with 0 / 1 masks: (pg_adv, vs, tol_pg_adv, tol_vs), all [k, n]; finite inputs, or
    lpt = -inf (a weight of exactly 0)"""
    r, v = np.asarray(r, np.float64), np.asarray(v, np.float64)
    lpb, lpt = np.asarray(lpb, np.float64), np.asarray(lpt, np.float64)
    k, n = r.shape
    g = float(F(gamma))
    gl = g * float(F(lam))
    e_gl = gl * U
    dd = lpt - lpb
    exact = (dd == 0) | np.isneginf(dd)
    w = np.exp(dd)
    with np.errstate(invalid="ignore"):
        rel = np.where(exact, 0.0, (1 + 2 * EXP_ULP * U) * np.exp(np.where(exact, 0.0, np.abs(dd)) * U) - 1)
    e_w = w * rel

    def clipped(c):
        c = float(F(c))
        return np.minimum(w, c), np.where(w * (1 - rel) > c, 0.0, e_w)

    (rho, e_rho), (c, e_c), (pg, e_pg) = (clipped(x) for x in clips)
    acc_next, e_next = np.zeros(n), np.zeros(n)
    out = [np.empty((k, n)) for _ in range(4)]
    zero = np.zeros(n)
    for t in range(k - 1, -1, -1):
        m = (np.asarray(d[t]) == 0).astype(np.float64)
        q, e_q = _mul(g * m, zero, v[t + 1], zero)                 # (a flagged row's q is the constant +0: the bound is 0 there)
        s, e_s = _add(r[t], zero, q, e_q)
        delta, e_delta = _add(s, e_s, -v[t], zero)
        first, e_first = _mul(rho[t], e_rho[t], delta, e_delta)
        glc, e_glc = _mul(gl, e_gl, c[t], e_c[t])
        trace, e_trace = _mul(glc, e_glc, acc_next, e_next)
        acc, e_acc = _add(first, e_first, trace * m, e_trace * m)
        vs, e_vs = _add(v[t], zero, acc, e_acc)
        boot, e_boot = _mul(gl, e_gl, acc_next, e_next)
        inner, e_inner = _add(delta, e_delta, boot * m, e_boot * m)
        pga, e_pga = _mul(pg[t], e_pg[t], inner, e_inner)
        out[0][t], out[1][t], out[2][t], out[3][t] = pga, vs, e_pga, e_vs
        acc_next, e_next = acc, e_acc
    return tuple(out)


def worst_share(got, want, tol):
    """the largest |got - want| / tol over the elements (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    return float(share.max())


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def make_case(k, n, pattern="random10", reward_dtype="float32", value_dtype="float32", seed=0, agents=2, kind="exact"):
    """``gae_judge.make_case`` (rewards, values, flags) with both agents' log-probs: lpb are log-probs of the size a policy over
    18 actions gives; lpt by `kind`: "exact" -- per element lpb's bits, -inf or lpb + 8, a third each; "on_policy" -- lpb's bits;
    "random" -- lpb + N(0, 0.5)"""
    c = GJ.make_case(k, n, pattern, reward_dtype, value_dtype, seed, agents)
    rng = np.random.default_rng([seed, k, n, 77])
    c["lpb"], c["lpt"], c["kind"] = [], [], kind
    for _ in range(agents):
        lpb = (-rng.uniform(0.05, 5.0, size=(k, n))).astype(F)
        if kind == "exact":
            plant = (rng.integers(0, 3, size=(k, n)) + np.arange(n)[None, :] + np.arange(k)[:, None]) % 3   # every game has all three from k = 3
            lpt = np.where(plant == 0, lpb, np.where(plant == 1, F(-np.inf), lpb + F(8))).astype(F)
        elif kind == "on_policy":
            lpt = lpb.copy()
        else:
            assert kind == "random"
            lpt = (lpb + rng.normal(0.0, 0.5, size=(k, n)).astype(F)).astype(F)
        c["lpb"].append(lpb)
        c["lpt"].append(lpt)
    return c


def spec(k, n, pattern="random10", rf="float32", vf="float32", seed=0, pitches=(PITCH,) * 5, both=True, gamma=GAMMA, lam=LAM, clips=CLIPS):
    """one launch of the exact kind: the case and how it goes through the C ABI (pitches: reward, flag, value, log-prob, output)"""
    return dict(k=k, n=n, pattern=pattern, rf=rf, vf=vf, seed=seed, pitches=tuple(pitches), both=both, gamma=gamma, lam=lam, clips=tuple(clips))


# the exact cases of tests/test_gpu_vtrace.py by test; tests/test_vtrace_host.py runs every mutant over the same table
EXACT = {
    "k_edges": [spec(k, 200, seed=1) for k in K_EDGES],
    "n_edges": [spec(33, n, seed=2) for n in N_EDGES],
    "flag_patterns": [spec(k, 200, p, seed=3) for p in FLAG_PATTERNS for k in (1, 17, 130)],
    "formats": [spec(k, n, rf=rf, vf=vf, seed=4) for rf in REWARD_DTYPES for vf in VALUE_DTYPES for k, n in ((33, 200), (7, 65))],
    "one_side": [spec(33, 200, rf=rf, vf=vf, seed=5, both=False) for rf, vf in (("int32", "float32"), ("float32", "bfloat16"))],
    "five_pitches": [spec(33, 200, "random50", rf, vf, seed=6, pitches=(256, 320, 208, 232, 264)) for rf, vf in (("float32", "float32"), ("int32", "float16"))],
    "pitch_is_n": [spec(k, n, seed=7, pitches=(n,) * 5) for k, n in ((33, 200), (8, 65))],
    "gamma_lam_ends": [spec(17, 65, seed=8, gamma=g, lam=l) for g, l in ((0.99, 1.0), (0.99, 0.0), (0.0, 0.95), (1.0, 1.0), (1.0, 0.0))],
    "clip_ends": [spec(17, 65, seed=9, clips=cl) for cl in ((0.0, 0.75, 3.0), (1.5, 0.0, 3.0), (1.5, 0.75, 0.0), (4.0, 0.75, 3.0), (1.5, 4.0, 3.0), (1.5, 0.75, 4.0),
                                                           (0.0, 0.0, 0.0), (4.0, 4.0, 4.0))],
    "many_workgroups": [spec(3, 100003, "random50", "int32", "bfloat16", seed=10, pitches=(100003,) * 5)],
}


# the tolerance cases: random log-ratios, one row, a head and four chunks, sixteen chunks and a head; the two ends of the formats
TOLERANCE = [spec(k, 200, rf=rf, vf=vf, seed=20) for k in (1, 33, 130) for rf, vf in (("float32", "float32"), ("int32", "bfloat16"))]


def case_of(s, kind="exact"):
    return make_case(s["k"], s["n"], s["pattern"], s["rf"], s["vf"], s["seed"], kind=kind)


def nan_case():
    """a NaN target log-prob in row 6 and a NaN behaviour log-prob in row 2 of a 9-row case whose row 4 is an episode end in
    every game: (the case, the rows whose outputs are NaN).  Row 6's NaN runs down the trace to row 5 and stops at the flag; row
    2's reaches rows 1 and 0.  Only vs carries it down: pg_adv of rows 5, 1 and 0 bootstraps from a NaN acc_next too."""
    c = make_case(9, 65, "none", seed=11)
    c["d"][4] = 1
    for lpb, lpt in zip(c["lpb"], c["lpt"]):
        lpt[6], lpb[2] = np.nan, np.nan
    return c, (0, 1, 2, 5, 6)
