"""The judge of the PPO-loss launches (include/pikazoo_ppo.h): the header's definition in numpy float64, on top of
tests/policy_judge.py (its row statistics, log-prob, gradient and row makers; that file is imported, not edited).  No GPU
result is ever an expected value; tests/test_ppo_host.py holds this file to central differences, to a torch float64
formulation under autograd, to a float32 restatement and to six mutants.

WHAT IS EXACT.  Every input is a float32 (or 16-bit) value and enters float64 without error; clip, value_clip, vf_coef,
ent_coef and eps are the float32 values the C ABI receives.  The float64 run is the real-number value of the definition;
every tolerance bounds |kernel - real value|.  U = 2^-24 (float32 unit roundoff: one rounded operation errs by at most
U |result|), u = 2^-53 (float64), EXP_ULP = 3 (the policy header's bound for expf).

THE TOLERANCES ARE DERIVED, operation by operation, in the kernel's order (csrc/pz_ppo.hip):
  * lp, H: policy_judge.log_prob's and entropy_tolerance's bounds, t_lp and t_H (the same row statistics, the same bits).
  * d = lp - old_logp, one subtraction of the kernel's lp:      t_d = t_lp + U (|d| + t_lp).
  * r = exp(d): the argument's error scales r by exp(+-t_d), expf's own is 2 EXP_ULP U r:
        t_r = r (expm1(t_d) + 2 EXP_ULP U exp(t_d)).
  * Ahat = adv, exact; or (adv - mean) * rscale with the float32 mean and rscale pz_ppo_moments wrote, which lie within
    t_mean and t_rs of the real ones (below): t_A = rscale t_mean + (|adv - mean| + t_mean) (t_rs + 2 U (rscale + t_rs)).
  * unc = -Ahat r:  t_unc = |Ahat| t_r + (r + t_r) t_A + U (|unc| + |Ahat| t_r + (r + t_r) t_A).
    The bounds lo = 1 - clip and hi = 1 + clip are one float32 operation each (error <= U, their values lie below 2); the
    clamp is 1-Lipschitz, so rc = clamp(r, lo, hi) errs by t_rc = max(t_r, U), and cl = -Ahat rc by t_cl (as t_unc with
    rc, t_rc).  pg = max(unc, cl): max is 1-Lipschitz in the sup norm, t_pg = max(t_unc, t_cl).  pg is CONTINUOUS in r:
    no branch of it is ambiguous.
  * kl = (r - 1) - d: t_kl = t_r + U |r - 1| + t_d + U (|kl| + t_r + t_d).
  * e = v - ret: t_e = U |e|.  vl = (0.5 e) e, one rounded product of a value with relative error U:
        t_vl = vl ((1 + U)^3 - 1).        With the value clip: dv = v - old_v (t_dv = U |dv|), its clamp errs by <= t_dv,
    vc = old_v + clamp: t_vc = t_dv + U (|vc| + t_dv), ec = vc - ret: t_ec = t_vc + U (|ec| + t_vc), and
    0.5 ec^2 errs by 0.5 ((|ec| + t_ec)^2 (1 + U)^2 - ec^2).
  * gradients of the row: grad_values = (vf_coef g_v) / M, two rounded operations (M = float(n) is exact up to 2^24 rows
    and errs by U beyond): t = vf_coef t_gv / M + (2 + [n > 2^24]) U (|grad| + vf_coef t_gv / M).
    grad_logits is policy_judge.gradient's value and bound for glogp = g_lp / M and gent = -ent_coef / M, plus what the
    two upstream factors themselves carry: glogp errs by t_glogp = (t_unc + (1 + [n > 2^24]) U (|g_lp| + t_unc)) / M and
    enters as glogp ([i == a] - p_i); gent errs by (1 + [n > 2^24]) U |gent| and enters as gent p_i w_i.
    A 16-bit gradient is compared with the judge's value rounded to the format and may sit one unit of the format's last
    place away from it, as in tests/test_gpu_policy.py.
  * A MEAN of n terms x_i with bounds t_i.  The kernel adds the 64 rows of a wave as a butterfly of 6 float32 levels
    (error <= ((1 + U)^6 - 1) sum |x_i| over the wave's own terms, which are up to t_i off), sums the wave partials in
    float64 (ceil(W / 256) + 8 additions deep at most, W = ceil(n / 64): g64 = (ceil(W / 256) + 9) u relative to the sum of
    the partials' magnitudes), divides by n in float64 and rounds once to float32:
        t_mean = (1 + g64) (sum t_i + ((1 + U)^6 - 1) sum (|x_i| + t_i)) / n + g64 sum |x_i| / n + U |mean|.
    loss = policy_loss + vf_coef value_loss - ent_coef entropy is formed in float64 from the unrounded means:
        t_loss = t_pl + vf_coef t_vl + ent_coef t_H + U |loss|.
  * pz_ppo_moments accumulates S1 = sum (x - K) and S2 = sum (x - K)^2 in float64 about K = x[0] (x - K is exact), in a
    fixed order of at most n additions: |err S1| <= g sum |x - K|, |err S2| <= g S2, g = (n + 1) u.
        mean = K + S1 / n:  t_mean = U |mean| + g sum |x - K| / n + 4 u (|K| + |S1 / n|)
        V = S2 - S1^2 / n (= (n - 1) var):  t_V = g S2 + 2 |S1| g sum |x - K| / n + 3 u (S2 + S1^2 / n)
        std = sqrt(V / (n - 1)): relative error t_V / (2 V) + 2 u;   rscale = 1 / (std + eps):
        t_rs = rscale (U + 4 u + (t_V / (2 V)) std / (std + eps)).
    (V == 0 -- a constant vector -- has every x - K == 0 exactly: no error at all.)

THE TWO BRANCH DECISIONS are not stable under roundoff on a boundary; such a row is AMBIGUOUS and either branch passes:
  * r against lo and hi (g_lp = unc or 0; cf = 0 or 1, whose boundary |r - 1| = clip is the same one): the kernel's r is
    within t_r of r and its bound within U of the real one, so the decision can differ only if |r - lo| or |r - hi| is
    at most  w_r = t_r + U.  With normalisation a sign of Ahat that t_A cannot tell (|Ahat| <= t_A) counts too.
  * ec^2 against e^2, and |dv| against value_clip.  The squares compare as |ec| against |e|; each magnitude is off by its
    bound and by U / 2 relative from the rounded square: w_v = t_ec + t_e + U (|ec| + |e|); the inner one: w_i = t_dv.
    An UNCLAMPED row has ec = e up to roundoff and sits on the outer boundary by construction -- both branches then give
    the same vl and g_v within their bounds; a row counts as ambiguous (for the 1 % cap) only if its admissible
    alternatives differ by more than their bounds.
For an ambiguous row every admissible alternative of g_lp, cf, vl, g_v and of the two gradients passes, and a reduced
statistic gets the slack sum_i max_k |alternative_k - judged value| / n on top of its bound.
"""
import numpy as np

import policy_judge as J

U = J.U
U64 = 2.0 ** -53
EXP_ULP = J.EXP_ULP
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")
MUTANTS = ("clip_on_the_wrong_side", "value_clip_gradient_kept", "entropy_sign_flipped", "mean_missing_from_value_gradient",
           "biased_variance", "naive_sum_of_squares")
ROWS_PER_WAVE = 64
FINISH_THREADS = 256
MOMENT_ROWS = 4096
GOOD_KINDS = tuple(k for k in J.ROW_KINDS if k not in ("nan", "plus_inf", "all_minus_inf"))


def f32(x):
    """the float32 value the C ABI receives for a by-value float, as float64"""
    return float(np.float32(x))


# ---- the moments -------------------------------------------------------------------------------------------------------------
def moments(x, eps=1e-8, mutant=None):
    """(mean, rscale, t_mean, t_rs) of the float32 vector x, in float64 (docstring: pz_ppo_moments)"""
    x = np.asarray(x, np.float64).ravel()
    n = x.size
    K = x[0]
    d = x - K
    S1, S2, sabs = d.sum(), (d * d).sum(), np.abs(d).sum()
    mean = K + S1 / n
    V = max(S2 - S1 * S1 / n, 0.0)
    std = np.sqrt(V / (n if mutant == "biased_variance" else n - 1))
    eps = f32(eps)
    rscale = 1.0 / (std + eps) if std + eps > 0 else np.inf
    g = (n + 1) * U64
    t_mean = U * abs(mean) + g * sabs / n + 4 * U64 * (abs(K) + abs(S1 / n))
    t_V = g * S2 + 2 * abs(S1) * g * sabs / n + 3 * U64 * (S2 + S1 * S1 / n)
    rel = 0.0 if t_V == 0 else (np.inf if V == 0 else t_V / (2 * V))
    t_rs = rscale * (U + 4 * U64 + rel * (std / (std + eps) if std + eps > 0 else 1.0))
    return mean, rscale, t_mean, t_rs


def restate_moments_float32(x, eps=1e-8, mutant=None):
    """(mean, rscale) as float32: the kernel's shifted sums (held in float64 there; here the float32 of its result), or --
    the mutant -- the naive sum x^2 / n - mean^2 accumulated in float32"""
    x32 = np.asarray(x, np.float32).ravel()
    n = x32.size
    if mutant == "naive_sum_of_squares":
        s1 = s2 = np.float32(0)
        for v in x32:
            s1 = np.float32(s1 + v)
            s2 = np.float32(s2 + v * v)
        mean = np.float32(s1 / np.float32(n))
        var = np.float32(max(np.float32(s2 / np.float32(n)) - mean * mean, np.float32(0))) * np.float32(n) / np.float32(n - 1)
        with np.errstate(divide="ignore"):
            return float(mean), float(np.float32(1) / (np.sqrt(np.float32(var)) + np.float32(eps)))
    mean, rscale, _, _ = moments(x32, eps, mutant)
    return float(np.float32(mean)), float(np.float32(rscale))


# ---- the loss ----------------------------------------------------------------------------------------------------------------
def _mean_bound(x, t, n, slack=0.0):
    """(mean, bound) of the kernel's mean of the per-row terms x with bounds t (docstring: A MEAN); NaN where a term is"""
    w = -(-n // ROWS_PER_WAVE)
    g64 = (-(-w // FINISH_THREADS) + 9) * U64
    fin = np.isfinite(x)
    mag, tt = np.abs(np.where(fin, x, 0.0)), np.where(fin, t, 0.0)
    level = (1 + U) ** 6 - 1
    mean = x.sum() / n
    bound = (1 + g64) * (tt.sum() + level * (mag + tt).sum()) / n + g64 * mag.sum() / n + U * abs(np.where(np.isfinite(mean), mean, 0.0))
    return mean, bound + slack


def judge(case, mutant=None):
    """The definition over one agent's rows.  `case`: logits [n, A] (float32 values), actions, old_logp, adv, ret, values,
    old_values (or None), clip, value_clip, vf_coef, ent_coef, normalize.  Returns per-row values, bounds and admissible
    alternatives, the six statistics with their bounds, and the rows that are ambiguous."""
    l = np.asarray(case["logits"], np.float64)
    n, A = l.shape
    a = np.asarray(case["actions"], np.int64)
    old_logp, adv, ret, v = (np.asarray(case[k], np.float64) for k in ("old_logp", "adv", "ret", "values"))
    clip, value_clip, vf, ent = f32(case["clip"]), f32(case["value_clip"]), f32(case["vf_coef"]), f32(case["ent_coef"])
    big = 1.0 if n > 1 << 24 else 0.0
    st = J.stats(l)
    lp, t_lp = J.log_prob(st, a)
    H, t_H = st["H"], J.entropy_tolerance(st)
    if mutant == "entropy_sign_flipped":
        ent = -ent
    nan_row = st["bad"] | (a < 0) | (a >= A)
    with np.errstate(invalid="ignore", over="ignore"):
        d = lp - old_logp
        t_d = t_lp + U * (np.abs(d) + t_lp)
        r = np.exp(d)
        t_r = r * (np.expm1(t_d) + 2 * EXP_ULP * U * np.exp(t_d))
        if case["normalize"]:
            mean, rscale, t_mean, t_rs = moments(adv, 1e-8, "biased_variance" if mutant == "biased_variance" else None)
            Ahat = (adv - mean) * rscale
            t_A = rscale * t_mean + (np.abs(adv - mean) + t_mean) * (t_rs + 2 * U * (rscale + t_rs))
        else:
            Ahat, t_A = adv, np.zeros(n)
        lo, hi = 1.0 - clip, 1.0 + clip

        def product(rr, t_rr):
            x = -Ahat * rr
            first = np.abs(Ahat) * t_rr + (rr + t_rr) * t_A
            return x, first + U * (np.abs(x) + first)

        unc, t_unc = product(r, t_r)
        cl, t_cl = product(np.clip(r, lo, hi), np.maximum(t_r, U))
        pg, t_pg = np.maximum(unc, cl), np.maximum(t_unc, t_cl)
        if mutant == "clip_on_the_wrong_side":
            flat = ((r > hi) & (Ahat < 0)) | ((r < lo) & (Ahat > 0))
            pg = np.minimum(unc, cl)
        else:
            flat = ((r > hi) & (Ahat > 0)) | ((r < lo) & (Ahat < 0))
        w_r = t_r + U
        near_r = (np.abs(r - lo) <= w_r) | (np.abs(r - hi) <= w_r)
        near_p = near_r | ((t_A > 0) & (np.abs(Ahat) <= t_A) & ((r > hi) | (r < lo)))
        kl = (r - 1.0) - d
        t_kl = t_r + U * np.abs(r - 1.0) + t_d + U * (np.abs(kl) + t_r + t_d)
        cf = (np.abs(r - 1.0) > clip).astype(np.float64)
    pg, kl, cf = (np.where(nan_row, np.nan, x) for x in (pg, kl, cf))
    # g_lp: alternative 0 = unc, alternative 1 = 0
    glp = np.stack([unc, np.zeros(n)], 1)
    t_glp = np.stack([t_unc, np.zeros(n)], 1)
    glp_k = flat.astype(np.int64)
    glp_ok = np.stack([~flat | near_p, flat | near_p], 1)
    # the value term: alternative 0 = unclipped (e), 1 = clipped loss, gradient through (ec), 2 = clipped loss, clamped (0)
    e = v - ret
    t_e = U * np.abs(e)
    vl = np.stack([0.5 * e * e] * 3, 1)
    t_vl = np.stack([0.5 * e * e * ((1 + U) ** 3 - 1)] * 3, 1)
    gv = np.stack([e, e, np.zeros(n)], 1)
    t_gv = np.stack([t_e, t_e, np.zeros(n)], 1)
    v_k = np.zeros(n, np.int64)
    v_ok = np.stack([np.ones(n, bool), np.zeros(n, bool), np.zeros(n, bool)], 1)
    material_v = np.zeros(n, bool)
    if value_clip > 0:
        old_v = np.asarray(case["old_values"], np.float64)
        dv = v - old_v
        t_dv = U * np.abs(dv)
        vc = old_v + np.clip(dv, -value_clip, value_clip)
        t_vc = t_dv + U * (np.abs(vc) + t_dv)
        ec = vc - ret
        t_ec = t_vc + U * (np.abs(ec) + t_vc)
        sel = ec * ec > e * e
        inner = np.abs(dv) <= value_clip
        near_o = np.abs(np.abs(ec) - np.abs(e)) <= t_ec + t_e + U * (np.abs(ec) + np.abs(e))
        near_i = np.abs(np.abs(dv) - value_clip) <= t_dv
        vlc = 0.5 * ec * ec
        t_vlc = 0.5 * ((np.abs(ec) + t_ec) ** 2 * (1 + U) ** 2 - ec * ec)
        vl[:, 1], vl[:, 2], t_vl[:, 1], t_vl[:, 2] = vlc, vlc, t_vlc, t_vlc
        gv[:, 1], t_gv[:, 1] = ec, t_ec
        if mutant == "value_clip_gradient_kept":
            gv[:, 2], t_gv[:, 2] = ec, t_ec
        v_k = np.where(sel, np.where(inner, 1, 2), 0)
        v_ok = np.stack([~sel | near_o, (sel | near_o) & (inner | near_i), (sel | near_o) & (~inner | near_i)], 1)
        rows = np.arange(n)
        for k in range(3):  # an alternative that differs from the judged one by more than the bounds: a real ambiguity
            differs = (np.abs(vl[:, k] - vl[rows, v_k]) > t_vl[:, k] + t_vl[rows, v_k]) | \
                      (np.abs(gv[:, k] - gv[rows, v_k]) > t_gv[:, k] + t_gv[rows, v_k])
            material_v |= v_ok[:, k] & differs
    rows = np.arange(n)
    ambiguous = (near_p & ~nan_row) | material_v
    # the statistics
    slack_vl = np.where(v_ok, np.abs(vl - vl[rows, v_k][:, None]) + t_vl, 0.0).max(1) - t_vl[rows, v_k]
    pl, t_pl = _mean_bound(pg, t_pg, n)
    vlm, t_vlm = _mean_bound(vl[rows, v_k], t_vl[rows, v_k], n, np.maximum(slack_vl, 0.0).sum() / n)
    Hm, t_Hm = _mean_bound(H, t_H, n)
    klm, t_klm = _mean_bound(kl, t_kl, n)
    cfm, t_cfm = _mean_bound(cf, np.zeros(n), n, float((near_r & ~nan_row).sum()) / n)
    loss = pl + vf * vlm - ent * Hm
    t_loss = t_pl + vf * t_vlm + abs(ent) * t_Hm + U * abs(loss if np.isfinite(loss) else 0.0)
    stats = dict(zip(STAT_NAMES, ((loss, t_loss), (pl, t_pl), (vlm, t_vlm), (Hm, t_Hm), (klm, t_klm), (cfm, t_cfm))))
    # the gradients
    M = float(n)
    gvals = vf * gv / (1.0 if mutant == "mean_missing_from_value_gradient" else M)
    t_gvals = vf * t_gv / M + (2 + big) * U * (np.abs(gvals) + vf * t_gv / M)
    p, live = st["p"], st["live"]
    with np.errstate(invalid="ignore"):
        dz = np.where(live, st["d"], 0.0)
        w = np.where(live, (dz - st["logS"][:, None]) + st["H"][:, None], 0.0)
    hot = (np.arange(A)[None, :] == a[:, None]).astype(np.float64)
    gent = -ent / M
    glogits, t_glogits = [], []
    for k in range(2):
        glogp = glp[:, k] / M
        t_glogp = (t_glp[:, k] + (1 + big) * U * (np.abs(glp[:, k]) + t_glp[:, k])) / M
        grad, tol = J.gradient(st, a, np.where(np.isfinite(glogp), glogp, 0.0), np.full(n, gent))
        tol = tol + t_glogp[:, None] * np.abs(hot - p) + (1 + big) * U * abs(gent) * p * np.abs(w)
        glogits.append(np.where(nan_row[:, None], np.nan, grad))
        t_glogits.append(tol)
    return dict(n=n, A=A, st=st, nan_row=nan_row, bad=st["bad"], ambiguous=ambiguous, near_r=near_r, lp=lp, r=r, Ahat=Ahat, pg=pg,
                kl=kl, cf=cf, glp=glp, glp_k=glp_k, glp_ok=glp_ok, vl=vl, gv=gv, v_k=v_k, v_ok=v_ok, stats=stats,
                grad_logits=glogits, t_grad_logits=t_glogits, grad_values=gvals, t_grad_values=t_gvals)


def compare(jd, got, logit_dtype="float32", value_dtype="float32"):
    """`got`: {"stats": [6] (or [8]) float, "grad_logits": [n, A] or None, "grad_values": [n] or None} of a kernel, a
    restatement or a mutant, against judge()'s result.  Returns {output: (passed, worst error / bound)}."""
    res = {}
    n = jd["n"]
    for q, name in enumerate(STAT_NAMES):
        want, tol = jd["stats"][name]
        have = float(got["stats"][q])
        if not np.isfinite(want):
            res[name] = ((np.isnan(want) and np.isnan(have)) or want == have, 0.0)
        else:
            share = abs(have - want) / tol if tol > 0 else (0.0 if have == want else np.inf)
            res[name] = (bool(np.isfinite(have) and share <= 1), float(share))
    if got.get("grad_values") is not None:
        have = np.asarray(got["grad_values"], np.float64)
        best = np.full(n, np.inf)
        for k in range(3):
            rounded, ulp = J.round_to(jd["grad_values"][:, k], value_dtype)
            allowed = jd["t_grad_values"][:, k] + (ulp if value_dtype != "float32" else 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                share = np.where(allowed > 0, np.abs(have - rounded) / np.where(allowed > 0, allowed, 1.0), np.where(have == rounded, 0.0, np.inf))
            share = np.where(np.isnan(rounded), np.where(np.isnan(have), 0.0, np.inf), share)
            best = np.where(jd["v_ok"][:, k], np.minimum(best, np.nan_to_num(share, nan=np.inf)), best)
        res["grad_values"] = (bool((best <= 1).all()), float(best.max()))
    if got.get("grad_logits") is not None:
        have = np.asarray(got["grad_logits"], np.float64)
        best = np.full(n, np.inf)
        for k in range(2):
            rounded, ulp = J.round_to(jd["grad_logits"][k], logit_dtype)
            allowed = jd["t_grad_logits"][k] + (ulp if logit_dtype != "float32" else 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(have - rounded)
                share = np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err == 0, 0.0, np.inf))
            share = np.where(np.isnan(rounded), np.where(np.isnan(have), 0.0, np.inf), np.nan_to_num(share, nan=np.inf)).max(1)
            best = np.where(jd["glp_ok"][:, k], np.minimum(best, share), best)
        res["grad_logits"] = (bool((best <= 1).all()), float(best.max()))
    return res


def failures(res):
    return sorted(name for name, (ok, _) in res.items() if not ok)


# ---- the definition once more, in numpy float32 in the kernel's order --------------------------------------------------------
def restate_float32(case, mutant=None):
    """{"stats", "grad_logits", "grad_values"} as float32 arithmetic gives them (numpy's exp and log, sums as float32
    pairwise butterflies of 64 and float64 above); it takes the mutants"""
    f = np.float32
    l = np.asarray(case["logits"], f)
    n, A = l.shape
    a = np.asarray(case["actions"], np.int64)
    old_logp, adv, ret, v = (np.asarray(case[k], f) for k in ("old_logp", "adv", "ret", "values"))
    clip, value_clip, vf, ent = f(case["clip"]), f(case["value_clip"]), f(case["vf_coef"]), f(case["ent_coef"])
    _, lp, H = J.restate_float32(l, np.zeros(n), actions=a)
    bad = np.isnan(H)
    nan_row = np.isnan(lp)
    M = f(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        d = lp - old_logp
        r = np.exp(d)
        if case["normalize"]:
            mean, rscale = restate_moments_float32(adv, 1e-8, mutant if mutant in ("biased_variance", "naive_sum_of_squares") else None)
            Ahat = (adv - f(mean)) * f(rscale)
        else:
            Ahat = adv
        lo, hi = f(1) - clip, f(1) + clip
        unc = -Ahat * r
        cl = -Ahat * np.minimum(np.maximum(r, lo), hi)
        if mutant == "clip_on_the_wrong_side":
            pg = np.where(cl < unc, cl, unc)
            flat = ((r > hi) & (Ahat < 0)) | ((r < lo) & (Ahat > 0))
        else:
            pg = np.where(cl > unc, cl, unc)
            flat = ((r > hi) & (Ahat > 0)) | ((r < lo) & (Ahat < 0))
        g_lp = np.where(flat, f(0), unc)
        kl = (r - f(1)) - d
        cf = np.where(np.isnan(r), f(np.nan), (np.abs(r - f(1)) > clip).astype(f))
        e = v - ret
        g_v, vl = e.copy(), f(0.5) * e * e
        if value_clip > 0:
            old_v = np.asarray(case["old_values"], f)
            dv = v - old_v
            ec = (old_v + np.minimum(np.maximum(dv, -value_clip), value_clip)) - ret
            sel = ec * ec > e * e
            vl = np.where(sel, f(0.5) * ec * ec, vl)
            keep = (np.abs(dv) <= value_clip) | (mutant == "value_clip_gradient_kept")
            g_v = np.where(sel, np.where(keep, ec, f(0)), g_v)
        gvals = vf * g_v if mutant == "mean_missing_from_value_gradient" else vf * g_v / M
        ent_used = -ent if mutant == "entropy_sign_flipped" else ent
        glogp, gent = g_lp / M, -ent_used / M
        safe = np.where(bad[:, None], f(0), l)
        m = safe.max(1, keepdims=True)
        di = safe - m
        ei = np.exp(di)
        S = np.zeros(n, f)
        for i in range(A):
            S = S + ei[:, i]
        logS = np.log(S)
        p = ei / S[:, None]
        hot = (np.arange(A)[None, :] == a[:, None]).astype(f)
        grad = glogp[:, None] * (hot - p)
        second = gent * (-p * ((np.where(ei > 0, di, f(0)) - logS[:, None]) + H[:, None]))
        grad = np.where(ei > 0, grad + second, grad)
        grad = np.where(nan_row[:, None], f(np.nan), grad).astype(f)

    def mean(x):
        pad = np.zeros(-(-n // ROWS_PER_WAVE) * ROWS_PER_WAVE, f)
        pad[:n] = x
        part = pad.reshape(-1, ROWS_PER_WAVE)
        with np.errstate(invalid="ignore"):
            while part.shape[1] > 1:
                half = part.shape[1] // 2
                part = part[:, :half] + part[:, half:]
        return part.astype(np.float64).sum() / n

    pl, vlm, Hm, klm, cfm = mean(pg), mean(vl), mean(H), mean(kl), mean(cf)
    loss = pl + float(vf) * vlm - float(ent_used) * Hm
    return dict(stats=np.array([loss, pl, vlm, Hm, klm, cfm], np.float64).astype(f), grad_logits=grad, grad_values=gvals.astype(f))


# ---- the cases the GPU tests run (tests/test_gpu_ppo.py) and the host tests hold to their conditions -------------------------
N_EDGES = J.N_EDGES + ((FINISH_THREADS + 44) * ROWS_PER_WAVE - 59,)   # 300 partials: the finisher's 256 threads and 44 more
A_EDGES = J.A_EDGES
CLIP, VALUE_CLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
PLANTED = ("ratio_at_upper", "ratio_at_lower", "value_step_at_clip")   # rows 0, 1, 2 of a planted case


def live_actions(logits, rng):
    """one action per row whose logit is finite (a sampled action is never a masked one); 0 for a row without any"""
    fin = np.isfinite(np.asarray(logits, np.float64))
    n = fin.shape[0]
    pick = np.zeros(n, np.int64)
    for g in range(n):
        idx = np.nonzero(fin[g])[0]
        if idx.size:
            pick[g] = idx[rng.integers(idx.size)]
    return pick


def make_case(n, A, dtype, value_dtype, seed, value_clip=VALUE_CLIP, normalize=True, kinds=GOOD_KINDS, planted=False, offset=0.0):
    """One agent's inputs of a case: logits of policy_judge's row kinds, a live action per row, old log-probs a normal
    step of 0.15 from the judged ones (a quarter of the ratios leave [0.8, 1.2]), normal advantages and returns, values
    half a unit and old values a third of a unit apart (value_clip 0.2 clamps about half the rows; float32(0.2) is no
    difference of two 16-bit values, so no row sits on that boundary by accident).  `planted` (float32 values only): rows 0, 1
    and 2 sit ON the boundaries (PLANTED)."""
    rng = np.random.default_rng([seed, n, A, 77])
    l, kind = J.make_rows(n, A, dtype, seed=seed, kinds=kinds)
    a = live_actions(l, rng)
    lp, _ = J.log_prob(J.stats(l), a)
    step = rng.normal(0.0, 0.15, n)
    if planted:
        step[0], step[1] = -np.log(1 + f32(CLIP)), -np.log(1 - f32(CLIP))
    with np.errstate(invalid="ignore"):
        old_logp = np.where(np.isfinite(lp), lp + step, rng.normal(-2.0, 0.5, n)).astype(np.float32)
    adv = (offset + rng.normal(0.0, 1.0, n)).astype(np.float32)
    ret = rng.normal(0.0, 1.0, n).astype(np.float32)
    v = J.as_logit_dtype((ret + rng.normal(0.0, 0.5, n)).astype(np.float32), value_dtype)
    old_v = J.as_logit_dtype((v + rng.normal(0.0, 1.0 / 3, n)).astype(np.float32), value_dtype)
    if planted and n > 2:
        v[2], old_v[2], ret[2] = 0.0, np.float32(value_clip), 1.0   # dv = -value_clip exactly and ec = e: clamped or not is open
    return dict(logits=l, kinds=kind, actions=a, old_logp=old_logp, adv=adv, ret=ret, values=v,
                old_values=old_v if value_clip > 0 else None, clip=CLIP, value_clip=value_clip, vf_coef=VF_COEF, ent_coef=ENT_COEF,
                normalize=normalize and n >= 2)


def moments_cases():
    """the vectors of the moments tests (GPU and host): name -> float32 vector; "offset" is advantages = 1000 + noise of
    spread 1e-3, "many_partials" 300 partials of 4096 rows for the finisher's 256 threads"""
    rng = np.random.default_rng(5)
    big = (FINISH_THREADS + 44) * MOMENT_ROWS - 59
    return {"normal": rng.normal(0.0, 1.0, 4133).astype(np.float32),
            "offset": (1000.0 + rng.normal(0.0, 1e-3, 4133)).astype(np.float32),
            "two": np.array([1.5, -0.25], np.float32),
            "constant": np.full(191, 3.25, np.float32),
            "first_is_an_outlier": np.concatenate([[1e4], rng.normal(0.0, 1.0, 65)]).astype(np.float32),
            "many_partials": rng.normal(0.3, 2.0, big).astype(np.float32)}


def gpu_cases(A, dtype):
    """the cases of tests/test_gpu_ppo.py's main test, which tests/test_ppo_host.py holds to the ambiguity cap and the
    restatement: (name, [agent 1's case, agent 2's], value dtype, planted, fused).  Value clip on for every other n,
    normalisation off for every third; the value format cycles; a fused case keeps the value in the logits' format."""
    out = []
    for i, n in enumerate(N_EDGES):
        vdt = J.LOGIT_DTYPES[(i + J.LOGIT_DTYPES.index(dtype)) % 3]
        out.append((f"n={n}", [make_case(n, A, dtype, vdt, seed=300 + side, value_clip=VALUE_CLIP if i % 2 == 0 else 0.0,
                                         normalize=i % 3 != 1) for side in (0, 1)], vdt, False, False))
    for n in (65, 4133):
        out.append((f"fused n={n}", [make_case(n, A, dtype, dtype, seed=320 + side) for side in (0, 1)], dtype, False, True))
    out.append(("planted", [make_case(191, A, dtype, "float32", seed=310 + side, planted=True) for side in (0, 1)], "float32", True, False))
    return out
