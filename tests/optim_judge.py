"""The judge of the optimizer step (include/pikazoo_optim.h): the header's definition in numpy float64, with a DERIVED
per-element tolerance for the parameters and both moments.  No GPU result is ever an expected value;
tests/test_optim_host.py holds this file to torch.optim.Adam / AdamW in float64 behind clip_grad_norm_, to a float32
restatement of the header's operation order and to seven mutants.

WHAT IS EXACT.  Parameters, gradients and moments are float32 values and enter float64 without error, the hyperparameters ARE
float64 (the header's pz_adam_config: the numbers torch computes with) and t is an integer, so ONE step in float64 from
float32 state is the real-number value of the definition (up to float64 roundoff,
which the bounds below carry as D = 2^-53 terms), and every tolerance bounds |float32 kernel - real value| of that one step.
Several steps are judged one at a time, each from the state the previous one left (`judge`); `step64` alone, iterated on its
own float64 state, is the k-step definition that the host test compares with torch.

THE TOLERANCES.  U = 2^-24.  Every quantity x carries a bound e_x on the error of the kernel's value.  A float32 operation
rounds once: + U |result|; the square root and the two divisions are given 2 U (one ulp: what the hardware's own
instructions promise; the correctly rounded forms the kernel asks for stay within U).  TINY = 2^-149 (the spacing of the
subnormals) is added to every final tolerance.
  norm   the float64 sum of N exact products, in any order: relative (N + 32) D; its square root and the rounding to float32:
         e_norm = norm (U + (N + 32) D).
  coef   den = norm + 1e-6f: e_den = e_norm + U den;  c = max_f / den: e_c = c e_den / (den - e_den) + U c + 2 U c;  coef = min(c, 1)
         is 1-Lipschitz in c, so e_coef = e_c -- the clip is CONTINUOUS at its boundary, and where c - e_c > 1 both sides are
         exactly 1: e_coef = 0.  Without clipping coef = 1 exactly.
  hyperparameters   max_f, omb1 = 1 - beta1, omb2 = 1 - beta2, beta2_f, eps_f and wd_f are float64 values rounded to float32
         once: U |x| each.
  step_size, bc2   pow in float64 within 4 D relative, so bc = 1 - b^t within 5 D absolute; lr / bc1 and sqrt(bc2^2) in
         float64, rounded to float32 once:  e_ss = U ss + 5 D ss / bc1 + 2 D ss,  e_bc2 = U bc2 + 5 D / (2 bc2)  (the square
         root halves a relative error).   decay = 1 - lr wd in float64, rounded once: U decay + 2 D.
  g1 = coef g: |g| e_coef + U |g1| (a product by an exact 1 is exact: 0);  + wd_f p by a fused multiply-add: + U wd |p| + U |g1|.
  p  = p decay: |p| e_decay + U |p decay|.
  m' = fma(omb1, fl(g1 - m), m): inputs (e_g1 + U |g1 - m|) omb1 + e_omb1 |d| + their product; + U |m'|.
  v' = fma(omb2, fl(g1^2), fl(beta2_f v)): e_gg = 2 |g1| e_g1 + e_g1^2 + U gg;  e_a = U a (beta2_f) + U a;  + U |v'|.
  r  = sqrt(v'): the square root is concave, so |sqrt(x + e) - sqrt(x)| <= sqrt(x) - sqrt(max(x - e, 0));  + 2 U r.
  q  = r / bc2, den = q + eps_f, u = m' / den: a quotient a / b with errors e_a, e_b is off by at most
         (e_a + |a / b| e_b) / (|b| - e_b);  + 2 U |q|, + U eps + U den, + 2 U |u|.  (den - e_den <= 0 would make the tolerance
         infinite; the host test asserts that this never happens in a case the tests use.)
  p' = fma(-ss, u, p): ss e_u + e_ss |u| + e_ss e_u + e_p, and the final rounding: + U |p'|  (>= ulp(p') / 2).
Second-order terms are kept where written; every input error is carried through a rounding with a factor (1 + 2 U).

NON-FINITE VALUES.  Where the definition gives NaN the kernel must give NaN, where it gives an infinity that infinity; the
skip decision (norm not finite) is exact because a float64 sum of float32 squares cannot overflow.  Nothing is ambiguous.
"""
import numpy as np

U = 2.0 ** -24
D = 2.0 ** -53
TINY = 2.0 ** -149
R = 1 + 2 * U
THREADS = 1024
CLIP_EPS = np.float32(1e-6)
MUTANTS = ("no_bias_correction", "eps_inside_sqrt", "clip_without_1e-6", "norm_of_first_tensor", "decay_swapped", "beta1_for_beta2",
           "float32_pow")


def options(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None, skip_nonfinite=False):
    """the hyperparameters as pz_adam_config holds them: float64"""
    mg = 0.0 if max_grad_norm is None else max_grad_norm
    return dict(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), wd=float(weight_decay), max_norm=float(mg),
                decoupled=bool(decoupled), skip=bool(skip_nonfinite))


def clipping(o):
    """the header's test, on the float32 value"""
    with np.errstate(over="ignore"):
        m = np.float32(o["max_norm"])
    return bool(m > 0 and np.isfinite(m))


def make_group(seed, shapes, grad_scale=1.0, t=0):
    """a drawn group: parameters ~ N(0, 0.1), gradients ~ grad_scale N(0, 1); fresh moments at t = 0, else moments as after
    steps on gradients of that scale"""
    rng = np.random.default_rng(seed)
    g = dict(p=[], g=[], m=[], v=[], t=int(t), skipped=0)
    for s in shapes:
        g["p"].append((0.1 * rng.standard_normal(s)).astype(np.float32))
        g["g"].append((grad_scale * rng.standard_normal(s)).astype(np.float32))
        if t:
            g["m"].append((0.3 * grad_scale * rng.standard_normal(s)).astype(np.float32))
            g["v"].append((grad_scale ** 2 * (0.5 + rng.random(s))).astype(np.float32))
        else:
            g["m"].append(np.zeros(s, np.float32))
            g["v"].append(np.zeros(s, np.float32))
    return g


def fresh_gradients(seed, group, grad_scale=1.0):
    rng = np.random.default_rng(seed)
    return [(grad_scale * rng.standard_normal(p.shape)).astype(np.float32) for p in group["p"]]


def bias_corrections(o, t):
    """(bc1, bc2) in float64 from the integer t: Python's pow on a float and an int is exact to float64 roundoff"""
    b1, b2 = float(o["beta1"]), float(o["beta2"])
    return 1.0 - b1 ** int(t), float(np.sqrt(1.0 - b2 ** int(t)))


def step64(p, g, m, v, t, o, lr=None):
    """One step of the definition in float64 on float64 (or float32) lists: (p', m', v', t', norm, coef, skipped?).  This is
    the real-number form: nothing is rounded to float32 (`lr`: the value of a device learning rate, else the options')."""
    lr = float(o["lr"] if lr is None else lr)
    g = [np.asarray(x, np.float64) for x in g]
    with np.errstate(all="ignore"):
        S = sum(float((x * x).sum()) for x in g)
        norm = float(np.sqrt(S))
        coef = 1.0
        if clipping(o):
            c = float(o["max_norm"]) / (norm + float(CLIP_EPS))
            coef = c if not c > 1.0 else 1.0
        if o["skip"] and not np.isfinite(norm):
            return [np.asarray(x, np.float64) for x in p], [np.asarray(x, np.float64) for x in m], [np.asarray(x, np.float64) for x in v], t, norm, coef, True
        t = t + 1
        bc1, bc2 = bias_corrections(o, t)
        b1, b2, eps, wd = float(o["beta1"]), float(o["beta2"]), float(o["eps"]), float(o["wd"])
        P, M, V = [], [], []
        for pi, gi, mi, vi in zip(p, g, m, v):
            pi, mi, vi = (np.asarray(x, np.float64) for x in (pi, mi, vi))
            g1 = coef * gi
            if wd != 0 and not o["decoupled"]:
                g1 = g1 + wd * pi
            if wd != 0 and o["decoupled"]:
                pi = pi * (1.0 - lr * wd)
            mi = mi + (1.0 - b1) * (g1 - mi)
            vi = b2 * vi + (1.0 - b2) * g1 * g1
            den = np.sqrt(vi) / bc2 + eps
            P.append(pi - (lr / bc1) * (mi / den))
            M.append(mi)
            V.append(vi)
    return P, M, V, t, norm, coef, False


def _quotient(a, ea, b, eb):
    """the error bound of a / b under errors ea, eb (inf where b's sign is in doubt)"""
    with np.errstate(all="ignore"):
        lo = np.abs(b) - eb
        return np.where(lo > 0, (ea + np.abs(a / b) * eb) / np.where(lo > 0, lo, 1.0), np.inf)


def judge(group, o, lr=None):
    """One step from the float32 state `group` (make_group's layout): a dict with the float64 references p, m, v (lists), their
    tolerances ep, em, ev, the new t and skipped, norm, coef and their tolerances e_norm, e_coef."""
    lr = float(o["lr"] if lr is None else lr)
    p, g, m, v, t = group["p"], group["g"], group["m"], group["v"], group["t"]
    P, M, V, t1, norm, coef, skipped = step64(p, g, m, v, t, o, lr)
    N = sum(x.size for x in g)
    out = dict(p=P, m=M, v=V, t=t1, skipped=group["skipped"] + int(skipped), norm=norm, coef=coef, did_skip=skipped)
    with np.errstate(all="ignore"):
        e_norm = norm * (U + (N + 32) * D) + TINY if np.isfinite(norm) else 0.0
        e_coef = 0.0
        if clipping(o) and np.isfinite(norm):
            den = norm + float(CLIP_EPS)
            e_den = e_norm * R + U * den
            c = float(o["max_norm"]) / den
            e_c = c * e_den / (den - e_den) * R + U * c * R + 2 * U * c
            e_coef = e_c if c - e_c <= 1.0 else 0.0
        out.update(e_norm=e_norm, e_coef=e_coef + (TINY if e_coef else 0.0))
        if skipped:
            out.update(ep=[np.zeros(x.shape) for x in p], em=[np.zeros(x.shape) for x in p], ev=[np.zeros(x.shape) for x in p])
            return out
        bc1, bc2 = bias_corrections(o, t1)
        e_bc2 = U * bc2 + 5 * D / (2 * bc2)
        ss = lr / bc1
        e_ss = U * ss + 5 * D * ss / bc1 + 2 * D * ss
        b1, b2, eps, wd = float(o["beta1"]), float(o["beta2"]), float(o["eps"]), float(o["wd"])
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        e_omb1, e_omb2, e_b2, e_eps, e_wd = U * omb1, U * omb2, U * b2, U * eps, U * wd
        decay = 1.0 - lr * wd
        e_decay = U * abs(decay) + 2 * D
        ep, em, ev = [], [], []
        for pi, gi, mi, vi in zip(p, g, m, v):
            pi, gi, mi, vi = (np.asarray(x, np.float64) for x in (pi, gi, mi, vi))
            g1 = coef * gi
            e_g1 = np.abs(gi) * e_coef * R + (U * np.abs(g1) if (coef != 1.0 or e_coef) else 0.0)
            e_p = np.zeros_like(pi)
            if wd != 0 and not o["decoupled"]:
                g1 = g1 + wd * pi
                e_g1 = (e_g1 + e_wd * np.abs(pi)) * R + U * np.abs(g1)
            if wd != 0 and o["decoupled"]:
                e_p = np.abs(pi) * e_decay * R + U * np.abs(pi * decay)
                pi = pi * decay
            d = g1 - mi
            e_d = e_g1 * R + U * np.abs(d)
            m1 = mi + omb1 * d
            e_m = (omb1 * e_d + e_omb1 * np.abs(d) + e_omb1 * e_d) * R + U * np.abs(m1)
            a = b2 * vi
            e_a = e_b2 * np.abs(vi) * R + U * np.abs(a)
            gg = g1 * g1
            e_gg = (2 * np.abs(g1) * e_g1 + e_g1 * e_g1) * R + U * gg
            v1 = a + omb2 * gg
            e_v = (omb2 * e_gg + e_omb2 * gg + e_omb2 * e_gg + e_a) * R + U * np.abs(v1)
            r = np.sqrt(v1)
            e_r = (r - np.sqrt(np.maximum(v1 - e_v, 0.0))) * R + 2 * U * r
            q = r / bc2
            e_q = _quotient(r, e_r, bc2, e_bc2) * R + 2 * U * q
            den = q + eps
            e_den = (e_q + e_eps) * R + U * den
            u = m1 / den
            e_u = _quotient(m1, e_m, den, e_den) * R + 2 * U * np.abs(u)
            p1 = pi - ss * u
            e_p1 = (ss * e_u + e_ss * np.abs(u) + e_ss * e_u + e_p) * R + U * np.abs(p1)
            ep.append(e_p1 + TINY)
            em.append(e_m + TINY)
            ev.append(e_v + TINY)
        out.update(ep=ep, em=em, ev=ev)
    return out


def worst_share(got, refs, tols):
    """(largest |got - ref| / tolerance over the finite references, elements beyond their tolerance or of the wrong class)"""
    worst, beyond = 0.0, 0
    for x, r, tol in zip(got, refs, tols):
        x = np.asarray(x, np.float64)
        r = np.asarray(r, np.float64)
        tol = np.broadcast_to(np.asarray(tol, np.float64), r.shape)
        fin = np.isfinite(r)
        beyond += int((np.isnan(r) != np.isnan(x)).sum()) + int((np.isinf(r) & (x != r)).sum()) + int((fin & ~np.isfinite(x)).sum())
        ok = fin & np.isfinite(x)
        if ok.any():
            with np.errstate(all="ignore"):
                diff = np.abs(x[ok] - r[ok])
                share = np.where(diff == 0, 0.0, diff / tol[ok])
            worst = max(worst, float(share.max()))
            beyond += int((share > 1).sum())
    return worst, beyond


def check_group(got, verdict):
    """(worst share over p, m, v; elements beyond) of got = dict(p, m, v) against judge()'s verdict"""
    worst, beyond = 0.0, 0
    for name in ("p", "m", "v"):
        w, b = worst_share(got[name], verdict[name], verdict["e" + name])
        worst, beyond = max(worst, w), beyond + b
    return worst, beyond


# ---- the float32 restatement of the header's operation order, and its mutants ----------------------------------------------
def sum_of_squares_in_kernel_order(grads):
    """S as the header orders it: 1024 float64 partials over the concatenation, the xor butterfly within each wave of 64, the
    16 wave sums in index order"""
    flat = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in grads]).astype(np.float64)
    rounds = -(-flat.size // THREADS)
    sq = np.zeros(rounds * THREADS)
    with np.errstate(all="ignore"):
        sq[:flat.size] = flat * flat
        acc = np.zeros(THREADS)
        for row in sq.reshape(rounds, THREADS):
            acc = acc + row
        acc = acc.reshape(THREADS // 64, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        S = acc[0, 0]
        for w in range(1, THREADS // 64):
            S = S + acc[w, 0]
    return float(S)


def _fma(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact, the sum rounds to float64 and then to
    float32 (a double rounding differs from the fused one only on a tie of the float64 sum: not in these tests' data)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def native_log_pow(b, t):
    """the `float32_pow` mutant: b^t as exp2(t log2 b) in float32 with log2 good to 2^-24 ABSOLUTE -- what a float32 pow built
    on a table or a native logarithm gives next to 1, where log2 b is of the order of 1 - b itself"""
    L = np.float32(np.round(np.log2(float(b)) * 2.0 ** 24) * 2.0 ** -24)
    return np.float32(np.exp2(np.float32(np.float32(t) * L)))


def restate_float32(group, o, lr=None, mutant=None):
    """One step in numpy float32 in the header's operation order: dict(p, m, v, t, skipped, norm, coef)"""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    lr = float(o["lr"] if lr is None else lr)
    p, g, m, v, t = group["p"], group["g"], group["m"], group["v"], group["t"]
    with np.errstate(all="ignore"):
        max_f = f(o["max_norm"])
        S = sum_of_squares_in_kernel_order(g[:1] if mutant == "norm_of_first_tensor" else g)
        norm = f(np.sqrt(S))
        coef = f(1)
        if clipping(o):
            c = max_f / (norm if mutant == "clip_without_1e-6" else f(norm + CLIP_EPS))
            coef = f(1) if c > f(1) else f(c)
        out = dict(norm=norm, coef=coef, t=t, skipped=group["skipped"])
        if o["skip"] and not np.isfinite(norm):
            out.update(p=[x.copy() for x in p], m=[x.copy() for x in m], v=[x.copy() for x in v], skipped=group["skipped"] + 1)
            return out
        t = t + 1
        bc1, bc2 = bias_corrections(o, t)
        ss, bc2 = f(lr / bc1), f(bc2)
        if mutant == "no_bias_correction":
            ss, bc2 = f(lr), f(1)
        if mutant == "float32_pow":
            ss = f(f(lr) / f(f(1) - native_log_pow(f(o["beta1"]), t)))
            bc2 = f(np.sqrt(f(f(1) - native_log_pow(f(o["beta2"]), t))))
        beta2, omb1, omb2 = f(o["beta2"]), f(1.0 - o["beta1"]), f(1.0 - o["beta2"])
        if mutant == "beta1_for_beta2":
            beta2, omb2 = f(o["beta1"]), omb1
        wd, eps = f(o["wd"]), f(o["eps"])
        decay = f(1.0 - lr * o["wd"])
        decoupled = o["decoupled"] != (mutant == "decay_swapped")
        P, M, V = [], [], []
        for pi, gi, mi, vi in zip(p, g, m, v):
            g1 = (coef * gi).astype(f)
            if wd != 0 and not decoupled:
                g1 = _fma(wd, pi, g1)
            if wd != 0 and decoupled:
                pi = (pi * decay).astype(f)
            d = (g1 - mi).astype(f)
            m1 = _fma(omb1, d, mi)
            a = (beta2 * vi).astype(f)
            gg = (g1 * g1).astype(f)
            v1 = _fma(omb2, gg, a)
            if mutant == "eps_inside_sqrt":
                den = (np.sqrt((v1 + eps).astype(f)).astype(f) / bc2).astype(f)
            else:
                den = ((np.sqrt(v1).astype(f) / bc2).astype(f) + eps).astype(f)
            u = (m1 / den).astype(f)
            P.append(_fma(-ss, u, pi))
            M.append(m1)
            V.append(v1)
        out.update(p=P, m=M, v=V, t=t)
    return out


# ---- the cases of tests/test_gpu_optim.py (the host test holds the mutants and the finiteness of the tolerances to them) -------
DEFAULT_NET = ((64, 35), (64,), (64, 64), (64,), (19, 64), (19,))          # 7 571 parameters
LARGEST_BOX = ((128, 72), (128,), (128, 128), (128,), (40, 128), (40,))    # 31 016
SINGLE_SIZES = (1, 3, 63, 64, 65, 1023, 1024, 1025, 4097)
ODD_VIEWS = (1, 3, 5, 64, 127, 1000)
SIXTEEN = tuple((7 + 13 * i,) for i in range(16))
# (name, options): the example's eps; gradients of scale 0.02 have a norm of 1.7 on the default net: a clip at 0.5 engages, at 100 not
OPTION_SETS = (
    ("clip_engaged", dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5)),
    ("clip_idle", dict(lr=3e-4, eps=1e-5, max_grad_norm=100.0)),
    ("no_clip", dict(lr=1e-3, eps=1e-8)),
    ("l2_decay", dict(lr=3e-4, eps=1e-8, weight_decay=0.01, max_grad_norm=0.5)),
    ("adamw", dict(lr=3e-4, eps=1e-8, weight_decay=0.01, decoupled=True, max_grad_norm=0.5)),
)
GRAD_SCALE = 0.02
PLANTED_T = (0, 999_999, 2 ** 31 + 5)
PLANTED_BETAS = (1 - 2.0 ** -16, 1 - 2.0 ** -20)  # betas whose powers are still alive at t = 10^6
STEPS = 3


def gpu_cases():
    """[(name, the shapes of each group, the name of the option set)]: three consecutive steps each"""
    cases = [(f"single_{n}", [((n,),)], "clip_engaged") for n in SINGLE_SIZES]
    cases.append(("odd_views", [tuple((n,) for n in ODD_VIEWS)], "clip_engaged"))
    cases += [(f"default_net_{name}", [DEFAULT_NET], name) for name, _ in OPTION_SETS]
    cases.append(("largest_box", [LARGEST_BOX], "clip_engaged"))
    cases.append(("sixteen_tensors", [SIXTEEN], "no_clip"))
    cases.append(("two_groups", [DEFAULT_NET, LARGEST_BOX], "clip_engaged"))
    cases.append(("two_groups_adamw", [SIXTEEN, DEFAULT_NET], "adamw"))
    return cases


def case_options(name):
    return options(**dict(OPTION_SETS)[name])


def case_groups(index, shapes, t=0):
    """the drawn groups of case number `index`"""
    return [make_group(1000 * index + a, s, GRAD_SCALE, t) for a, s in enumerate(shapes)]


def case_gradients(index, a, step, group):
    """the gradients of group `a` for step 1, 2, ... of case `index` (step 0: the ones make_group drew)"""
    return fresh_gradients(1000 * index + 10 * step + a + 500, group, GRAD_SCALE)


def exact_pin_case(seed=5, shapes=((64, 35), (19,), (3,))):
    """b1 = 0.5, b2 = 0.75, eps = 0, no clip, t = 0, gradients +-2^k, lr = 2^-10, parameters multiples of lr: every
    parameter moves by exactly lr against its gradient's sign, m = g / 2, v = g^2 / 4.  (group, options, expected p, m, v)"""
    rng = np.random.default_rng(seed)
    lr = 2.0 ** -10
    grp = dict(p=[], g=[], m=[], v=[], t=0, skipped=0)
    want = dict(p=[], m=[], v=[])
    for s in shapes:
        g = (rng.choice([-1.0, 1.0], s) * 2.0 ** rng.integers(-8, 9, s)).astype(np.float32)
        p = (lr * rng.integers(-512, 513, s)).astype(np.float32)
        grp["p"].append(p)
        grp["g"].append(g)
        grp["m"].append(np.zeros(s, np.float32))
        grp["v"].append(np.zeros(s, np.float32))
        want["p"].append((p.astype(np.float64) - lr * np.sign(g)).astype(np.float32))
        want["m"].append(g / np.float32(2))
        want["v"].append(g * g / np.float32(4))
    return grp, options(lr=lr, betas=(0.5, 0.75), eps=0.0), want
