"""The judge of the policy-net backward (include/pikazoo_netgrad.h): the header's definition in numpy float64, with a DERIVED
per-element tolerance built on tests/net_judge.py's.  No GPU result is ever an expected value; tests/test_netgrad_host.py
holds this file to torch float64 autograd, to a float32 restatement in two row orders and to seven mutants.

WHAT IS EXACT.  Observations, parameters and grad_head are float32 (or narrower) values and enter float64 without error (an
int32 observation beyond 2^24 carries its rounding as e_x), so the float64 run is the real-number value of the definition and
every tolerance bounds |float32 kernel - real value|.

THE TOLERANCES.  U = 2^-24, gamma_m = m U / (1 - m U).  Every quantity q carries a bound e_q on the error of the kernel's value.
  * The forward errors e_z1, e_h1, e_z2, e_h2 are net_judge.judge's recursion, layer for layer (the host test asserts that the
    third layer of the recursion here reproduces net_judge.judge's tolerance bit for bit).
  * An inner product of m products, summed in ANY order and grouping with one rounding per addition or fused multiply-add,
    of factors a (error e_a) and b (error e_b):
        e = (1 + gamma_m) (|a| e_b + e_a |b| + e_a e_b)  +  gamma_m sum |a| |b|.
    This is W3^T d3 (m = O), W2^T d2 (m = H) and every sum over the rows (m = the number of rows: a row passes through at
    most (rows of its workgroup) + (workgroups - 1) + (1 for the second agent of a shared net) <= m roundings; products by the
    kernel's own zero pads are exact).  A bias gradient is such a sum with b = 1 exactly.
  * tanh: act' = 1 - h^2 is computed from the kernel's h: |hc^2 - h^2| <= 2 |h| e_h + e_h^2, and the square and the
    subtraction round once each on values of magnitude <= 1 + U: e_f = 2 |h| e_h + e_h^2 + 2 U (1 + U).
  * relu: act' is a branch on the sign of z.  A unit with |z_ref| <= e_z is AMBIGUOUS: e_f = 1 there (the full magnitude of
    the factor), else e_f = 0.  The cases the tests use are CHOSEN to have no ambiguous unit (`make_case` draws an offending
    row again, deterministically; the host test asserts it for every case), so no element is ever excused by this rule.
  * d = u f rounds once: e_d = (|u| e_f + |f| e_u + e_u e_f) (1 + U) + U |u f|.
"""
import numpy as np

import net_judge as N
import policy_judge as J

U = N.U
gamma = N.gamma
NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")
GRAD_DTYPES = N.OUT_DTYPES
MUTANTS = ("bfloat16_hidden", "tanh_derivative_not_squared", "relu_derivative_one_at_zero", "w3_columns_swapped", "db2_dropped",
           "last_row_dropped", "agent2_not_summed")


def _product(a, ea, b, eb, m):
    """(a^T b, its tolerance) of [n, p] and [n, q] factors summed over the n rows, m = the roundings a term can pass through"""
    g = gamma(m)
    A, B = np.abs(a), np.abs(b)
    return a.T @ b, (1 + g) * (A.T @ eb + ea.T @ B + ea.T @ eb) + g * (A.T @ B)


def documented_roundings(n, hidden, cus, shared=False):
    """the most roundings a row's term passes through in a sum over the rows, by the sentence of include/pikazoo_netgrad.h: a
    workgroup takes passes of R = 128 / hidden * 32 rows, there are B = min(passes, compute units) workgroups per agent, so a
    workgroup holds at most ceil(passes / B) passes: (rows of its workgroup) + (workgroups - 1) + (1 for a shared net).  `n` is
    the number of rows of ONE agent."""
    R = 32 * (128 // hidden)
    passes = -(-n // R)
    B = min(passes, cus)
    return -(-passes // B) * R + (B - 1) + int(bool(shared))


def judge(sides, params, activation, roundings=None):
    """(six float64 gradients, six tolerances, the number of ambiguous relu units) of `sides` = [(obs [n, K], grad_head [n, O]),
    ...] under `params` = (W1, b1, W2, b2, W3, b3): the gradients are summed over all rows of all sides (a shared net); judge
    one side at a time for separate nets.  `roundings` is the m of the sums over the rows: by default the number of rows, which
    holds for every order of summation; `documented_roundings` gives the header's own, smaller count, under which a large
    batch's tolerance still sees a lost pass."""
    x = np.concatenate([np.asarray(o) for o, _ in sides])
    d3 = np.concatenate([np.asarray(g, np.float64) for _, g in sides])
    W1, b1, W2, b2, W3, b3 = (np.asarray(p, np.float64) for p in params)
    n = x.shape[0]
    roundings = n if roundings is None else roundings
    with np.errstate(invalid="ignore", over="ignore"):
        h0 = x.astype(np.float64)
        e0 = np.abs(h0 - h0.astype(np.float32).astype(np.float64)) if x.dtype.kind == "i" else np.zeros_like(h0)
        zs, hs, ezs, ehs = [], [h0], [], [e0]
        for W, b in ((W1, b1), (W2, b2), (W3, b3)):  # net_judge.judge's recursion
            g = gamma(W.shape[1] + 1)
            zs.append(hs[-1] @ W.T + b)
            ezs.append((1 + g) * (ehs[-1] @ np.abs(W).T) + g * (np.abs(hs[-1]) @ np.abs(W).T + np.abs(b)))
            hs.append(N.activation64(zs[-1], activation))
            ehs.append(ezs[-1] + (N.TANH_ABS if activation == "tanh" else 0.0))
        ambiguous = 0

        def factor(layer):
            nonlocal ambiguous
            z, ez, h, eh = zs[layer], ezs[layer], hs[layer + 1], ehs[layer + 1]
            if activation == "tanh":
                return 1 - h * h, 2 * np.abs(h) * eh + eh * eh + 2 * U * (1 + U)
            unsure = np.abs(z) <= ez
            ambiguous += int(unsure.sum())
            return np.where(z <= 0, 0.0, 1.0), unsure.astype(np.float64)  # (a NaN z: 1, as the header says)

        def through(d, ed, W, layer):
            m = W.shape[0]
            g = gamma(m)
            u = d @ W
            eu = (1 + g) * (ed @ np.abs(W)) + g * (np.abs(d) @ np.abs(W))
            f, ef = factor(layer)
            return u * f, (np.abs(u) * ef + np.abs(f) * eu + eu * ef) * (1 + U) + U * np.abs(u * f)

        e3 = np.zeros_like(d3)
        d2, e2 = through(d3, e3, W3, 1)
        d1, e1 = through(d2, e2, W2, 0)
        one, zero = np.ones((n, 1)), np.zeros((n, 1))
        grads, tols = [], []
        for d, ed, h, eh in ((d1, e1, hs[0], ehs[0]), (d2, e2, hs[1], ehs[1]), (d3, e3, hs[2], ehs[2])):
            for b, eb in ((h, eh), (one, zero)):
                ref, tol = _product(d, ed, b, eb, roundings)
                grads.append(ref if b is h else ref[:, 0])
                tols.append(tol if b is h else tol[:, 0])
    return grads, tols, ambiguous


def forward_tolerance(obs, params, activation):
    """the head and its tolerance out of the recursion above's own first three layers: must equal net_judge.judge"""
    x = np.asarray(obs)
    h = x.astype(np.float64)
    e = np.abs(h - h.astype(np.float32).astype(np.float64)) if x.dtype.kind == "i" else np.zeros_like(h)
    for layer in range(3):
        W, b = (np.asarray(p, np.float64) for p in params[2 * layer:2 * layer + 2])
        g = gamma(W.shape[1] + 1)
        z = h @ W.T + b
        e = (1 + g) * (e @ np.abs(W).T) + g * (np.abs(h) @ np.abs(W).T + np.abs(b))
        if layer < 2:
            h = N.activation64(z, activation)
            e = e + (N.TANH_ABS if activation == "tanh" else 0.0)
    return z, e


def worst_share(have, refs, tols):
    """(the largest |have - ref| / tol over all six tensors, the names of the tensors with an element beyond its tolerance)"""
    worst, beyond = 0.0, []
    for name, h, r, t in zip(NAMES, have, refs, tols):
        h, r, t = (np.asarray(v, np.float64).reshape(-1) for v in (h, r, t))
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(h - r)
            share = np.where(err == 0, 0.0, err / t)  # (a tolerance of 0 -- no term at all, a dead relu unit -- asks for equality)
        share = np.where(np.isnan(h) & np.isnan(r), 0.0, np.where(np.isnan(share), np.inf, share))
        top = float(share.max()) if share.size else 0.0
        worst = max(worst, top)
        if top > 1:
            beyond.append(name)
    return worst, beyond


def _row_chain32(obs, grad, params, activation, mutant=None):
    """the per-row half of the float32 restatement: [(d1, x), (d2, h1), (d3, h2)], each row's factors of the three weight
    gradients, every inner product a chain of fused multiply-adds in index order"""
    f = np.float32
    bf = lambda v: J.from_bfloat16_bits(J.to_bfloat16_bits(np.asarray(v, f)))  # noqa: E731
    W1, b1, W2, b2, W3, b3 = (np.asarray(p, f) for p in params)
    x, d3 = np.asarray(obs).astype(f), np.asarray(grad).astype(f)

    def dense(h, W, b):
        acc = np.broadcast_to(b, (h.shape[0], W.shape[0])).astype(f)
        for k in range(W.shape[1]):
            acc = N.fma32(h[:, k:k + 1], W[None, :, k], acc)
        return acc

    def act(z):
        h = np.where(z < 0, f(0), z) if activation == "relu" else np.tanh(z.astype(np.float64)).astype(f)
        return bf(h) if mutant == "bfloat16_hidden" else h

    def factor(z, h):
        if activation == "tanh":
            return (f(1) - h) if mutant == "tanh_derivative_not_squared" else (f(1) - h * h).astype(f)
        if mutant == "relu_derivative_one_at_zero":
            return np.where(z < 0, f(0), f(1))
        return np.where(z <= 0, f(0), f(1))

    z1 = dense(x, W1, b1)
    h1 = act(z1)
    z2 = dense(h1, W2, b2)
    h2 = act(z2)
    W3b = W3
    if mutant == "w3_columns_swapped":
        W3b = W3.copy()
        W3b[:, [0, 1]] = W3b[:, [1, 0]]
    d2 = (dense(d3, W3b.T.copy(), f(0)) * factor(z2, h2)).astype(f)
    d1 = (dense(d2, W2.T.copy(), f(0)) * factor(z1, h1)).astype(f)
    return [(d1, x), (d2, h1), (d3, h2)]


def restate_float32(sides, params, activation, order=None, mutant=None):
    """the definition as float32 arithmetic gives it: every inner product a chain of fused multiply-adds, the rows summed in
    index order or, with `order` = a numpy Generator, in a drawn order; a shared net's sides are summed one after the other.
    It takes the mutants too.  Six float32 arrays."""
    f = np.float32
    total = None
    for index, (obs, grad) in enumerate(sides):
        if mutant == "agent2_not_summed" and index == 1:
            continue
        if mutant == "last_row_dropped":
            obs, grad = np.asarray(obs)[:-1], np.asarray(grad)[:-1]
        pairs = _row_chain32(obs, grad, params, activation, mutant)
        rows = np.arange(pairs[0][0].shape[0])
        if order is not None:
            rows = order.permutation(rows)
        out = []
        for d, h in pairs:
            dw, db = np.zeros((d.shape[1], h.shape[1]), f), np.zeros(d.shape[1], f)
            for r in rows:
                dw = N.fma32(d[r][:, None], h[r][None, :], dw)
                db = (db + d[r]).astype(f)
            out += [dw, db]
        if mutant == "db2_dropped":
            out[3] = np.zeros_like(out[3])
        total = out if total is None else [(a + b).astype(f) for a, b in zip(total, out)]
    return total


def restate_float32_in_pass_order(sides, params, activation, cus):
    """the float32 restatement with the rows summed in the ORDER include/pikazoo_netgrad.h documents: passes of R = 128 / hidden
    * 32 consecutive rows, B = min(passes, cus) workgroups per agent, workgroup b summing the rows of its passes p = b, b + B,
    ... one after the other into a partial sum; the partials added in index order; a shared net's second agent's total added
    last.  (All workgroups advance together here, one row at a time: the chains are independent.)  Six float32 arrays."""
    f = np.float32
    H = np.asarray(params[0]).shape[0]
    R = 32 * (128 // H)
    total = None
    for obs, grad in sides:
        pairs = _row_chain32(obs, grad, params, activation)
        n = pairs[0][0].shape[0]
        passes = -(-n // R)
        B = min(passes, cus)
        out = []
        for d, h in pairs:
            dw, db = np.zeros((B, d.shape[1], h.shape[1]), f), np.zeros((B, d.shape[1]), f)
            for first in range(0, passes, B):                        # the workgroups' turn-th passes
                for r in range(R):
                    rows = (first + np.arange(B)) * R + r
                    at = np.flatnonzero(rows < n)                    # (workgroups without this pass, or behind row n - 1: +0)
                    if not len(at):
                        break
                    dr, hr = d[rows[at]], h[rows[at]]
                    dw[at] = N.fma32(dr[:, :, None], hr[:, None, :], dw[at])
                    db[at] = (db[at] + dr).astype(f)
            w, b = dw[0], db[0]
            for k in range(1, B):
                w, b = (w + dw[k]).astype(f), (b + db[k]).astype(f)
            out += [w, b]
        total = out if total is None else [(a + b).astype(f) for a, b in zip(total, out)]
    return total


PASS_MUTANTS = ("a_pass_dropped", "a_pass_counted_twice", "partial_last_pass_dropped")


def pass_mutant_rows(n, hidden, mutant, which=1):
    """the rows a kernel with a broken pass loop would sum, as indices into the n rows: pass `which` missing, pass `which` twice,
    or the partial pass at the end missing"""
    R = 32 * (128 // hidden)
    rows = np.arange(n)
    own = (rows >= which * R) & (rows < (which + 1) * R)
    if mutant == "a_pass_dropped":
        return rows[~own]
    if mutant == "a_pass_counted_twice":
        return np.concatenate([rows, rows[own]])
    assert mutant == "partial_last_pass_dropped" and n % R
    return rows[:n - n % R]


# ---- the cases ------------------------------------------------------------------------------------------------------------
def make_grad(n, O, dtype, seed):
    """[n, O] of the format's own values: d loss / d head of a mean over n rows, uniform in +-1 / n"""
    rng = np.random.default_rng([seed, n, O, GRAD_DTYPES.index(dtype)])
    return J.as_logit_dtype((rng.uniform(-1, 1, (n, O)) / n).astype(np.float32), dtype)


def ambiguous_rows(obs, params):
    """which rows hold a relu unit with |z_ref| <= e_z, in either hidden layer (a property of the row and the parameters alone)"""
    x = np.asarray(obs)
    h = x.astype(np.float64)
    e = np.abs(h - h.astype(np.float32).astype(np.float64)) if x.dtype.kind == "i" else np.zeros_like(h)
    bad = np.zeros(x.shape[0], bool)
    for layer in range(2):
        W, b = (np.asarray(p, np.float64) for p in params[2 * layer:2 * layer + 2])
        g = gamma(W.shape[1] + 1)
        z = h @ W.T + b
        e = (1 + g) * (e @ np.abs(W).T) + g * (np.abs(h) @ np.abs(W).T + np.abs(b))
        bad |= (np.abs(z) <= e).any(axis=1)
        h = N.activation64(z, "relu")
    return bad


def make_case(n, K, H, O, activation, seed, agents=1, nets=1, obs_dtype="float32", grad_dtype="float32"):
    """(sides, params): `agents` sides of n rows under one parameter set (`nets` = 1: `params` is that set), or each under a
    set of its own (`nets` = 2: `params` is the list of the two sets, drawn from seed and seed + 1).  A relu case has NO
    ambiguous unit in the judge: a row that holds one under its side's parameters (a unit within its own rounding bound of 0:
    some 1e-3 of the rows at the widest net) is drawn again, from a generator seeded by (seed, side, round), until none is
    left -- deterministic in the arguments, and checked again by the host test for every case the GPU tests use."""
    sets = [N.make_params(K, H, O, seed + i) for i in range(nets)]
    sides = []
    for s in range(agents):
        params = sets[min(s, nets - 1)]
        x = N.make_obs(n, K, obs_dtype, seed + 7 * s + 1)
        if activation == "relu":
            for round_ in range(1, 100):
                bad = ambiguous_rows(x, params)
                if not bad.any():
                    break
                x = x.copy()
                x[bad] = N.make_obs(n, K, obs_dtype, seed + 7 * s + 1 + 100000 * round_)[bad]
            else:
                raise AssertionError(f"no relu case without an ambiguous unit at n = {n}")
        sides.append((x, make_grad(n, O, grad_dtype, seed + 7 * s + 2)))
    if activation == "relu":
        assert all(judge([side], sets[min(s, nets - 1)], activation)[2] == 0 for s, side in enumerate(sides))
    return sides, (sets[0] if nets == 1 else sets)


def integer_case(n, K, H, O, seed=5, small=False):
    """relu on small integers: weights in [-3, 3], biases in [-2, 2], observations in [-2, 4], grad_head in [-2, 2] (`small`:
    [-1, 1], [-1, 1], [-1, 2] and [-1, 1], for many rows).  Every intermediate and every partial sum of every gradient, in
    any order of the rows, is an exact float32 (the sum of the magnitudes of the terms stays below 2^24: asserted), so the
    result must EQUAL the int64 one.  Units with z == 0 are present in both hidden layers' worth of units taken together:
    they pin act'(0) = 0.  (observations, float32 parameters, grad_head, six int64 gradients)"""
    rng = np.random.default_rng([seed, n, K, H, O, int(small)])
    w, b, lo, hi, g = (1, 1, -1, 3, 1) if small else (3, 2, -2, 5, 2)
    params = []
    for rows, cols in ((H, K), (H, H), (O, H)):
        params += [rng.integers(-w, w + 1, (rows, cols)), rng.integers(-b, b + 1, rows)]
    W1, b1, W2, b2, W3, b3 = params
    x = rng.integers(lo, hi, (n, K))
    d3 = rng.integers(-g, g + 1, (n, O))
    limit = 2 ** 24
    mm = N.exact_matmul  # (int64 results through float64 BLAS: exact below 2^53, which it asserts)
    z1 = mm(x, W1.T) + b1
    h1 = np.maximum(z1, 0)
    z2 = mm(h1, W2.T) + b2
    h2 = np.maximum(z2, 0)
    assert (mm(np.abs(x), np.abs(W1).T) + np.abs(b1)).max() < limit and (mm(h1, np.abs(W2).T) + np.abs(b2)).max() < limit
    assert ((z1 == 0).sum() + (z2 == 0).sum()) > 0
    d2 = mm(d3, W3) * (z2 > 0)
    d1 = mm(d2, W2) * (z1 > 0)
    assert mm(np.abs(d3), np.abs(W3)).max() < limit and mm(np.abs(d2), np.abs(W2)).max() < limit
    out = []
    for d, h in ((d1, x), (d2, h1), (d3, h2)):
        assert mm(np.abs(d).T, np.abs(h)).max() < limit and np.abs(d).sum(axis=0).max() < limit
        out += [mm(d.T, h), d.sum(axis=0)]
    return x, [np.asarray(p, np.float32) for p in params], d3, out
