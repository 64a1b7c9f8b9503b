"""The judge of the policy-net launch (include/pikazoo_net.h): the header's definition in numpy float64.  No GPU result is
ever an expected value; tests/test_net_host.py holds this file to a torch float64 ``nn.Sequential``, to a float32
restatement in two summation orders and to six mutants.

WHAT IS EXACT.  Observations (int32, int16, float32, 16-bit floats), weights and biases are float32 values -- or, for an
int32 beyond 2^24, integers -- and enter float64 without error, so the float64 run is, for the purposes below, the
real-number value of the definition, and every tolerance bounds |float32 kernel - real value|.

THE TOLERANCES ARE DERIVED, not tuned.  U = 2^-24 is the float32 unit roundoff and gamma_m = m U / (1 - m U).  A layer with
inputs h (float64 values, each carrying an error of at most e), weights W with K columns and bias b computes z = W h + b as
K fused multiply-adds on top of the bias -- K + 1 terms, at most K roundings, in whatever order -- so
    e_z = (1 + gamma_{K+1}) |W| e  +  gamma_{K+1} (|W| |h| + |b|)
(the standard bound of an inner product, which holds for every summation order; products by the kernel's own zero pads are
exact and add nothing).  Through the activation: tanh is 1-Lipschitz and the header's bound on the device's tanh is 5 ulp
of a value of magnitude <= 1, so e_h = e_z + T with T = 10 U; relu is 1-Lipschitz and exact, e_h = e_z.  The first layer
starts from e = 0, or from |x - float32(x)| where an int32 observation had to round.  A 16-bit output is the kernel's
float32 value rounded once more: half a unit of the target format's last place at |ref| + tol is added.  There are no
branch decisions, hence no ambiguity set: every element of every row is judged.
"""
import numpy as np

import policy_judge as J

U = J.U
TANH_ULP = 5.0                 # include/pikazoo_net.h: the bound assumed for tanhf ...
TANH_ABS = 2 * TANH_ULP * U    # ... as an absolute error, |tanh| <= 1
OBS_DTYPES = ("int32", "int16", "float32", "float16", "bfloat16")    # the values of pz_net_obs_format
OUT_DTYPES = J.LOGIT_DTYPES                                          # ... of pz_net_out_format
ACTIVATIONS = ("tanh", "relu")                                       # ... of pz_net_activation
MUTANTS = ("bfloat16_operands", "bfloat16_hidden", "rational_tanh", "b2_dropped", "w2_columns_swapped", "last_input_dropped")


def gamma(m):
    return m * U / (1 - m * U)


def activation64(z, activation):
    return np.tanh(z) if activation == "tanh" else np.where(z < 0, 0.0, z)


def judge(obs, params, activation, out_dtype="float32"):
    """(head [n, O] float64, tolerance [n, O]) of observation rows `obs` (any integer or float array: its values are the
    observations) under `params` = (W1, b1, W2, b2, W3, b3) float32.  A NaN row gives NaN rows of both."""
    x = np.asarray(obs)
    h = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(h - h.astype(np.float32).astype(np.float64)) if x.dtype.kind == "i" else np.zeros_like(h)
        for layer in range(3):
            W, b = (np.asarray(p, np.float64) for p in params[2 * layer:2 * layer + 2])
            g = gamma(W.shape[1] + 1)
            z = h @ W.T + b
            e = (1 + g) * (e @ np.abs(W).T) + g * (np.abs(h) @ np.abs(W).T + np.abs(b))
            if layer < 2:
                h = activation64(z, activation)
                if activation == "tanh":
                    e = e + TANH_ABS
        tol = e
        if out_dtype != "float32":
            _, ulp = J.round_to(np.abs(z) + tol, out_dtype)
            tol = tol + 0.5 * ulp
    return z, tol


def fma32(a, b, c):
    """float32(a * b + c) with one rounding (the product of two float32 is exact in float64; the second rounding of the sum,
    float64 -> float32, moves a result only in cases too rare to matter to a bound)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def rational_tanh(z):
    """the fast tanh of the mutant: a Pade form, clipped"""
    z = z.astype(np.float32)
    return np.clip(z * (np.float32(27) + z * z) / (np.float32(27) + np.float32(9) * z * z), -1, 1).astype(np.float32)


def restate_float32(obs, params, activation, order=None, mutant=None):
    """the definition as float32 arithmetic gives it: each output its bias plus a chain of fused multiply-adds over k, in index
    order or, with `order` = a numpy Generator, in an order drawn per layer; numpy's tanh rounded to float32, not the
    device's.  It takes the mutants too."""
    f = np.float32
    bf = lambda v: J.from_bfloat16_bits(J.to_bfloat16_bits(np.asarray(v, f)))  # noqa: E731
    h = np.asarray(obs).astype(f)
    params = [np.asarray(p, f) for p in params]
    if mutant == "bfloat16_operands":
        h, params = bf(h), [bf(p) if p.ndim == 2 else p for p in params]
    if mutant == "w2_columns_swapped":
        params[2] = params[2].copy()
        params[2][:, [0, 1]] = params[2][:, [1, 0]]
    for layer in range(3):
        W, b = params[2 * layer], params[2 * layer + 1]
        if mutant == "b2_dropped" and layer == 1:
            b = np.zeros_like(b)
        ks = np.arange(W.shape[1])
        if mutant == "last_input_dropped" and layer == 0:
            ks = ks[:-1]
        if order is not None:
            ks = order.permutation(ks)
        acc = np.broadcast_to(b, (h.shape[0], W.shape[0])).astype(f)
        for k in ks:
            acc = fma32(h[:, k:k + 1], W[None, :, k], acc)
        if layer < 2:
            if activation == "relu":
                h = np.where(acc < 0, f(0), acc)
            elif mutant == "rational_tanh":
                h = rational_tanh(acc)
            else:
                h = np.tanh(acc.astype(np.float64)).astype(f)
            if mutant == "bfloat16_hidden":
                h = bf(h)
    return acc


def worst_share(have, ref, tol):
    """(the largest |have - ref| / tol over the elements, the share of rows with an element beyond its tolerance); a NaN on
    one side alone counts as infinite, -inf on both sides (a -inf mask in b3) as no error; +inf stays an error"""
    have, ref = np.asarray(have, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.abs(have - ref) / tol
    both = (np.isnan(have) & np.isnan(ref)) | (np.isneginf(ref) & np.isneginf(have))
    share = np.where(both, 0.0, np.where(np.isnan(share), np.inf, share))
    return float(share.max()) if share.size else 0.0, float((share > 1).any(axis=1).mean()) if share.size else 0.0


# ---- the cases ------------------------------------------------------------------------------------------------------------
def make_params(K, H, O, seed):
    """weights uniform in +-1 / sqrt(fan_in), biases uniform in +-0.2: (W1, b1, W2, b2, W3, b3) float32"""
    rng = np.random.default_rng([seed, K, H, O])
    out = []
    for rows, cols in ((H, K), (H, H), (O, H)):
        out.append(rng.uniform(-1, 1, (rows, cols)).astype(np.float32) / np.float32(np.sqrt(cols)))
        out.append(rng.uniform(-0.2, 0.2, rows).astype(np.float32))
    return out


def make_obs(n, K, dtype, seed):
    """[n, K] observations as an array of the format's own values: uniform in [0, 1) for the float formats (rounded to the
    format), raw integers in [-20, 432] for the integer ones -- the env's own range"""
    rng = np.random.default_rng([seed, n, K, OBS_DTYPES.index(dtype)])
    if dtype in ("int32", "int16"):
        return rng.integers(-20, 433, (n, K)).astype(dtype)
    return J.as_logit_dtype(rng.uniform(0, 1, (n, K)).astype(np.float32), dtype)


def exact_matmul(a, b):
    """a @ b of integer matrices as int64, through a float64 BLAS call (numpy's int64 product takes seconds at the batch sizes
    of the large cases): every product and every partial sum, in any order, is an integer below 2^53 and so an exact float64
    -- asserted on the bound (inner dimension) x max |a| x max |b|"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype.kind == "i" and b.dtype.kind == "i"
    if a.size and b.size:
        assert a.shape[-1] * int(np.abs(a).max()) * int(np.abs(b).max()) < 2 ** 53
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def integer_case(n, K, H, O, seed=5):
    """small integers for relu: weights in [-3, 3] (drawn, so W[i][k] != W[k][i] and no two rows or columns agree), biases in
    [-2, 2], observations in [-2, 4].  Every float32 sum is exact, so the output EQUALS the integer result (int64 here):
    (observations, float32 parameters, the result)."""
    rng = np.random.default_rng([seed, n, K, H, O])
    params = []
    for rows, cols in ((H, K), (H, H), (O, H)):
        params += [rng.integers(-3, 4, (rows, cols)), rng.integers(-2, 3, rows)]
    x = rng.integers(-2, 5, (n, K))
    h = x
    for layer in range(3):
        h = exact_matmul(h, params[2 * layer].T) + params[2 * layer + 1]
        if layer < 2:
            h = np.maximum(h, 0)
            assert np.abs(h).max() < 2 ** 24 // max(H, K) // 4  # every partial sum of the next layer stays an exact float32
    assert np.abs(h).max() < 2 ** 24
    return x, [np.asarray(p, np.float32) for p in params], h
