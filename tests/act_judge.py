"""The judge of the act launch (include/pikazoo_act.h: ``pz_mlp_act``).  The header defines the launch by reference to
pz_mlp_forward and pz_sample_actions, and so does this file: the composition of tests/net_judge.py and tests/policy_judge.py
in numpy float64, a float32 restatement that chains theirs (and takes seven mutants of the seam between the two), the case
tables of tests/test_gpu_act.py, and the planted-row construction.  No GPU result is ever an expected value.

HOW A LAUNCH IS JUDGED (``verdict``), independent of the two older kernels:
  * the head the launch stored is held to net_judge's derived tolerance;
  * policy_judge.sample runs on the launch's OWN head logits (float32 values, which enter float64 exactly: the head's error
    is judged above and is not judged twice), with the uniforms of the header's Philox block: a row that is not ambiguous
    must return the judge's action exactly, an ambiguous one a live action between its neighbours; log-prob and entropy lie
    within policy_judge's tolerances at the returned action;
  * the value is column A of the head, bit for bit.
THE CAP ON AMBIGUOUS ROWS.  A row is ambiguous when a boundary c_i / S lies within tau of u (policy_judge's docstring); u is
uniform over 2^24 values, there are at most A - 1 boundaries, so the expected share is about 2 tau (A - 1): with A = 18 and
tau = 26.4 * 2^-23, 1.1e-4 of the rows.  A case may leave at most max(1, 1 % of n) rows out; the seeds below are fixed so
that the float32 restatement stays inside the cap (tests/test_act_host.py prints the shares).

THE PLANTED ROWS.  relu, W1 and W2 identity blocks with zero biases, one-hot observations: row g with observation e_i
(i = g mod min(K, H)) has hidden vectors e_i exactly (every other product is 0 * w = 0 and 1 * 1 = 1, no rounding), and its
head is column i of W3 plus b3 -- exactly when, per element, one of the two summands is 0 or infinite.  Finite row kinds go in
W3's columns (with b3 = 0); -inf masks and +inf go in b3, never in W3 (0 * inf is NaN); NaN rows come from a NaN
observation, which reaches every hidden unit through 0 * NaN.
"""
import numpy as np

import net_judge as N
import policy_judge as J

MUTANTS = ("words_swapped", "first_game_ignored", "step_dev_ignored", "value_from_column_A_minus_1", "logits_at_pitch_A",
           "agent2_on_agent1_parameters", "half1_columns_dropped")
FINITE_KINDS = ("random0.5", "random2", "random6", "equal", "plus80", "minus80", "plus100", "minus100")

# ---- the cases of tests/test_gpu_act.py -----------------------------------------------------------------------------------------
N_EDGES = (1, 31, 32, 33, 64, 65, 129, 4099)     # below, at and above one tile; two tiles and one row; a workgroup and a row; 129 tiles
SIZES = ((35, 64, 19, 18), (35, 32, 19, 18), (36, 64, 14, 13), (72, 128, 33, 32), (8, 32, 2, 2))   # (K, H, O, A); the last: no value
DRAWS = J.DRAWS
# the cases judged against float64, two agents on nets of their own: (n, size, activation, observation format, index into DRAWS)
JUDGE_CASES = ((257, SIZES[0], "tanh", "float32", 0), (4099, SIZES[0], "tanh", "float32", 1), (129, SIZES[1], "relu", "int32", 2),
               (129, SIZES[2], "tanh", "bfloat16", 2), (65, SIZES[3], "relu", "float16", 1), (129, SIZES[4], "tanh", "int16", 0))
CAP = lambda n: max(1, n // 100)  # noqa: E731


def case_inputs(n, K, H, O, obs_dtype="float32", seed=0):
    """both agents' observations [n, K] (values of `obs_dtype`) and parameter sets"""
    return ([N.make_obs(n, K, obs_dtype, 10 * seed + 3 + s) for s in (0, 1)], [N.make_params(K, H, O, 10 * seed + 1 + s) for s in (0, 1)])


# the case of tests/test_gpu_wide_pitch.py: 40 rows 2^31 elements apart, float16 observations, two agents on nets of their own.
# CAP(40) is one row, and a cap is a condition, not a measurement: the draw and the seed are picked so that the float32
# restatement has NO ambiguous row for either agent (tests/test_act_host.py asserts it and prints the shares)
WIDE_CASE = dict(n=40, size=SIZES[0], activation="tanh", obs_dtype="float16", draw=1, seed=7)


def wide_case_inputs():
    K, H, O, _ = WIDE_CASE["size"]
    return case_inputs(WIDE_CASE["n"], K, H, O, WIDE_CASE["obs_dtype"], seed=WIDE_CASE["seed"])


def uniforms(draw, n):
    seed, first_game, step, step_dev = draw
    return J.uniforms(seed, first_game, step, step_dev, n)


# ---- the definition in float64 ----------------------------------------------------------------------------------------------
def judge(obs, params, activation, A, u):
    """float64: (head [n, O], its tolerance, action [n], ambiguous [n], the row statistics) of one agent"""
    head, tol = N.judge(obs, params, activation)
    a, amb, _, st = J.sample(head[:, :A], u)
    return head, tol, a, amb, st


# ---- the float32 restatement, which also plays the kernel for the mutants ------------------------------------------------------
def restate_float32(obs, params, activation, A, draw, mutant=None):
    """both agents: a list of dicts (head float32 [n, O], actions, log_probs, entropy, values or None), net_judge's float32
    chain followed by policy_judge's; `obs` and `params` are lists over the agents"""
    n = obs[0].shape[0]
    seed, first_game, step, step_dev = draw
    us = J.uniforms(seed, first_game, step, step_dev, n, mutant=mutant if mutant in J.MUTANTS else None)
    out = []
    for s, x in enumerate(obs):
        ps = params[0] if mutant == "agent2_on_agent1_parameters" else params[s]
        head = N.restate_float32(x, ps, activation)
        O = head.shape[1]
        logits = head[:, :A]
        if mutant == "logits_at_pitch_A":  # row g read at g * A of the dense [n, O] head
            flat = np.concatenate([head.ravel(), np.zeros(A, np.float32)])
            logits = np.stack([flat[g * A:g * A + A] for g in range(n)])
        if mutant == "half1_columns_dropped":  # the columns that lanes 32 .. 63 hold never reach the image
            logits = np.where(((np.arange(A) >> 2) & 1)[None, :] == 1, np.float32(0), logits)
        a, logp, ent = J.restate_float32(logits, us[s])
        val = None
        if O > A:
            val = head[:, A - 1] if mutant == "value_from_column_A_minus_1" else head[:, A]
        out.append(dict(head=head, actions=a, log_probs=logp, entropy=ent, values=val))
    return out


def verdict(got, obs, params, activation, A, u, what=""):
    """One agent's outputs `got` (dict: head float32 [n, O], actions, log_probs, entropy, values or None) against the judge, as
    the module docstring says.  Returns (the number of ambiguous rows, the list of failures: empty for a pass)."""
    head = np.asarray(got["head"], np.float32)
    n, O = head.shape
    act, logp, ent = np.asarray(got["actions"], np.int64), np.asarray(got["log_probs"], np.float32), np.asarray(got["entropy"], np.float32)
    fails = []
    ref, tol = N.judge(obs, params, activation)
    worst, rows = N.worst_share(head, ref, tol)
    if worst > 1:
        fails.append(f"{what}: head error / tolerance {worst:.3g} ({rows:.2%} of the rows)")
    a, amb, nb, st = J.sample(head[:, :A].astype(np.float64), u)
    if not ((act >= 0) & (act < A)).all():
        return int(amb.sum()), fails + [f"{what}: an action outside [0, {A})"]
    wrong = np.nonzero(~amb & (act != a))[0]
    if wrong.size:
        fails.append(f"{what}: {wrong.size} unambiguous rows off the judge's action, first row {int(wrong[0])}: {int(act[wrong[0]])} for {int(a[wrong[0]])}")
    if not ((act >= nb[:, 0]) & (act <= nb[:, 1]) & (st["live"][np.arange(n), act] | st["bad"])).all():
        fails.append(f"{what}: an ambiguous row outside its neighbours, or a dead action drawn")
    good = ~st["bad"]
    if not ((act[~good] == 0).all() and np.isnan(logp[~good]).all() and np.isnan(ent[~good]).all()):
        fails.append(f"{what}: a row of step 6 without action 0 and NaN")
    want, ltol = J.log_prob(st, act)
    with np.errstate(invalid="ignore"):
        share_logp = (np.abs(logp.astype(np.float64) - want) / ltol)[good]
        share_ent = (np.abs(ent.astype(np.float64) - st["H"]) / J.entropy_tolerance(st))[good]
    share_logp, share_ent = (np.where(np.isnan(x), np.inf, x) for x in (share_logp, share_ent))
    if good.any():
        print(f"{what}: head {worst:.4f}, log-prob {share_logp.max():.3f}, entropy {share_ent.max():.3f} of the tolerance; {int(amb.sum())} ambiguous of {n}")
        if share_logp.max() > 1:
            fails.append(f"{what}: log-prob error / tolerance {share_logp.max():.3g}")
        if share_ent.max() > 1:
            fails.append(f"{what}: entropy error / tolerance {share_ent.max():.3g}")
    if O > A:
        if got["values"] is None or not np.array_equal(np.asarray(got["values"], np.float32).view(np.uint32), np.ascontiguousarray(head[:, A]).view(np.uint32)):
            fails.append(f"{what}: the value is not column {A} of the head, bit for bit")
    if int(amb.sum()) > CAP(n):
        fails.append(f"{what}: {int(amb.sum())} ambiguous rows, above the cap of {CAP(n)}")
    return int(amb.sum()), fails


# ---- planted rows ---------------------------------------------------------------------------------------------------------------
PLANTED_B3 = ("zero", "masked", "one_hot", "plus_inf")


def planted(n, K, H, O, A, b3_kind, seed=0):
    """(observations [n, K] float32, parameters, the exact float32 logits [n, A], the kind of every row, the masked columns):
    row g holds observation e_i, i = g mod D with D = min(K, H), or a NaN in place of the 1 for the kind "nan"; column i of W3
    holds a finite row kind"""
    D = min(K, H)
    kinds = [(FINITE_KINDS + ("nan",))[i % (len(FINITE_KINDS) + 1)] for i in range(D)]
    finite = [k if k != "nan" else "random2" for k in kinds]
    rows = np.stack([J.make_rows(1, A, "float32", seed=1000 * seed + i, kinds=(k,))[0][0] for i, k in enumerate(finite)])  # [D, A]
    rng = np.random.default_rng([seed, K, H, O, A])
    W1, W2 = np.zeros((H, K), np.float32), np.eye(H, dtype=np.float32)
    W1[np.arange(D), np.arange(D)] = 1
    W3 = np.zeros((O, H), np.float32)
    W3[:A, :D] = rows.T
    if O > A:
        W3[A:, :D] = rng.normal(0, 1, (O - A, D)).astype(np.float32)
    b3 = np.zeros(O, np.float32)
    masked = np.zeros(A, bool)
    if b3_kind == "masked":
        masked[rng.choice(A, size=max(1, A // 3), replace=False)] = True
        masked[A - 1] = True  # (the tail too: the clamp's side)
        if masked.all():
            masked[0] = False
        b3[:A][masked] = -np.inf
    elif b3_kind == "one_hot":
        masked[:] = True
        masked[int(rng.integers(A))] = False
        b3[:A][masked] = -np.inf
    elif b3_kind == "plus_inf":
        b3[int(rng.integers(A))] = np.inf
    params = [W1, np.zeros(H, np.float32), W2, np.zeros(H, np.float32), W3, b3]
    which = np.arange(n) % D
    x = np.zeros((n, K), np.float32)
    kind = [kinds[i] for i in which]
    x[np.arange(n), which] = [np.nan if k == "nan" else 1.0 for k in kind]
    logits = rows[which] + b3[None, :A]
    logits[np.array(kind) == "nan"] = np.nan
    return x, params, logits.astype(np.float32), kind, masked
