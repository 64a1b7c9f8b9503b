"""The judge of the pool library (include/pikazoo_pool.h).  No GPU result is ever an expected value.

THE PLAN is the header's, in numpy integers with a stable argsort (``plan``), and once more as a scalar pure-Python walk
(``plan_scalar``); tests/test_pool_host.py holds the two to each other and to the properties the header states.

THE FORWARD has no arithmetic of its own: a row's expected value is ``net_judge.judge`` of that row under the parameters of
the row's own member, with net_judge's derived tolerance (``judge``).  A row whose member is not valid is expected to be
left unwritten.  ``effective_members`` says which member's parameters each row runs on -- the definition, or one of the
mutants the host test shows the GPU test's cases to be sharp enough for.

The cases of tests/test_gpu_pool.py are made here, so that the host test can hold the mutants against exactly them.
"""
import numpy as np

import net_judge as N

G = 128                 # PZ_POOL_GROUP_ROWS
MAX_MEMBERS = 16        # PZ_POOL_MAX_MEMBERS
MEMBER_DTYPES = ("uint8", "int32", "int64")      # the values of pz_pool_member_format
PLAN_MUTANTS = ("unstable_order", "missing_pad", "first_off_by_one_group")
FORWARD_MUTANTS = ("next_member_parameters", "invalid_clamped_to_zero", "invalid_clamped_to_last", "agent_2_through_agent_1_plan")

PLAN_N = (1, 31, 32, 33, 127, 128, 129, 257, 4099)
PLAN_P = (1, 2, 3, 16)
MEMBER_KINDS = ("all_one_member", "one_member_empty", "every_count_1_mod_g", "round_robin", "sorted", "reverse_sorted", "invalid_entries")


def capacity(n, P):
    return (n // G + P) * G


def typed(values, dtype):
    """the member vector as the device holds it: the values reduced to the format (-1 is 255 in uint8)"""
    return np.asarray(values, np.int64).astype(dtype)


def valid_rows(members, P):
    m = np.asarray(members).astype(np.int64)       # (uint8 widens to 0..255)
    return (m >= 0) & (m < P)


def plan(members, P, mutant=None):
    """(order int32 [capacity], first int32 [P + 1], errors) of a typed member vector"""
    members = np.asarray(members)
    n = len(members)
    m = members.astype(np.int64)
    valid = valid_rows(members, P)
    rows = np.flatnonzero(valid)
    by_member = rows[np.argsort(m[rows], kind="stable")]
    counts = np.bincount(m[rows], minlength=P)[:P]
    padded = -(-counts // G) * G
    first = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = np.full(capacity(n, P), -1, np.int64)
    for p in range(P):
        mine = by_member[starts[p]:starts[p + 1]]
        if mutant == "unstable_order":
            mine = mine[::-1]
        order[first[p]:first[p] + counts[p]] = mine
        if mutant == "missing_pad" and counts[p]:
            order[first[p] + counts[p]:first[p] + padded[p]] = mine[-1]
    if mutant == "first_off_by_one_group":
        first[1:] += G
    return order.astype(np.int32), first.astype(np.int32), int(n - valid.sum())


def plan_scalar(members, P):
    """the same, one row at a time in plain integers: count, lay the groups out, then deal the rows in index order"""
    values = [int(v) for v in np.asarray(members).tolist()]
    n = len(values)
    count = [0] * P
    errors = 0
    for v in values:
        if 0 <= v < P:
            count[v] += 1
        else:
            errors += 1
    first = [0]
    for p in range(P):
        first.append(first[p] + (count[p] + G - 1) // G * G)
    order = [-1] * ((n // G + P) * G)
    nxt = list(first[:P])
    for i, v in enumerate(values):
        if 0 <= v < P:
            order[nxt[v]] = i
            nxt[v] += 1
    return order, first, errors


def member_vector(kind, n, P, seed=0):
    """int64 VALUES of one of the GPU test's member vectors (``typed`` gives them a format).  ``every_count_1_mod_g`` has a
    length of its own, P + G * (n // G): the nearest size at which every count can be 1 mod G, where the capacity bound is met
    with equality."""
    rng = np.random.default_rng([seed, n, P, MEMBER_KINDS.index(kind)])
    drawn = rng.integers(0, P, n)
    if kind == "all_one_member":
        return np.full(n, P - 1, np.int64)
    if kind == "one_member_empty":
        empty = P // 2
        return np.where(drawn == empty, (empty + 1) % P, drawn).astype(np.int64)
    if kind == "every_count_1_mod_g":
        groups = rng.multinomial(n // G, np.full(P, 1.0 / P))
        return rng.permutation(np.repeat(np.arange(P), 1 + G * groups)).astype(np.int64)
    if kind == "round_robin":
        return (np.arange(n) % P).astype(np.int64)
    if kind == "sorted":
        return np.sort(drawn).astype(np.int64)
    if kind == "reverse_sorted":
        return np.sort(drawn)[::-1].astype(np.int64)
    assert kind == "invalid_entries"
    out = drawn.astype(np.int64)
    bad = rng.random(n) < 0.2
    bad[rng.integers(0, n)] = True
    out[bad] = rng.choice(np.array([-1, P, 255, 1 << 32, -(1 << 31)]), int(bad.sum()))
    return out


def invalid_for(values, dtype):
    """the invalid entries of ``invalid_entries`` stay invalid in every format: 2^32 and -2^31 have a low byte (and 2^32 a low
    word) of 0, which would name member 0, so the narrower formats get 255 in their place"""
    v = np.asarray(values, np.int64).copy()
    if dtype == "uint8":
        v[(v == 1 << 32) | (v == -(1 << 31))] = 255
    elif dtype == "int32":
        v[v == 1 << 32] = 255
    return typed(v, dtype)


def plan_cases(n):
    """[(kind, P, dtype, typed members)] of one n of the GPU test: every kind x P, the formats rotated over them (all three at
    ``invalid_entries``, where they differ)"""
    out = []
    turn = 0
    for P in PLAN_P:
        for kind in MEMBER_KINDS:
            values = member_vector(kind, n, P)
            dtypes = MEMBER_DTYPES if kind in ("invalid_entries", "round_robin") else (MEMBER_DTYPES[turn % 3],)
            turn += 1
            for dtype in dtypes:
                out.append((kind, P, dtype, invalid_for(values, dtype)))
    return out


# ---- the forward ---------------------------------------------------------------------------------------------------------------
def effective_members(members, P, mutant=None, other=None):
    """per row the member whose parameters it runs on, -1 for a row that is not written.  ``members`` None: an unplanned
    agent, member 0 everywhere.  ``other``: the other agent's typed member vector (for the mutant that reads it)."""
    if mutant == "agent_2_through_agent_1_plan" and other is not None:
        members = other
    if members is None:
        return None
    m = np.asarray(members).astype(np.int64)
    valid = valid_rows(members, P)
    eff = np.where(valid, m, -1)
    if mutant == "next_member_parameters":
        eff = np.where(valid, (m + 1) % P, -1)
    elif mutant == "invalid_clamped_to_zero":
        eff = np.where(valid, m, 0)
    elif mutant == "invalid_clamped_to_last":
        eff = np.where(valid, m, P - 1)
    return eff


def judge(obs, member_params, eff, activation, out_dtype="float32"):
    """(head [n, O] float64, tolerance [n, O]) with every row judged under the parameters of member eff[row]; rows with
    eff = -1 are NaN in both (they are expected to keep the sentinel, which the caller checks).  eff None: member 0."""
    obs = np.asarray(obs)
    n = obs.shape[0]
    O = member_params[0][4].shape[0]
    eff = np.zeros(n, np.int64) if eff is None else eff
    ref, tol = np.full((n, O), np.nan), np.full((n, O), np.nan)
    for p in np.unique(eff[eff >= 0]):
        rows = np.flatnonzero(eff == p)
        ref[rows], tol[rows] = N.judge(obs[rows], member_params[p], activation, out_dtype)
    return ref, tol


def forward_cases():
    """The forward cases of the GPU test: sizes, activation, formats, n, P, pitches above the widths, a base offset, and per
    agent the kind of its member vector (None: that agent passes no plan and runs on member 0).  One and two agents, agent 1
    unplanned beside a planned agent 2, and one case large enough that a workgroup holds several groups and re-stages."""
    c = lambda **kw: dict(dict(K=35, H=64, O=19, activation="tanh", obs_dtype="float32", out_dtype="float32", n=257, P=3, obs_extra=0, out_extra=0,  # noqa: E731
                               offset=0, kinds=("round_robin", "invalid_entries")), **kw)
    return [
        c(obs_extra=3, out_extra=2, offset=1),
        c(activation="relu", obs_dtype="int32", out_dtype="bfloat16", n=129, P=16, kinds=("every_count_1_mod_g", "reverse_sorted")),
        c(K=1, H=32, O=1, obs_dtype="float16", out_dtype="float16", n=33, P=2, kinds=("one_member_empty",), out_extra=1, offset=1),
        c(K=1, H=32, O=1, activation="relu", n=127, P=3, kinds=("invalid_entries", "sorted")),
        c(K=72, H=128, O=40, n=4099, P=4, kinds=(None, "invalid_entries"), obs_extra=1),
        c(K=72, H=128, O=40, activation="relu", obs_dtype="bfloat16", n=130, P=3, kinds=("sorted", "round_robin"), out_extra=3),
        c(obs_dtype="int16", n=4099, P=16, kinds=("invalid_entries", "one_member_empty")),
        c(n=128, P=1, kinds=("all_one_member", None)),
        c(n=40000, P=16, kinds=("invalid_entries", "round_robin")),          # more groups than resident workgroups: re-staging
        # Sized for a grid cap of at most 256 compute units (`max_cus`, which the GPU test asserts).  H = 128 holds one
        # workgroup per compute unit, two agents share them: at most 128 workgroups for the unplanned side's 157 groups of
        # all rows, so some workgroups walk two groups with order == NULL ...
        c(K=72, H=128, O=40, n=20000, P=3, kinds=(None, "sorted"), obs_extra=1, out_extra=2, offset=1, max_cus=256),
        # ... and H = 32, two workgroups per compute unit: at most 256 for 313 plain groups and as many planned ones
        c(H=32, activation="relu", obs_dtype="float16", n=40000, P=4, kinds=("reverse_sorted", None), obs_extra=2, out_extra=1, offset=1,
          max_cus=256),
    ]


def case_members(case, dtype_turn=0):
    """per agent the typed member vector of a forward case, or None (the vectors of the two agents differ).  Their length is
    the case's n: ``every_count_1_mod_g`` is cut or filled with member 0 to it."""
    out = []
    for s, kind in enumerate(case["kinds"]):
        if kind is None:
            out.append(None)
            continue
        v = member_vector(kind, case["n"], case["P"], seed=7 + s)
        if len(v) != case["n"]:
            v = np.concatenate([v, np.zeros(case["n"], np.int64)])[:case["n"]]
        out.append(invalid_for(v, MEMBER_DTYPES[(dtype_turn + s) % 3]))
    return out


def case_inputs(case, seed=0):
    """(per agent [n, K] observations, the P parameter sets) of a forward case"""
    obs = [N.make_obs(case["n"], case["K"], case["obs_dtype"], 100 + seed + s) for s in range(len(case["kinds"]))]
    params = [N.make_params(case["K"], case["H"], case["O"], 200 + seed + p) for p in range(case["P"])]
    return obs, params
