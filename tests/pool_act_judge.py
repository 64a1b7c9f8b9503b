"""The judge of the pool-act launch (include/pikazoo_pool_act.h: ``pz_mlp_act_pool``).  It holds NO expected GPU values and no
arithmetic of its own: the header defines the launch by reference to pz_mlp_forward_pool and pz_sample_actions, and this file
composes their judges -- tests/pool_judge.py (``effective_members``: which member's parameters a row runs on and which rows
are written at all; ``judge``; ``member_vector``) with tests/act_judge.py's ``verdict`` (policy_judge on the launch's OWN
logits, net_judge's derived tolerance on the head, the value bit for bit).

HOW A LAUNCH IS JUDGED (``verdict``).  Per agent: the rows that were written are exactly those whose member is valid (an
unplanned agent: all of them); then, member by member, the rows of that member go through ``act_judge.verdict`` under that
member's parameters with the uniforms of their own GLOBAL game ids first_game + row.  An agent that was launched without its
statistics is judged on its head and its action alone (``verdict_actions``: the same lines of act_judge.verdict).  The cap on
ambiguous rows is act_judge.CAP, held per member's rows by act_judge.verdict and once more over the agent's n rows here.

THE FLOAT32 RESTATEMENT (``restate_float32``) chains net_judge.restate_float32 per member with policy_judge.restate_float32,
and plays the kernel for the mutants of the seams this launch adds: which member, which rows, which game id, which word,
which column, and the statistics switch.  tests/test_pool_act_host.py holds it to the float64 composition on every case, shows
that every mutant fails on the GPU test's own cases, and prints the shares of ambiguous rows.

THE CASES of tests/test_gpu_pool_act.py are made here (``cases``), the smallest shapes at which this kernel can go wrong.
"""
import numpy as np

import act_judge as AJ
import net_judge as N
import policy_judge as J
import pool_judge as PJ

MUTANTS = ("next_member_parameters", "invalid_clamped_to_zero", "agent_2_through_agent_1_plan", "global_id_is_the_slot_not_the_row",
           "words_swapped", "value_from_column_A_minus_1", "stats_off_changes_the_action")

N_EDGES = (1, 31, 32, 33, 127, 128, 129, 257, 4099)   # around one tile and one group of four; two groups and a row; 33 groups
P_EDGES = (1, 3, 16)
SIZES = ((35, 32, 19, 18), (36, 64, 14, 13), (72, 128, 33, 32), (8, 32, 2, 2))   # (K, H, O, A) beside the default; the last: no value
MEMBER_KINDS = ("round_robin", "invalid_entries", "one_member_empty", "every_count_1_mod_g", "reverse_sorted")
# act_judge.DRAWS (the plain one, a first_game and a step beyond 2^32, a step carried by step_dev) and the last one by value
DRAWS = AJ.DRAWS + ((AJ.DRAWS[2][0], AJ.DRAWS[2][1], AJ.DRAWS[2][2] + AJ.DRAWS[2][3], None),)
CAP = AJ.CAP


def cases():
    """The cases of the GPU test.  ``kinds``: per agent the kind of its member vector, None for an agent that passes no plan
    (member 0 everywhere); ``turn``: which member dtype agent 1 takes (agent 2 the next); ``stats``: per agent whether
    log_probs, entropy and values are asked for; ``head_extra`` / ``offset``: the head's pitch above O and the base offset of
    every buffer, in elements; ``draw``: index into DRAWS."""
    c = lambda **kw: dict(dict(K=35, H=64, O=19, A=18, activation="tanh", obs_dtype="float32", action_dtype="int64", n=257, P=3,  # noqa: E731
                               kinds=(None, "round_robin"), turn=0, stats=(True, True), obs_extra=0, head_extra=0, offset=0, draw=0, seed=0), **kw)
    out = []
    # every edge of n x P in {1, 3, 16}: agent 1 unplanned beside a planned agent 2, and both planned, in turn
    for i, n in enumerate(N_EDGES):
        for j, P in enumerate(P_EDGES):
            kinds = (None, "invalid_entries") if (i + j) % 2 == 0 else ("round_robin", "reverse_sorted")
            out.append(c(n=n, P=P, kinds=kinds, turn=i + j, draw=(i + j) % 3, seed=len(out)))
    # the other sizes, tanh and relu, at a head pitch above O and a base offset
    for size in SIZES:
        for activation in N.ACTIVATIONS:
            K, H, O, A = size
            out.append(c(K=K, H=H, O=O, A=A, activation=activation, n=129, kinds=("one_member_empty", "round_robin"), obs_extra=3, head_extra=2,
                         offset=1, draw=1, seed=len(out)))
    # the five observation formats into both action formats
    for obs_dtype in N.OBS_DTYPES:
        for action_dtype in J.ACTION_DTYPES:
            out.append(c(obs_dtype=obs_dtype, action_dtype=action_dtype, activation="relu" if obs_dtype.startswith("int") else "tanh", n=65,
                         kinds=("round_robin", "invalid_entries"), obs_extra=1, offset=1, seed=len(out)))
    # the member kinds in the three member dtypes: one agent only, agent 1 unplanned beside agent 2, both planned
    for kind in MEMBER_KINDS:
        for turn, kinds in ((0, (kind,)), (0, (None, kind)), (2, (kind, kind))):   # uint8; int32 for agent 2; int64 and uint8
            out.append(c(kinds=kinds, turn=turn, head_extra=turn, seed=len(out)))
    # the draws: by value, beyond 2^32, through step_dev, and that one by value
    for draw in range(len(DRAWS)):
        out.append(c(n=129, kinds=("round_robin", "round_robin"), draw=draw, seed=len(out)))
    # the statistics switched off: the league's call, its mirror image, both, and one agent alone
    out.append(c(stats=(True, False), kinds=(None, "invalid_entries"), draw=2, seed=len(out)))
    out.append(c(stats=(False, True), kinds=("reverse_sorted", None), P=16, seed=len(out)))
    out.append(c(stats=(False, False), kinds=("round_robin", "one_member_empty"), draw=1, seed=len(out)))
    out.append(c(stats=(False,), kinds=("invalid_entries",), n=129, seed=len(out)))
    # re-staging, sized as in pool_judge.forward_cases(): more groups than resident workgroups, so a workgroup walks several
    # groups and crosses member boundaries; and H = 128 at the largest net, one workgroup per compute unit shared by two agents:
    # at most 128 workgroups (for `max_cus` = 256 compute units, which the GPU test asserts) for the unplanned side's 157 groups
    out.append(c(n=40000, P=16, kinds=("invalid_entries", "round_robin"), stats=(True, False), seed=len(out)))
    out.append(c(K=72, H=128, O=40, A=32, n=20000, P=3, kinds=(None, "sorted"), obs_extra=1, head_extra=2, offset=1, max_cus=256, draw=1,
                 seed=len(out)))
    return out


def wide_case():
    """(the case, observations, parameters, members) of tests/test_gpu_wide_pitch.py: 40 rows 2^31 elements apart, float16
    observations, three members round-robin for both agents (int32 and int64 member vectors), and per agent one row of an
    invalid member -- agent 1's below the limit, agent 2's behind it.  act_judge.CAP(40) is one row; the draw and the seed are
    picked so that the float32 restatement has no ambiguous row at all (tests/test_pool_act_host.py asserts it)."""
    case = dict(K=35, H=64, O=19, A=18, activation="relu", obs_dtype="float16", action_dtype="int64", n=40, P=3, kinds=("round_robin", "round_robin"),
                turn=1, stats=(True, True), obs_extra=0, head_extra=0, offset=0, draw=2, seed=70)
    obs, params = case_inputs(case)
    members = case_members(case)
    members[0][5], members[1][38] = -1, -1
    return case, obs, params, members


def case_members(case):
    """per agent the typed member vector of a case, or None"""
    return PJ.case_members(case, case["turn"])


def case_inputs(case):
    """(per agent [n, K] observations, the P parameter sets) of a case"""
    return PJ.case_inputs(case, seed=case["seed"])


def uniforms(case):
    """u[2, n]: the header's Philox block for the global game ids first_game + row of the case's draw"""
    seed, first_game, step, step_dev = DRAWS[case["draw"]]
    return J.uniforms(seed, first_game, step, step_dev, case["n"])


def effective(case, members, s, mutant=None):
    """(the member each row of agent s runs on, the rows that are written)"""
    eff = PJ.effective_members(members[s], case["P"], mutant=mutant if mutant in PJ.FORWARD_MUTANTS else None, other=members[0] if s == 1 else None)
    eff = np.zeros(case["n"], np.int64) if eff is None else eff
    return eff, eff >= 0


# ---- the definition in float64 ----------------------------------------------------------------------------------------------
def judge(case, obs, params, members):
    """per agent (head [n, O] float64, its tolerance, action [n], ambiguous [n], written [n]): pool_judge.judge followed by
    policy_judge.sample on ITS head; rows that are not written are NaN in the head and carry no meaning elsewhere"""
    us = uniforms(case)
    out = []
    for s, x in enumerate(obs):
        eff, written = effective(case, members, s)
        head, tol = PJ.judge(x, params, eff, case["activation"])
        a, amb, _, _ = J.sample(np.where(written[:, None], head[:, :case["A"]], 0.0), us[s])
        out.append((head, tol, a, amb, written))
    return out


# ---- the float32 restatement, which also plays the kernel for the mutants ------------------------------------------------------
def restate_float32(case, obs, params, members, mutant=None):
    """per agent a dict (written [n] bool, head float32 [n, O], actions, and log_probs, entropy, values or None where the
    case does not ask for the agent's statistics): net_judge's float32 chain under each row's member, then policy_judge's"""
    n, P, A, O = case["n"], case["P"], case["A"], case["O"]
    seed, first_game, step, step_dev = DRAWS[case["draw"]]
    us = J.uniforms(seed, first_game, step, step_dev, n, mutant=mutant if mutant == "words_swapped" else None)
    out = []
    for s, x in enumerate(obs):
        eff, written = effective(case, members, s, mutant)
        head = np.zeros((n, O), np.float32)
        for p in np.unique(eff[written]):
            rows = np.flatnonzero(eff == p)
            head[rows] = N.restate_float32(x[rows], params[p], case["activation"])
        u = us[s]
        if mutant == "global_id_is_the_slot_not_the_row" and members[s] is not None:  # G from the position in `order`
            order, _, _ = PJ.plan(members[s], P)
            slot_of = np.zeros(n, np.int64)
            slot_of[order[order >= 0]] = np.flatnonzero(order >= 0)
            u = np.where(written, J.uniforms(seed, first_game, step, step_dev, len(order))[s][slot_of], u)
        a, logp, ent = J.restate_float32(head[:, :A], u)
        on = case["stats"][s]
        if mutant == "stats_off_changes_the_action" and not on:  # (the sums of steps 1 and 2 skipped with the statistics: S = 0)
            a = np.zeros_like(a)
        val = None
        if O > A and on:
            val = head[:, A - 1] if mutant == "value_from_column_A_minus_1" else head[:, A]
        out.append(dict(written=written, head=head, actions=a, log_probs=logp if on else None, entropy=ent if on else None, values=val))
    return out


def verdict_actions(got, obs, params, activation, A, u, what=""):
    """act_judge.verdict's lines for an agent launched without its statistics: the head within net_judge's tolerance, and on
    the launch's own logits an unambiguous row returns the judge's action, an ambiguous one a live action between its
    neighbours.  Returns (the number of ambiguous rows, the failures)."""
    head = np.asarray(got["head"], np.float32)
    n = head.shape[0]
    act = np.asarray(got["actions"], np.int64)
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
    if int(amb.sum()) > CAP(n):
        fails.append(f"{what}: {int(amb.sum())} ambiguous rows, above the cap of {CAP(n)}")
    return int(amb.sum()), fails


def verdict(case, got, obs, params, members, what=""):
    """The outputs of one launch -- per agent a dict as ``restate_float32`` returns it (the head asked for on both agents) --
    against the judge, as the module docstring says.  Returns (ambiguous rows per agent, the failures: empty for a pass)."""
    us = uniforms(case)
    ambiguous, fails = [], []
    for s, x in enumerate(obs):
        eff, written = effective(case, members, s)
        g = got[s]
        if not np.array_equal(np.asarray(g["written"], bool), written):
            fails.append(f"{what} side {s}: rows of valid members must be written and rows of invalid members must not: "
                         f"{int((np.asarray(g['written'], bool) != written).sum())} rows differ")
            ambiguous.append(0)
            continue
        on = case["stats"][s]
        if on != (g["log_probs"] is not None) or on != (g["entropy"] is not None) or (on and case["O"] > case["A"]) != (g["values"] is not None):
            fails.append(f"{what} side {s}: the statistics are there exactly where they are asked for")
            ambiguous.append(0)
            continue
        total = 0
        for p in np.unique(eff[written]):
            rows = np.flatnonzero(eff == p)
            sub = {k: (np.asarray(v)[rows] if v is not None else None) for k, v in g.items() if k != "written"}
            run = AJ.verdict if on else verdict_actions
            count, f = run(sub, x[rows], params[p], case["activation"], case["A"], us[s][rows], what=f"{what} side {s} member {int(p)}")
            total += count
            fails += f
        if total > CAP(case["n"]):
            fails.append(f"{what} side {s}: {total} ambiguous rows, above the cap of {CAP(case['n'])}")
        ambiguous.append(total)
    return ambiguous, fails
