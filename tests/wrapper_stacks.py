"""Every wrapper stack of depth one to four: the table, the run recipe, the judge's replay and the comparison rule.

Pure data and numpy -- no GPU, no torch.  Three users share it, so that they cannot drift apart:

* ``oracle/ref_capture.capture_stack_sweep`` runs the unmodified reference on every stack of the table and records its
  results (``tests/golden/stack_sweep_*.npz``);
* ``tests/test_wrapper_stacks_host.py`` pins ``oracle.wrappers_oracle.WrappedOracle`` to those recordings on every stack
  and shows that the cases bite;
* ``tests/test_gpu_wrapper_stacks.py`` steps the product's wrapper classes against ``WrappedOracle`` by :func:`mismatches`.

The table
---------
Alphabet (innermost first, with repetition): RewardByBallPosition, RewardInNormalState, NormalizeObservation,
RecordEpisodeStatistics -- 4 + 16 + 64 + 256 = 340 stacks.  ``SimplifyAction`` commutes with all four; stack k gets it at
the place ``k % 4`` says: absent, innermost, in the middle, outermost.

Parameters, so that instances can be told apart and every instance has work to do:

* the i-th RewardByBallPosition of a stack takes ``BALLPOS_SETS[i]``.  ``oracle.ref_capture.TEST_TABLE`` (216 / 176) and
  ``INT_TABLE`` (200 / 150) are the third and the fourth set; the first two are tables of distinct dyadic values (sums of
  them are exact in float32 and float64 alike) built so that sums of the sets can be exactly 0:

  - both hold a 0 for player_1 in zone 0, ``ZERO_TABLE`` pays player_1 +1 / -1 in the two zones a rally ends in (the ball
    on the ground left / right of x = 216: a lost / won point, -1 + 1 == 0 == 1 - 1), and both hold -0.25, which cancels
    the first RewardInNormalState's +0.25.  Without that a RewardInNormalState above them would never see a 0 again.
  - an instance above a NormalizeObservation compares the NORMALIZED coordinates: it gets the set's lines inside (0, 1);
    an instance below every NormalizeObservation keeps the integer lines.

* the i-th RewardInNormalState takes ``NORMAL_REWARDS[i]``.

What no choice of parameters can give: a RewardInNormalState above another one with no RewardByBallPosition between the
two never sees a 0 (the lower one left none), in the reference as here.  :func:`shadowed` names those instances, and the
host test asserts that they replace NOTHING and every other instance something.
"""
from __future__ import annotations

import functools
import itertools
import math

import numpy as np

ALPHABET = ("RewardByBallPosition", "RewardInNormalState", "NormalizeObservation", "RecordEpisodeStatistics")
SHORT = {"RewardByBallPosition": "B", "RewardInNormalState": "N", "NormalizeObservation": "O",
         "RecordEpisodeStatistics": "S", "SimplifyAction": "A"}
REWARD_WRAPPERS = ("RewardByBallPosition", "RewardInNormalState")

TEST_TABLE = (0.0, -0.01, 0.0, 0.01, 0.0, 0.01, 0.0, -0.01)   # oracle.ref_capture.TEST_TABLE
INT_TABLE = (1, -2, 3, -4, 5, -6, 7, -8)                       # oracle.ref_capture.INT_TABLE
ZERO_TABLE = (0.0, 1.0, -0.25, -1.0, -0.5, 0.75, 0.125, -0.375)
DYADIC_TABLE = (0.0, -0.75, -0.25, 2.0, 0.5, 1.5, -0.625, 0.875)
# (table, integer x_line, y_line, the lines an instance above a NormalizeObservation gets)
BALLPOS_SETS = (
    (ZERO_TABLE, 232, 120, 0.625, 0.5),
    (DYADIC_TABLE, 184, 208, 0.375, 0.25),
    (TEST_TABLE, 216, 176, 0.5, 0.7),
    (INT_TABLE, 200, 150, 0.25, 0.75),
)
NORMAL_REWARDS = (0.25, -0.5, 0.125, -0.002)

# the run recipe: the smallest batch with a whole wave and a ragged tail, one-point games (an episode is one rally of some
# 50 frames), and the smallest T (a multiple of 10) at which tests/test_wrapper_stacks_host.py's coverage conditions hold
# on the oracle -- on the batch (from T = 50) AND on the four games the reference was recorded on (from T = 70), so that
# the recordings show the reference itself doing everything the conditions name
NUM_ENVS = 64 + 5
FIXTURE_LANES = 4          # the reference runs the first four games of the batch
RECIPE = dict(winning_score=1, seed=20260117, env_id_base=4100, action_seed=59, T=70)

ACTION_MAP = ((0, 1, 2, 3, 4, 6, 7, 10, 11, 12, 13, 14, 16), (0, 1, 2, 4, 3, 7, 6, 10, 12, 11, 13, 15, 17))
# pikazoo_env.py:485-562 (player, opponent, ball)
_PLAYER_LOW = [32, 108, -15, -1, -2, 0, 0, 0, 0, 0, 0, 0, 0]
_PLAYER_HIGH = [400, 244, 16, 1, 3, 4, 4, 1, 1, 1, 1, 1, 1]
OBS_LOW = np.array(_PLAYER_LOW * 2 + [20, 0, 0, 0, 0, 0, -20, -124, 0], dtype=np.float64)
OBS_HIGH = np.array(_PLAYER_HIGH * 2 + [432, 252, 432, 252, 432, 252, 20, 124, 1], dtype=np.float64)


# --------------------------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_names():
    """The 340 stacks as tuples of class names, innermost first: by depth, then in the alphabet's order."""
    return tuple(s for depth in (1, 2, 3, 4) for s in itertools.product(ALPHABET, repeat=depth))


def with_parameters(names):
    """[(class name, kwargs)] of a tuple of alphabet names (no SimplifyAction yet)."""
    out, n_ball, n_normal, normalized = [], 0, 0, False
    for name in names:
        kw = {}
        if name == "RewardByBallPosition":
            table, x_line, y_line, x_norm, y_norm = BALLPOS_SETS[n_ball]
            kw = dict(additional_reward=list(table), x_line=x_norm if normalized else x_line,
                      y_line=y_norm if normalized else y_line)
            n_ball += 1
        elif name == "RewardInNormalState":
            kw = dict(reward=NORMAL_REWARDS[n_normal])
            n_normal += 1
        elif name == "NormalizeObservation":
            normalized = True
        out.append((name, kw))
    return out


def simplify_place(k, depth):
    """Where stack k gets its SimplifyAction: None (absent), or the index it is inserted at."""
    return (None, 0, (depth + 1) // 2, depth)[k % 4]


def insert_simplify(stack, k):
    place = simplify_place(k, len(stack))
    stack = list(stack)
    if place is not None:
        stack.insert(place, ("SimplifyAction", {}))
    return stack


@functools.lru_cache(maxsize=None)
def _stacks():
    return tuple(tuple(insert_simplify(with_parameters(names), k)) for k, names in enumerate(all_names()))


def stack(k):
    """Stack k of the table: [(class name, kwargs), ...] innermost first, SimplifyAction included."""
    return [(n, dict(kw)) for n, kw in _stacks()[k]]


def n_stacks():
    return len(all_names())


def label(st):
    return "".join(SHORT[n] for n, _ in st)


def simplified(st):
    return any(n == "SimplifyAction" for n, _ in st)


def n_normalize(st):
    return sum(n == "NormalizeObservation" for n, _ in st)


def has_stats(st):
    return any(n == "RecordEpisodeStatistics" for n, _ in st)


def groups():
    """The GPU sweep's parametrisation: stacks by their two innermost alphabet wrappers (16 groups of 1 + 4 + 16), and
    the four stacks of depth one."""
    out = {"depth1": [k for k, names in enumerate(all_names()) if len(names) == 1]}
    for k, names in enumerate(all_names()):
        if len(names) >= 2:
            out.setdefault(SHORT[names[0]] + SHORT[names[1]], []).append(k)
    return out


def shadowed(st):
    """Indices (into `st`) of the RewardInNormalState instances that can never see a 0: another one sits below with no
    RewardByBallPosition between the two."""
    out, zeros_possible = [], True
    for p, (name, _) in enumerate(st):
        if name == "RewardByBallPosition":
            zeros_possible = True
        elif name == "RewardInNormalState":
            if not zeros_possible:
                out.append(p)
            zeros_possible = False
    return out


# --------------------------------------------------------------------------------------------------------------------
# tolerances
# --------------------------------------------------------------------------------------------------------------------
def reward_error_bound(st):
    """How far a float32 evaluation of the stack's reward wrappers, in the stack's order, can be from the reference's
    float64 one, per step.

    The product computes every reward wrapper in float32 (in the kernel or with torch on its outputs); the reference in
    float64 (whose own rounding, 1e-16 relative, is ignored).  Let M bound the magnitude so far (1 for the env's -1 / 0 /
    +1) and e the error so far (0: integers).

    * RewardByBallPosition adds a table entry t: the float32 entry is within |t| * 2^-24 of t, and the float32 sum is
      rounded once more, by at most half an ulp of a float32 of the new magnitude M + max|t|:
      ``e += max|t| * 2^-24 + 2^(floor(log2 M') - 24)``.
    * RewardInNormalState replaces exact zeros by r: a replaced reward is within |r| * 2^-24 of r, the others keep e:
      ``e = max(e, |r| * 2^-24)``.  (Both sides replace the SAME rewards: every value the sets above can produce is a
      multiple of 1/8 plus at most one of 0, +-0.01, -0.002, so a non-zero one is at least 0.002 -- four orders above e.)

    The bound is not tight (sums of dyadic values are exact); it is what the number formats guarantee."""
    m, e = 1.0, 0.0
    for name, kw in st:
        if name == "RewardByBallPosition":
            t = max(abs(float(v)) for v in kw["additional_reward"])
            m += t
            e += t * 2.0 ** -24 + 2.0 ** (math.floor(math.log2(m)) - 24)
        elif name == "RewardInNormalState":
            r = abs(float(kw["reward"]))
            m = max(m, r)
            e = max(e, r * 2.0 ** -24)
    return e


def tolerances(st):
    """(reward atol, per-step error of an episode return) of a stack.

    The rule tests/test_gpu_parity.py::test_wrapper_stacks_the_kernel_cannot_fuse_match_the_reference uses -- rewards
    within 1e-6, returns within rtol 1e-7 + atol 2e-6 -- holds wherever :func:`reward_error_bound` stays below it; the
    stacks that add up to four tables (magnitudes up to 12, half an ulp 4.8e-7, several roundings) get their own bound
    instead.  An episode return is a float64 sum of l rewards, each within the per-step bound: atol = max(2e-6, l * e)."""
    e = reward_error_bound(st)
    return max(1e-6, e), e


def mismatches(st, got, want, *, float_obs=None):
    """THE comparison rule: a product run `got` against the judge's run `want` of stack `st`.  Both are dicts of numpy
    arrays with a leading time axis (or without: one step): ``state`` int [.., 44, n], ``term`` [.., n], ``obs``
    [.., 2, n, 35] (`want`: the float64 rows), ``rew`` [.., 2, n] and, with statistics in the stack, ``ep_l`` [.., n] and
    ``ep_r`` [.., 2, n] -- compared where ``want["ep_mask"]`` (bool [.., n], default: everywhere) says so.

    * state words and terminations equal;
    * observations equal to the float32 rounding of the float64 rows (integer rows: equal);
    * rewards within :func:`tolerances` (no reward wrapper: equal);
    * episode lengths equal, episode returns within rtol 1e-7 + max(2e-6, l * e).

    Returns the list of what differs (empty: the runs agree)."""
    out = []
    if "state" in got and not np.array_equal(got["state"], want["state"]):
        out.append("state words differ")
    if not np.array_equal(np.asarray(got["term"]).astype(np.uint8), np.asarray(want["term"]).astype(np.uint8)):
        out.append("terminations differ")
    normalized = n_normalize(st) > 0 if float_obs is None else float_obs
    g_obs = np.asarray(got["obs"])
    if normalized:
        if g_obs.dtype != np.float32 or not np.array_equal(g_obs, np.asarray(want["obs"]).astype(np.float32)):
            out.append("observations differ from the float32 rounding of the float64 rows")
    elif g_obs.dtype.kind != "i" or not np.array_equal(g_obs, np.asarray(want["obs"]).astype(np.int64)):
        out.append("integer observations differ")
    atol, e = tolerances(st)
    g_rew, w_rew = np.asarray(got["rew"]).astype(np.float64), np.asarray(want["rew"], np.float64)
    if not any(n in REWARD_WRAPPERS for n, _ in st):
        if np.asarray(got["rew"]).dtype.kind != "i" or not np.array_equal(g_rew, w_rew):
            out.append("integer rewards differ")
    elif not (np.abs(g_rew - w_rew) <= atol).all():
        out.append(f"rewards differ by {np.abs(g_rew - w_rew).max():.3g} > {atol:.3g}")
    if has_stats(st):
        mask = np.asarray(want.get("ep_mask", np.ones(np.shape(want["ep_l"]), bool)))
        g_l, w_l = np.asarray(got["ep_l"]).astype(np.int64), np.asarray(want["ep_l"]).astype(np.int64)
        if not np.array_equal(g_l[mask], w_l[mask]):
            out.append("episode lengths differ")
        m2 = np.broadcast_to(np.expand_dims(mask, -2), np.shape(want["ep_r"]))
        l2 = np.broadcast_to(np.expand_dims(w_l, -2), np.shape(want["ep_r"]))
        g_r, w_r = np.asarray(got["ep_r"], np.float64), np.asarray(want["ep_r"], np.float64)
        bound = 1e-7 * np.abs(w_r) + np.maximum(2e-6, l2 * e)
        bad = m2 & ~(np.abs(g_r - w_r) <= bound)
        if bad.any():
            out.append(f"episode returns differ by {np.abs(g_r - w_r)[bad].max():.3g} (bound {bound[bad].min():.3g})")
    return out


# --------------------------------------------------------------------------------------------------------------------
# the judge's runs: the un-wrapped oracle once per action space, every stack replayed on top of it
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_run(num_envs, simplify, T=None):
    """The un-wrapped C oracle on the recipe, stepped with the policy stream of 13 (`simplify`) or 18 actions -- the
    13 mapped through SimplifyAction's tables, which is all that wrapper does.  Arrays (read-only, shared by every stack):
    ``obs0`` [2, n, 35], ``actions`` [T, 2, n] (as the policy drew them), ``mapped`` (as the env saw them), ``obs``
    [T, 2, n, 35], ``rew`` [T, 2, n], ``term`` [T, n], ``state_ctor`` / ``state0`` [44, n], ``state`` [T, 44, n]."""
    from oracle import pz_oracle as po

    po.build()
    T = RECIPE["T"] if T is None else T
    env = po.OracleEnv(num_envs, po.make_config(auto_reset=True, winning_score=RECIPE["winning_score"],
                                                seed=RECIPE["seed"], env_id_base=RECIPE["env_id_base"]))
    run = dict(state_ctor=env.state.copy())
    run["obs0"] = np.stack([o.copy() for o in env.reset()]).astype(np.int64)
    run["state0"] = env.state.copy()
    n_actions = 13 if simplify else 18
    for key, shape, dt in (("actions", (T, 2, num_envs), np.int32), ("mapped", (T, 2, num_envs), np.int32),
                           ("obs", (T, 2, num_envs, 35), np.int64), ("rew", (T, 2, num_envs), np.int64),
                           ("term", (T, num_envs), np.uint8), ("state", (T, 44, num_envs), np.int32)):
        run[key] = np.zeros(shape, dt)
    for t in range(T):
        a = np.stack(po.random_actions(num_envs, RECIPE["env_id_base"], RECIPE["action_seed"], t, n_actions))
        m = np.stack([np.array(ACTION_MAP[i], np.int32)[a[i]] for i in range(2)]) if simplify else a
        obs, rew, term = env.step(m[0].astype(np.int32), m[1].astype(np.int32))
        run["actions"][t], run["mapped"][t] = a, m
        run["obs"][t, 0], run["obs"][t, 1] = obs
        run["rew"][t, 0], run["rew"][t, 1] = rew
        run["term"][t], run["state"][t] = term, env.state
    for v in run.values():
        v.setflags(write=False)
    return run


class ReplayEnv:
    """``raw_run`` behind the interface ``WrappedOracle`` drives (``reset`` / ``step`` / ``state``): every stack of the
    sweep runs on the SAME un-wrapped trajectory, computed once.  ``step`` insists on the recorded actions."""

    def __init__(self, run):
        self.run, self.t = run, -1
        self.state = run["state_ctor"].copy()

    def reset(self):
        assert self.t == -1, "a replay starts with its one reset()"
        self.state = self.run["state0"].copy()
        return self.run["obs0"][0], self.run["obs0"][1]

    def step(self, a1, a2):
        self.t += 1
        run, t = self.run, self.t
        assert np.array_equal(a1, run["mapped"][t, 0]) and np.array_equal(a2, run["mapped"][t, 1]), \
            "the stack handed the env other actions than the recorded ones"
        self.state = run["state"][t].copy()
        return (run["obs"][t, 0], run["obs"][t, 1]), (run["rew"][t, 0], run["rew"][t, 1]), run["term"][t]


def judge(st, num_envs, T=None):
    """``WrappedOracle`` of stack `st` on the recipe's shared un-wrapped run, and that run."""
    from oracle.wrappers_oracle import WrappedOracle

    run = raw_run(num_envs, simplified(st), T)
    return WrappedOracle(num_envs, st, env=ReplayEnv(run)), run


def judge_run(st, num_envs, T=None):
    """The whole run of :func:`judge` as arrays with a leading time axis (what :func:`mismatches` takes as `want`), plus
    ``obs0`` [2, n, 35] float64."""
    env, run = judge(st, num_envs, T)
    T = run["term"].shape[0]
    stats = has_stats(st)
    out = dict(obs0=np.stack(env.reset()), state=run["state"], obs=np.zeros((T, 2, num_envs, 35)),
               rew=np.zeros((T, 2, num_envs)), term=np.zeros((T, num_envs), np.uint8))
    if stats:
        out.update(ep_r=np.zeros((T, 2, num_envs)), ep_l=np.zeros((T, num_envs), np.int64))
    for t in range(T):
        obs, rew, term, episode = env.step(run["actions"][t, 0], run["actions"][t, 1])
        out["obs"][t, 0], out["obs"][t, 1] = obs
        out["rew"][t, 0], out["rew"][t, 1] = rew
        out["term"][t] = term
        if stats:
            out["ep_r"][t], out["ep_l"][t] = episode["r"], episode["l"]
    return out


def trace(st, num_envs, T=None):
    """What every instance of stack `st` did on the judge's run, vectorised over time (rewards and zones need no
    sequential state): per position p of the stack

    * RewardByBallPosition: ``zones`` -- the set of zones it paid;
    * RewardInNormalState: ``replaced`` -- how many rewards it replaced, ``replaced_nonzero`` -- how many of those were
      non-zero before the wrapper directly below it."""
    run = raw_run(num_envs, simplified(st), T)
    o = run["obs"][:, 0].astype(np.float64)          # player_1's rows [T, n, 35]
    r = run["rew"].astype(np.float64)                # [T, 2, n]
    before = [r]                                      # rewards below position p
    low, high = OBS_LOW, OBS_HIGH
    out = {}
    for p, (name, kw) in enumerate(st):
        if name == "NormalizeObservation":
            o = (o - low) / (high - low)
            low, high = np.zeros(35), np.ones(35)
        elif name == "RewardByBallPosition":
            zone = (o[..., 27] > kw["y_line"]).astype(np.int64) + 2 * (o[..., 26] >= kw["x_line"])
            table = np.asarray(kw["additional_reward"], np.float64)
            r = np.stack([r[:, i] + table[i * 4 + zone] for i in range(2)], axis=1)
            out[p] = dict(zones=set(np.unique(zone).tolist()))
        elif name == "RewardInNormalState":
            hit = r == 0
            below = before[-2] if len(before) >= 2 else before[-1]
            out[p] = dict(replaced=int(hit.sum()), replaced_nonzero=int((hit & (below != 0)).sum()))
            r = np.where(hit, float(kw["reward"]), r)
        before.append(r)
    return out
