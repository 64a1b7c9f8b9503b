"""The runtime configurations of the policy-rollout launch (include/pikazoo_rollout.h: ``pz_rollout_policy``, the six
``rollout_policy_kernel<H, ACT>`` of csrc/pz_rollout.hip) -- the counterpart of tests/kernel_configs.py and
tests/held_configs.py, whose factors, tables, planting recipe and seed it reuses unchanged.  Host only: nothing here needs a
device.

Structure (picks the instantiation and the LDS layout): hidden {32, 64, 128} x activation {tanh, relu}, and one parameter set
for both agents or one each (never two at hidden 128: the refusal is tests/test_gpu_policy_rollout.py's).  Runtime: RUNTIME
below -- the `pz_config` factors of kernel_configs.FACTORS, the two 4-byte row formats, both action element types, entropy
asked for or not, a state stride of n or n + 64, slabs at a pitch of n, n + 4 or n + 3 games, `step` by value or on the device,
the head ("random": net_judge.make_params; "masked": -inf in b3 at five actions; "bad": a NaN in one logit of agent 2's b3, so
every row of agent 2 is a step-6 row that must hand action 0 to the frame), the ids (IDS) and the shape (n, k).  What cannot be
combined (`compatible`): a bad head needs agent 2's own set; n = 67 takes a pitch of 67 or 70 (the dword flush); the large ids
need the batches in which every one of their three wraps has live games (or steps) on both sides -- the low env-id word at game
64, first_game + g at game 40, T0 + t at t = 2 -- which leaves out n = 36 and k = 1.

Every launch starts from kernel_configs.plant_states.  ``generated()`` is deterministic (kernel_configs.SEED) and such that
  * every instantiation receives every level of every factor that applies to it, in at least MIN_PER_KERNEL configurations;
  * every compatible pair of levels of two factors occurs in some configuration;
  * every instantiation has a configuration that ``raw_env.rollout_policy`` can repeat (``Config.binding``);
  * the cancelling table under RewardInNormalState outside -- the one order that sees the table's 0 -- has a launch of k = 8;
  * every configuration BITES on the CPU restatement alone (``misses()``), and its restated trajectory stays within the
    judge's cap on ambiguous rows in every slab.  A drawn configuration that misses is drawn again under the next seed.

``restate()`` is the whole launch on the CPU, from parts the project already trusts: the C oracle for the frame,
net_judge.restate_float32 for the head and policy_judge.restate_float32 for the draw at (first_game + g, T0 + t).  It also
plays the kernel for MUTANTS.  ``compare()`` is what tests/test_gpu_policy_rollout_configs.py holds a launch's outputs to;
tests/test_policy_rollout_configs_host.py shows that it passes the restatement and rejects every mutant.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import random

import numpy as np

import act_judge as AJ
import kernel_configs as kc
import net_judge as N
import policy_judge as J
from kernel_configs import FACTORS, MIN_PER_KERNEL, NORMAL_STATE_REWARD, SEED, SHAPING, plant_states, random_valid_states  # noqa: F401 (reused as they are)

HIDDEN, ACTIVATIONS = (32, 64, 128), N.ACTIVATIONS
SHAPES = ((36, 8), (68, 8), (132, 8), (132, 1), (67, 5))   # (n, k); (67, 5): the C ABI alone
CROSSING = ((68, 8), (132, 8), (67, 5))                    # the shapes in which each wrap of the large ids has both sides
IDS = {"small": dict(env_id_base=kc.IDS["small"][0], first_game=3, step=kc.IDS["small"][1]),
       # the low env-id word wraps at game 64, first_game + g at game 40, T0 + t at t = 2
       "large": dict(env_id_base=(5 << 32) + 0xFFFFFFC0, first_game=(1 << 32) - 40, step=(1 << 32) - 2)}
RUNTIME = {
    **{f: FACTORS[f] for f in ("winning_score", "serve", "auto_reset", "simplify_action", "shaping", "normal_state_mode", "episode_stats")},
    "obs_format": (kc.OBS_I32, kc.OBS_F32_NORM),
    "action_format": ("i32", "i64"),
    "entropy": (1, 0),
    "stride": FACTORS["stride"],
    "pitch": ("n", "n+4", "n+3"),
    "step": ("value", "device"),
    "head": ("random", "masked", "bad"),
    "ids": FACTORS["ids"],
    "shape": SHAPES,
    "weights": ("shared", "separate"),
}
MASKED_ACTIONS, BAD_LOGIT = 5, 3
REDRAWS = 16                     # seeds tried on one set of levels before other levels are drawn
MUTANTS = ("step_truncated_to_32_bits", "game_id_truncated_to_32_bits", "env_id_high_word_dropped", "ended_game_not_reset",
           "frozen_game_still_paid", "statistics_of_the_other_reward", "normal_state_on_the_wrong_side", "agent2_on_agent1_parameters",
           "step_consumed_for_the_bootstrap_row", "rewards_one_slab_early", "bad_row_action_not_reaching_the_frame")


def kernel_name(hidden, activation) -> str:
    return f"rollout_policy_kernel<{hidden}, {ACTIVATIONS.index(activation)}>"


KERNELS = tuple(kernel_name(h, a) for h in HIDDEN for a in ACTIVATIONS)


def structures():
    return [(h, a) for h in HIDDEN for a in ACTIVATIONS]


def domain(hidden) -> dict:
    """factor -> the levels an instantiation of width `hidden` takes"""
    dom = dict(RUNTIME)
    if hidden == 128:  # two staged sets do not fit the LDS
        dom["weights"], dom["head"] = ("shared",), ("random", "masked")
    return dom


def compatible(lv: dict) -> bool:
    return ((lv["head"] != "bad" or lv["weights"] == "separate") and (lv["shape"] != (67, 5) or lv["pitch"] != "n+4") and
            (lv["ids"] != "large" or lv["shape"] in CROSSING))


_BOUND = ("head", "weights", "shape", "pitch", "ids")  # the factors `compatible` reads


def compatible_pair(pair) -> bool:
    """some compatible configuration holds both levels of `pair`"""
    fixed = dict(pair)
    return any(compatible({**dict(zip(_BOUND, lv)), **fixed}) for lv in itertools.product(*(RUNTIME[f] for f in _BOUND)))


@dataclasses.dataclass(frozen=True)
class Config:
    """One launch: the instantiation, the runtime levels, and the seed of pz_config.seed / the planted states / the nets"""
    kernel: str
    hidden: int
    activation: str
    name: str
    seed: int
    winning_score: int
    serve: str
    auto_reset: int
    simplify_action: int
    shaping: str
    normal_state_mode: int
    episode_stats: object
    obs_format: int
    action_format: str
    entropy: int
    stride: str
    pitch: str
    step: str
    head: str
    ids: str
    shape: tuple
    weights: str

    matrix = False  # (plant_states: scores drawn below the winning score)

    @property
    def n(self) -> int:
        return self.shape[0]

    @property
    def k(self) -> int:
        return self.shape[1]

    @property
    def n_actions(self) -> int:
        return 13 if self.simplify_action else 18

    @property
    def stride_games(self) -> int:
        return self.n + (64 if self.stride == "n+64" else 0)

    @property
    def pitch_games(self) -> int:
        return self.n + {"n": 0, "n+4": 4, "n+3": 3}[self.pitch]

    @property
    def stats_ptr(self) -> bool:
        return self.episode_stats in (1, 2)

    @property
    def stats_mode(self) -> int:
        return 1 if self.episode_stats == "1-null" else int(self.episode_stats)

    @property
    def shaped(self) -> bool:
        return SHAPING[self.shaping] is not None

    @property
    def float_rewards(self) -> bool:
        return self.shaped or self.normal_state_mode != 0

    @property
    def env_id_base(self) -> int:
        return IDS[self.ids]["env_id_base"]

    @property
    def first_game(self) -> int:
        return IDS[self.ids]["first_game"]

    @property
    def t0(self) -> int:
        return IDS[self.ids]["step"]

    @property
    def policy_seed(self) -> int:
        return self.seed ^ 0x5EED

    @property
    def separate(self) -> bool:
        return self.weights == "separate"

    @property
    def binding(self) -> bool:
        """raw_env.rollout_policy can run this launch: n % 4 == 0 at the env's own pitch, and a `pz_config` a wrapper stack
        builds (a statistics mode has its pointer; mode 2 of either wrapper names a wrapper below it)"""
        return (self.n % 4 == 0 and self.pitch == "n" and self.episode_stats != "1-null" and
                not (self.episode_stats == 2 and not self.float_rewards) and not (self.normal_state_mode == 2 and not self.shaped))

    def oracle_kwargs(self, **over) -> dict:
        table, x_line, y_line = SHAPING[self.shaping] or (None, 216, 176)
        kw = dict(winning_score=self.winning_score, serve=self.serve, seed=self.seed, simplify_action=bool(self.simplify_action),
                  additional_reward=table, x_line=x_line, y_line=y_line, auto_reset=bool(self.auto_reset),
                  normal_state_reward=NORMAL_STATE_REWARD if self.normal_state_mode else None,
                  normal_state_outside=self.normal_state_mode == 2, normalize_obs=self.obs_format == kc.OBS_F32_NORM,
                  episode_stats=self.stats_mode, env_id_base=self.env_id_base)
        kw.update(over)
        return kw

    def levels(self) -> dict:
        return {f: getattr(self, f) for f in RUNTIME}

    def masked(self):
        """bool[A]: the actions a masked head never draws (the last one among them: the clamp's side)"""
        A = self.n_actions
        m = np.zeros(A, bool)
        if self.head == "masked":
            rng = np.random.default_rng([self.seed & 0xFFFFFFFF, A])
            m[rng.choice(A - 1, MASKED_ACTIONS - 1, replace=False)] = True
            m[A - 1] = True
        return m

    def params(self, unmasked=False):
        """[agent 1's (W1, b1, W2, b2, W3, b3), agent 2's]: the same list twice with shared weights"""
        A = self.n_actions
        base = int(self.seed % 100003)
        sets = [N.make_params(35, self.hidden, A + 1, base + s) for s in range(2 if self.separate else 1)]
        for ps in sets:
            if self.head == "masked":
                ps[5][:A][self.masked()] = 0.0 if unmasked else -np.inf
        if self.head == "bad":
            sets[1][5][BAD_LOGIT] = np.nan
        return [sets[0], sets[-1]]

    def start_state(self):
        """(planted int32[44, n], over bool[n])"""
        return plant_states(self, self.n)


def make(structure, levels: dict, name: str, seed: int) -> Config:
    hidden, activation = structure
    return Config(kernel=kernel_name(hidden, activation), hidden=hidden, activation=activation, name=name, seed=seed, **levels)


# ---- the launch on the CPU --------------------------------------------------------------------------------------------------
def _oracle():
    try:
        from oracle import pz_oracle
    except ImportError:  # outside pytest: tests/conftest.py puts the repository root on sys.path
        import sys
        from pathlib import Path

        sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
        from oracle import pz_oracle
    pz_oracle.build()
    return pz_oracle


def uniforms(seed, games, T):
    """u[2, n] float64: policy_judge.uniforms for explicit game ids `games` (uint64 [n]) at step T"""
    T = int(T) & J.MASK
    G = np.asarray(games, np.uint64)
    ctr = (G & np.uint64(0xFFFFFFFF), G >> np.uint64(32), np.full(G.size, T & 0xFFFFFFFF, np.uint64),
           np.full(G.size, (2 + 4 * (T >> 32)) & 0xFFFFFFFF, np.uint64))
    w = J.philox4x32_10_numpy(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return np.stack([(x >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for x in w[:2]])


def shaped_zero(c: Config, state):
    """what shape_rewards makes of an env reward of 0 on `state`'s ball: float32 [2, n] (the pay of a game that is not frozen)"""
    n = state.shape[1]
    table = SHAPING[c.shaping]
    r = np.zeros((2, n), np.float32)
    nsr = np.float32(NORMAL_STATE_REWARD)
    if c.normal_state_mode == 1:
        r[:] = nsr
    if table is not None:
        values, x_line, y_line = table
        zone = (state[27] > y_line).astype(np.int64) + 2 * (state[26] >= x_line)
        r = np.stack([r[p] + np.asarray(values, np.float32)[p * 4 + zone] for p in range(2)])
    if c.normal_state_mode == 2:
        r = np.where(r == 0, nsr, r)
    return r.astype(np.float32)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x.astype(np.int32)


def restate(c: Config, mutant=None) -> dict:
    """Every output of the header's definition for `c` from its planted states, as numpy arrays: obs int32 bits [2][k + 1, n,
    35], actions int64 [2][k, n], log_probs / entropy float32 [2][k, n] (entropy: None when not asked for), values float32
    [2][k + 1, n], rewards int32 bits [2][k, n], terminated uint8 [k, n], state int32 [44, n], returns float64 [2, n] and
    lengths int32 [n] (None without a statistics pointer), episodes_done (what *episodes_done must receive), and head: float32
    [k + 1][2][n, O], the head of each slab's rows under the launch's parameters.  `mutant`: one of MUTANTS, played in place of
    the kernel (the head stays the honest one: on the device it comes from pz_mlp_forward).  Under "_watch" it also carries
    what the trajectory did, for measure()."""
    assert mutant is None or mutant in MUTANTS, mutant
    po = _oracle()
    n, k, A = c.n, c.k, c.n_actions
    over_kw = {}
    if mutant == "env_id_high_word_dropped":
        over_kw["env_id_base"] = c.env_id_base & 0xFFFFFFFF
    if mutant == "ended_game_not_reset":
        over_kw["auto_reset"] = False
    if mutant == "statistics_of_the_other_reward":
        over_kw["episode_stats"] = {0: 0, 1: 2, 2: 1}[c.stats_mode]
    if mutant == "normal_state_on_the_wrong_side" and c.normal_state_mode:
        over_kw["normal_state_outside"] = c.normal_state_mode == 1
    env = po.OracleEnv(n, po.make_config(**c.oracle_kwargs(**over_kw)))
    planted, over = c.start_state()
    env.state[:] = planted
    params = c.params()
    open_params = c.params(unmasked=True) if c.head == "masked" else None
    masked = c.masked()
    games = np.arange(n, dtype=np.uint64) + np.uint64(c.first_game)
    if mutant == "game_id_truncated_to_32_bits":
        games = games & np.uint64(0xFFFFFFFF)
    out = dict(obs=[[], []], actions=[[], []], log_probs=[[], []], entropy=[[], []], values=[[], []], rewards=[[], []], terminated=[], head=[])
    watch = dict(frozen=[], ended=[], on_line=0, cancelled=0, masked_hits=0, ambiguous=[], off_policy=0)
    table, x_line, y_line = SHAPING[c.shaping] or (None, None, None)
    nsr = np.float32(NORMAL_STATE_REWARD)
    done = 0

    def heads(rows):
        honest = [N.restate_float32(rows[s], params[s], c.activation) for s in range(2)]
        played = [honest[0], N.restate_float32(rows[1], params[0], c.activation)] if mutant == "agent2_on_agent1_parameters" else honest
        return honest, played

    def draw(rows, T):
        honest, played = heads(rows)
        u = uniforms(c.policy_seed, games, T & 0xFFFFFFFF if mutant == "step_truncated_to_32_bits" else T)
        picked = [J.restate_float32(played[s][:, :A], u[s]) for s in range(2)]
        if mutant is None:
            true_u = uniforms(c.policy_seed, np.arange(n, dtype=np.uint64) + np.uint64(c.first_game), T)
            watch["ambiguous"].append([int(J.sample(honest[s][:, :A].astype(np.float64), true_u[s])[1].sum()) for s in range(2)])
            if open_params is not None:
                for s in range(2):
                    free = N.restate_float32(rows[s], open_params[s], c.activation)
                    watch["masked_hits"] += int(masked[J.sample(free[:, :A].astype(np.float64), true_u[s])[0]].sum())
        return honest, played, picked

    rows = env.observe()
    for t in range(k):
        honest, played, picked = draw(rows, c.t0 + t)
        out["head"].append(honest)
        for s in range(2):
            out["obs"][s].append(_bits(rows[s]).copy())
            out["actions"][s].append(picked[s][0].astype(np.int64))
            out["log_probs"][s].append(picked[s][1].astype(np.float32))
            out["entropy"][s].append(picked[s][2].astype(np.float32))
            out["values"][s].append(played[s][:, A].copy())
        a1, a2 = picked[0][0].astype(np.int32), picked[1][0].astype(np.int32)
        if mutant == "bad_row_action_not_reaching_the_frame":
            a2 = np.where(np.isnan(picked[1][1]), 1, a2).astype(np.int32)
        frozen = (env.state[po.E_GAME_ENDED] != 0) & (not env.cfg.auto_reset)
        obs, rew, term = env.step(a1, a2)
        ended = (term != 0) & ~frozen
        done += int(ended.sum())
        pay = [_bits(rew[p]).copy() for p in range(2)]
        if mutant == "frozen_game_still_paid" and c.float_rewards:
            zero = shaped_zero(c, env.state)
            pay = [np.where(frozen, zero[p].view(np.int32), pay[p]) for p in range(2)]
        for p in range(2):
            out["rewards"][p].append(pay[p])
        out["terminated"].append(term.copy())
        watch["frozen"].append(frozen)
        watch["ended"].append(ended)
        if table is not None:
            bx, by = env.state[po.B_X], env.state[po.B_Y]
            watch["on_line"] += int((~frozen & ((bx == x_line) | (by == y_line))).sum())
            if c.shaping == "cancel" and c.normal_state_mode == 2:
                watch["cancelled"] += int((~frozen & (by == 252) & (rew[0] == nsr) & (rew[1] == nsr)).sum())
        rows = [obs[0].copy(), obs[1].copy()]
    honest, played = heads(rows)
    out["head"].append(honest)
    for s in range(2):
        out["obs"][s].append(_bits(rows[s]).copy())
        out["values"][s].append(played[s][:, A].copy())
    if mutant == "step_consumed_for_the_bootstrap_row":
        _, _, picked = draw(rows, c.t0 + k)
        frozen = (env.state[po.E_GAME_ENDED] != 0) & (not env.cfg.auto_reset)
        _, _, term = env.step(picked[0][0].astype(np.int32), picked[1][0].astype(np.int32))
        done += int(((term != 0) & ~frozen).sum())
    if mutant == "rewards_one_slab_early":
        for p in range(2):
            out["rewards"][p] = out["rewards"][p][1:] + [np.zeros(n, np.int32)]
    res = {key: [np.stack(v[0]), np.stack(v[1])] for key, v in out.items() if key not in ("terminated", "head")}
    if not c.entropy:
        res["entropy"] = None
    res["terminated"] = np.stack(out["terminated"]).astype(np.uint8)
    res["head"] = out["head"]
    res["state"] = env.state.copy()
    res["returns"] = env.episode_returns.copy() if c.stats_ptr else None
    res["lengths"] = env.episode_lengths.copy() if c.stats_ptr else None
    res["episodes_done"] = done
    watch["over"] = over
    res["_watch"] = watch
    return res


# ---- what a launch's outputs are held to ------------------------------------------------------------------------------------
def wrapper_stack(c: Config):
    """check_config's stack for `c` (the fused wrappers as the reference would stack them, innermost first)"""
    from test_gpu_kernel_matrix import _wrapper_stack

    return _wrapper_stack(c)


def compare(c: Config, got: dict):
    """The outputs `got` of one launch of `c` (restate()'s keys) against the references.  Returns (failures: empty for a pass,
    the ambiguous rows per slab and agent [k][2]).
      * the C oracle, stepped from the planted states with the actions `got` reports: every observation slab 0 .. k, rewards,
        flags, the final state and the statistics (returns as uint64 bits) bit for bit, episodes_done against its count of games
        that ended;
      * with auto_reset, the float outputs of a fused configuration in float64 against WrappedOracle under check_config's rule
        and tolerances: normalised rows exact, rewards within 1e-6, returns within 2e-6;
      * per slab and agent act_judge.verdict on the slab's rows with `got`'s head, which it first holds to float64; the
        bootstrap value bit-equal to column A of the head of slab k, that head within its tolerance; a masked head never draws
        a masked action and has finite log-probs; a bad head's rows are step-6 rows whose value is still column A."""
    from oracle.wrappers_oracle import WrappedOracle

    po = _oracle()
    n, k, A = c.n, c.k, c.n_actions
    fails = []
    acts = [np.asarray(got["actions"][s]) for s in range(2)]
    for s in range(2):
        if acts[s].shape != (k, n) or not ((acts[s] >= 0) & (acts[s] < A)).all():
            return [f"agent {s + 1}: actions outside [0, {A}) or of the wrong shape"], []
    planted, over = c.start_state()
    ref = po.OracleEnv(n, po.make_config(**c.oracle_kwargs()))
    ref.state[:] = planted
    judge64 = bool(c.auto_reset) and (c.float_rewards or c.obs_format == kc.OBS_F32_NORM or c.stats_ptr)
    wo = None
    if judge64:
        wo = WrappedOracle(n, wrapper_stack(c), winning_score=c.winning_score, serve=c.serve, seed=c.seed, env_id_base=c.env_id_base)
        wo.plant(planted)
    rows = ref.observe()
    done = 0
    for s in range(2):
        if not np.array_equal(got["obs"][s][0], _bits(rows[s])):
            fails.append(f"slab 0: observations of agent {s + 1}")
    for t in range(k):
        frozen = (ref.state[po.E_GAME_ENDED] != 0) & (not c.auto_reset)
        obs, rew, term = ref.step(acts[0][t].astype(np.int32), acts[1][t].astype(np.int32))
        done += int(((term != 0) & ~frozen).sum())
        wout = wo.step(acts[0][t], acts[1][t]) if wo else None
        for p in range(2):
            if not np.array_equal(got["obs"][p][t + 1], _bits(obs[p])):
                fails.append(f"slab {t + 1}: observations of agent {p + 1}")
            if not np.array_equal(got["rewards"][p][t], _bits(rew[p])):
                fails.append(f"slab {t}: rewards of agent {p + 1}")
        if not np.array_equal(got["terminated"][t], term):
            fails.append(f"slab {t}: terminated")
        if wo:
            w_obs, w_rew, w_term, _ = wout
            if not np.array_equal(got["terminated"][t], w_term):
                fails.append(f"slab {t}: terminated (float64 judge)")
            for p in range(2):
                if c.obs_format == kc.OBS_F32_NORM and not np.array_equal(got["obs"][p][t + 1], _bits(w_obs[p].astype(np.float32))):
                    fails.append(f"slab {t + 1}: normalised rows of agent {p + 1} vs float64")
                if c.float_rewards:
                    err = np.abs(np.ascontiguousarray(got["rewards"][p][t]).view(np.float32).astype(np.float64) - w_rew[p]).max()
                    if not err <= 1e-6:
                        fails.append(f"slab {t}: rewards of agent {p + 1} vs float64: {err}")
    if not np.array_equal(got["state"], ref.state):
        f, lane = np.argwhere(np.asarray(got["state"]) != ref.state)[0]
        fails.append(f"the final state: lane {lane} word {po.FIELD_NAMES[f]}: {got['state'][f, lane]} != oracle {ref.state[f, lane]}")
    if c.stats_ptr:
        if not np.array_equal(np.ascontiguousarray(got["returns"]).view(np.uint64), ref.episode_returns.view(np.uint64)):
            fails.append("episode returns")
        if not np.array_equal(got["lengths"], ref.episode_lengths):
            fails.append("episode lengths")
        if wo:
            err = np.abs(np.asarray(got["returns"]) - wo.episode_returns).max()
            if not err <= 2e-6:
                fails.append(f"episode returns vs float64: {err}")
            if not np.array_equal(got["lengths"], wo.episode_lengths):
                fails.append("episode lengths (float64 judge)")
    if int(got["episodes_done"]) != done:
        fails.append(f"episodes_done {int(got['episodes_done'])}, the oracle counts {done} games that ended")

    # the policy side
    params = c.params()
    masked = c.masked()
    ambiguous = []
    f32 = lambda x: np.ascontiguousarray(x).view(np.float32) if np.asarray(x).dtype != np.float32 else np.asarray(x)  # noqa: E731
    for t in range(k):
        us = J.uniforms(c.policy_seed, c.first_game, c.t0 + t, None, n)
        row = []
        for s in range(2):
            head = np.asarray(got["head"][t][s], np.float32)
            st = J.stats(head[:, :A])
            ent = got["entropy"][s][t] if got["entropy"] is not None else np.where(st["bad"], np.nan, st["H"]).astype(np.float32)
            slab = dict(head=head, actions=acts[s][t], log_probs=got["log_probs"][s][t], entropy=ent, values=got["values"][s][t])
            amb, bad = AJ.verdict(slab, f32(got["obs"][s][t]) if c.obs_format == kc.OBS_F32_NORM else got["obs"][s][t], params[s], c.activation,
                                  A, us[s], what=f"slab {t} agent {s + 1}")
            fails += bad
            row.append(amb)
            if c.head == "masked" and (masked[acts[s][t]].any() or not np.isfinite(got["log_probs"][s][t]).all()):
                fails.append(f"slab {t} agent {s + 1}: a masked action drawn, or a log-prob that is not finite")
            if c.head == "bad" and s == 1 and not (st["bad"].all() and (acts[s][t] == 0).all() and np.isnan(got["log_probs"][s][t]).all()):
                fails.append(f"slab {t} agent 2: a bad head's row is not a step-6 row")
        ambiguous.append(row)
    for s in range(2):  # the bootstrap row
        head = np.asarray(got["head"][k][s], np.float32)
        rows_k = f32(got["obs"][s][k]) if c.obs_format == kc.OBS_F32_NORM else got["obs"][s][k]
        want, tol = N.judge(rows_k, params[s], c.activation)
        if not np.array_equal(np.ascontiguousarray(got["values"][s][k]).view(np.uint32), np.ascontiguousarray(head[:, A]).view(np.uint32)):
            fails.append(f"agent {s + 1}: the bootstrap value is not column {A} of the head, bit for bit")
        if N.worst_share(head, want, tol)[0] > 1:
            fails.append(f"agent {s + 1}: the head of slab {k} beyond its tolerance")
    return fails, ambiguous


# ---- what a configuration does on the restatement alone ---------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Facts:
    ended_early: int       # games that end before slab k - 1
    revived: int           # ... that are reset (over at entry, or ended inside) and run in the next slab
    frozen_unpaid: int     # ... that enter a frame frozen and leave it with the flag up and reward 0
    over_at_entry: int
    on_line: int           # post-step balls of running games exactly on a shaping line
    cancelled: int         # points the cancelling table took to 0 and RewardInNormalState replaced
    masked_hits: int       # rows whose uniform falls into a masked action's interval with the mask at 0
    bad_rows: int          # step-6 rows
    wrap_side: int         # games that run (not frozen in frame 0) on the thinnest side of the wraps at game 40 and game 64
    worst_ambiguity: int   # ambiguous rows in one slab of one agent, at most


@functools.lru_cache(maxsize=None)
def measure(c: Config) -> Facts:
    r = restate(c)
    w = r["_watch"]
    k, n = c.k, c.n
    term, ended, frozen = r["terminated"] != 0, np.stack(w["ended"]), np.stack(w["frozen"])
    early = ended[:max(k - 1, 0)].any(0) if k > 1 else np.zeros(n, bool)
    revived = w["over"] & bool(c.auto_reset) & ~term[0]
    for t in range(k - 1):
        revived |= ended[t] & ~term[t + 1] & (r["obs"][0][t + 2] != r["obs"][0][t + 1]).any(1)
    unpaid = np.zeros(n, bool)
    for t in range(k):
        unpaid |= frozen[t] & term[t] & (r["rewards"][0][t] == 0) & (r["rewards"][1][t] == 0)
    running = ~frozen[0]
    side = min(int(part.sum()) for part in (running[:40], running[40:], running[:64], running[64:]))
    return Facts(int(early.sum()), int(revived.sum()), int(unpaid.sum()), int(w["over"].sum()), w["on_line"], w["cancelled"], w["masked_hits"],
                 int(np.isnan(r["log_probs"][1]).sum()), side, max(max(row) for row in w["ambiguous"]))


def misses(c: Config, f: Facts) -> list:
    """The conditions that `f` does not meet (empty: the configuration bites)"""
    out = []
    if c.k > 1 and f.ended_early == 0:
        out.append("no game ends before the last slab")
    if c.auto_reset and f.revived == 0:
        out.append("no game is reset and moves afterwards")
    if not c.auto_reset and f.frozen_unpaid == 0:
        out.append("no game stays frozen with reward 0")
    if f.over_at_entry == 0:
        out.append("no game is over at entry")
    if c.shaped and f.on_line == 0:
        out.append("no post-step ball of a running game on a shaping line")
    if c.shaping == "cancel" and c.normal_state_mode == 2 and f.cancelled == 0:
        out.append("no point cancelled by the table and replaced by RewardInNormalState")
    if c.ids == "large":
        base, first = c.env_id_base, c.first_game
        if not (base >> 32 < (base + c.n - 1) >> 32 and first >> 32 < (first + c.n - 1) >> 32 and c.t0 >> 32 < (c.t0 + c.k - 1) >> 32):
            out.append("a wrap of the large ids without live games or steps on both sides")
        elif f.wrap_side == 0:
            out.append("a wrap of the large ids without a running game on one side")
    if c.head == "masked" and f.masked_hits == 0:
        out.append("no uniform falls into a masked action's interval")
    if c.head == "bad" and f.bad_rows != c.n * c.k:
        out.append("agent 2's rows are not all step-6 rows")
    if f.worst_ambiguity > AJ.CAP(c.n):
        out.append("a slab with more ambiguous rows than the judge's cap")
    return out


# ---- the generator ----------------------------------------------------------------------------------------------------------
def required_pairs() -> set:
    return {p for p in kc.required_pairs([domain(h) for h in HIDDEN]) if compatible_pair(p)}


def _generate(seed: int):
    rng = random.Random(seed)
    structs = structures()
    doms = {kernel_name(*s): domain(s[0]) for s in structs}
    covered = set()
    out = []

    def draw(dom, fixed, prefer):
        made = 0
        for _ in range(4000):
            cand = {f: (rng.choice(prefer[f]) if prefer.get(f) and rng.random() < 0.85 else rng.choice(dom[f])) for f in dom}
            cand.update(fixed)
            if compatible(cand):
                yield cand
                made += 1
                if made == 400:
                    return

    def emit(s, levels):
        """`levels` on `s` under the first of REDRAWS seeds that bites; None if none does"""
        kernel = kernel_name(*s)
        name = f"{kernel} #{sum(1 for c in out if c.kernel == kernel)}"
        for attempt in range(REDRAWS):
            c = make(s, levels, name, kc._seed(f"{name}/{seed}/{attempt}"))
            if not misses(c, measure(c)):
                out.append(c)
                covered.update(kc._pairs(c.levels()))
                return c
        return None

    for s in structs:
        dom = doms[kernel_name(*s)]
        need = {f: set(v) for f, v in dom.items()}
        made, bound = 0, False
        for _ in range(200):
            if not (any(need.values()) or made < MIN_PER_KERNEL or not bound):
                break
            # an instantiation whose own configurations the binding cannot repeat: one that it can
            fixed = {} if bound or any(need.values()) else dict(pitch="n", shape=rng.choice([sh for sh in SHAPES if sh[0] % 4 == 0 and sh[1] > 1]),
                                                                episode_stats=rng.choice((0, 1)), normal_state_mode=rng.choice((0, 1)))
            best, best_score = None, -1
            for cand in itertools.islice(draw(dom, fixed, {f: sorted(v, key=str) for f, v in need.items()}), 24):
                score = 1000 * sum(cand[f] in need[f] for f in need) + len(kc._pairs(cand) - covered)
                if score > best_score:
                    best, best_score = cand, score
            c = emit(s, best)
            if c is None:
                continue  # these levels miss under every seed tried: the next draw differs (the stream moved on)
            for f in need:
                need[f].discard(best[f])
            made += 1
            bound = bound or c.binding
        else:
            raise AssertionError(f"{kernel_name(*s)}: no covering set of biting configurations")

    # the pairs no kernel's own configurations brought: more configurations, each with as many of them as a draw finds
    for _ in range(400):
        missing = sorted(required_pairs() - covered, key=str)
        if not missing:
            break
        (f, a), (g, b) = missing[0]
        takers = [s for s in structs if a in doms[kernel_name(*s)][f] and b in doms[kernel_name(*s)][g]]
        assert takers, f"no instantiation takes {missing[0]}"
        s = min(takers, key=lambda s: sum(1 for c in out if c.kernel == kernel_name(*s)))
        best, best_score = None, -1
        for cand in itertools.islice(draw(doms[kernel_name(*s)], {f: a, g: b}, {}), 48):
            score = len(kc._pairs(cand) & set(missing))
            if score > best_score:
                best, best_score = cand, score
        assert best is not None, f"no compatible configuration with {missing[0]}"
        emit(s, best)
    else:
        raise AssertionError(f"no biting configuration with {missing[0]}")

    # the cancelling table under RewardInNormalState outside is the one stack in which the table's 0 is seen: one such launch
    # of k = 8 on top of whatever the pairs brought
    sharp = lambda c: c.shaping == "cancel" and c.normal_state_mode == 2 and c.k == 8  # noqa: E731
    for _ in range(40):
        if any(sharp(c) for c in out):
            break
        s = min(structs, key=lambda s: sum(1 for c in out if c.kernel == kernel_name(*s)))
        fixed = dict(shaping="cancel", normal_state_mode=2, shape=rng.choice([sh for sh in SHAPES if sh[1] == 8]))
        emit(s, next(draw(doms[kernel_name(*s)], fixed, {})))
    else:
        raise AssertionError("no biting configuration of the cancelling table under RewardInNormalState outside at k = 8")
    return tuple(out), doms


@functools.lru_cache(maxsize=None)
def generated(seed: int = SEED):
    """(configurations, {kernel: domain}) of `seed`"""
    return _generate(seed)


def configs(seed: int = SEED):
    return generated(seed)[0]


# the configuration of the test of observation bases at 4 mod 16: n = 68, pitch = 68, k = 2
def misaligned_case() -> Config:
    levels = dict(winning_score=3, serve="winner", auto_reset=1, simplify_action=0, shaping="off", normal_state_mode=0, episode_stats=0,
                  obs_format=kc.OBS_I32, action_format="i64", entropy=1, stride="n", pitch="n", step="value", head="random", ids="small",
                  shape=(68, 2), weights="shared")
    return make((64, "tanh"), levels, "bases at 4 mod 16", kc._seed("bases at 4 mod 16"))
