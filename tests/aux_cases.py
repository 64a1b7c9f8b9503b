"""The cases of the kernels that bracket every run -- init_kernel, reset_kernel, observe_kernel, random_actions_kernel
behind pz_init, pz_reset, pz_observe, pz_random_actions -- and the judge's side of each.

The judge is the unchanged CPU oracle: `OracleEnv(n, make_config(...))` for the constructor's state, `reset(mask)`,
`observe()`, the statistics views and `random_actions`.  Rows in the 2-byte and float formats are the oracle's rows as
`mixed_judge.rows_as` converts them.  tests/test_gpu_aux_kernels.py runs every case through the C ABI;
tests/test_aux_kernels_host.py shows on the oracle alone that the cases bite and that every axis value occurs.

A reset keeps the carry-over words of a game (CARRY_OVER) and continues its draws from the game's counter, so a reset
case starts from one of three states (STARTS): the constructor's, where every carry-over word holds its initial value;
`kernel_configs.plant_states` (random valid states, an eighth of the games over); and the state after PLAYED_FRAMES
frames of random actions under WINNING_SCORE without auto reset, taken from the oracle.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from kernel_configs import NORMALIZED, plant_states
from mixed_judge import rows_as  # noqa: F401  (the GPU tests take it from here: one judge, one conversion)

WORDS, OBS = 44, 35
LANES = 64                                  # games per workgroup of the four kernels (one wave)
# (n, stride): one game, a wave short of / exactly / one past its last lane, three waves and a tail at a pitch that is
# not the batch size; and an odd batch at its own pitch (the 2-byte rows then share their last dword with the pad row)
SIZES = ((1, 256), (63, 256), (64, 256), (65, 256), (200, 256), (129, 129))
STARTS = ("constructed", "planted", "played")
SERVES = ("winner", "alternate", "random")
MASKS = ("null", "zeros", "ones", "lane", "random")
POINTERS = ("both", "p1", "p2", "none")
FORMATS = tuple(range(7))                   # enum pz_obs_format
ID_BASES = (0, 2**32 - 3, 2**40 + 5)        # the second: the batch crosses 2^32 at its fourth game
SEEDS = (20261018, 0x9E3779B97F4A7C15)      # the second: a key whose high word is not 0
WINNING_SCORE = 2
PLAYED_FRAMES = 150
ACTION_SEED = 0x5EED0AC700000AC7            # both key words non-zero
# what raw_env.reset leaves alone (pikazoo_env.py:149-173): per player diving_direction, lying_down_duration_left,
# computer_where_to_stand_by, power_hit_key_is_down_previous; of the ball the two previous positions, fine_rotation,
# expected_landing_point_x, punch_effect_x.  (The draw counter is carried over too, but a reset advances it.)
CARRY_OVER = (7, 8, 11, 12, 20, 21, 24, 25, 31, 32, 33, 34, 35, 36, 37)


# ---- start states -----------------------------------------------------------------------------------------------------
def constructed_state(oracle, n, seed, env_id_base):
    return oracle.OracleEnv(n, oracle.make_config(winning_score=WINNING_SCORE, seed=seed, env_id_base=env_id_base)).state.copy()


def start_state(oracle, kind, n, seed, env_id_base):
    """int32[44, n] of STARTS[kind]"""
    if kind == "constructed":
        return constructed_state(oracle, n, seed, env_id_base)
    if kind == "planted":
        return plant_states(SimpleNamespace(seed=seed, winning_score=WINNING_SCORE, matrix=False, n=n))[0]
    assert kind == "played", kind
    env = oracle.OracleEnv(n, oracle.make_config(winning_score=WINNING_SCORE, seed=seed, env_id_base=env_id_base,
                                                 auto_reset=False))
    env.reset()
    for t in range(PLAYED_FRAMES):
        env.step(*oracle.random_actions(n, env_id_base, ACTION_SEED, t, 18))
    return env.state.copy()


def seeded_stats(n, seed):
    """(float64[2, n] returns, int32[n] lengths), every one non-zero: a cleared lane is visible"""
    rng = np.random.default_rng(seed ^ 0x57A75)
    returns = rng.integers(1, 40, (2, n)) * 0.25 * rng.choice([-1.0, 1.0], (2, n))
    lengths = rng.integers(1, 5000, n).astype(np.int32)
    return returns, lengths


# ---- pz_reset -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ResetCase:
    name: str
    n: int
    stride: int
    packed: bool
    obs_format: int
    serve: str
    mask: str            # MASKS
    pointers: str        # POINTERS: which observation pointers are passed
    stats: bool          # a statistics pointer, with episode_stats_mode on
    start: str           # STARTS
    seed: int = SEEDS[0]
    env_id_base: int = 1 << 20

    def mask_array(self):
        """uint8[n], or None for the NULL mask"""
        n = self.n
        if self.mask == "null":
            return None
        m = np.zeros(n, np.uint8)
        if self.mask == "ones":
            m[:] = 1
        elif self.mask == "lane":  # the last lane of the last full wave, alone
            assert n >= LANES
            m[n // LANES * LANES - 1] = 1
        elif self.mask == "random":
            m[:] = np.random.default_rng(self.seed ^ (n * 0x9E37)).random(n) < 0.4
            if n > 1:  # both kinds of lane occur
                m[0], m[n - 1] = 1, 0
        return m

    def masked(self):
        """bool[n]: the games the reset re-initialises"""
        m = self.mask_array()
        return np.ones(self.n, bool) if m is None else m.astype(bool)


def _reset(name, size, packed, fmt, serve, mask, pointers, stats, start, **kw):
    return ResetCase(name, size[0], size[1], packed, fmt, serve, mask, pointers, stats, start, **kw)


def reset_cases():
    """About twenty: every value of every axis at least once, and the two named pairs -- (packed, 2-byte rows, random
    mask, statistics) and (int32, float32 normalized, single-lane mask)."""
    s1, s63, s64, s65, s200, s129 = SIZES
    return [
        _reset("int32-i32-null-constructed", s200, False, 0, "winner", "null", "both", False, "constructed"),
        _reset("packed-i32-ones-stats", s64, True, 0, "alternate", "ones", "both", True, "planted"),
        _reset("int32-f32norm-lane", s65, False, 1, "random", "lane", "both", False, "planted"),
        _reset("packed-i16-random-stats-odd", s129, True, 2, "winner", "random", "both", True, "played"),
        _reset("int32-f16-random-stats-63", s63, False, 3, "alternate", "random", "both", True, "planted"),
        _reset("packed-bf16-lane-p1", s200, True, 4, "random", "lane", "p1", False, "played"),
        _reset("int32-f16norm-zeros-p2-stats", s65, False, 5, "winner", "zeros", "p2", True, "planted"),
        _reset("packed-bf16norm-random-stats-64", s64, True, 6, "alternate", "random", "both", True, "planted"),
        _reset("int32-i16-null-stats-one-game", s1, False, 2, "random", "null", "both", True, "constructed"),
        _reset("packed-f32norm-ones-one-game", s1, True, 1, "winner", "ones", "both", False, "planted"),
        _reset("packed-f32norm-random-stats", s200, True, 1, "random", "random", "both", True, "planted"),
        _reset("int32-bf16norm-random-p1-stats-odd", s129, False, 6, "random", "random", "p1", True, "played"),
        _reset("packed-f16-zeros-none-stats", s63, True, 3, "winner", "zeros", "none", True, "planted"),
        _reset("int32-i32-random-none-stats", s200, False, 0, "alternate", "random", "none", True, "played"),
        _reset("packed-f16norm-random-p2", s65, True, 5, "alternate", "random", "p2", False, "planted"),
        _reset("int32-bf16-ones-stats-odd", s129, False, 4, "winner", "ones", "both", True, "planted"),
        _reset("packed-i32-random-stats-ids-cross-2^32", s200, True, 0, "random", "random", "both", True, "played",
               env_id_base=ID_BASES[1]),
        _reset("int32-i16-lane-stats-64", s64, False, 2, "alternate", "lane", "both", True, "planted", seed=SEEDS[1]),
        _reset("packed-i16-null-63", s63, True, 2, "random", "null", "both", False, "played"),
        _reset("int32-f32norm-random-stats-large-ids", s200, False, 1, "alternate", "random", "both", True, "played",
               seed=SEEDS[1], env_id_base=ID_BASES[2]),
        _reset("packed-bf16norm-lane-p2-stats-odd", s129, True, 6, "winner", "lane", "p2", True, "planted"),
        _reset("int32-f16-random-p2-65", s65, False, 3, "winner", "random", "p2", False, "constructed"),
    ]


def reset_config(oracle, case):
    return oracle.make_config(winning_score=WINNING_SCORE, serve=case.serve, seed=case.seed, env_id_base=case.env_id_base,
                              normalize_obs=case.obs_format in NORMALIZED, episode_stats=1 if case.stats else 0)


def reset_judgement(oracle, case):
    """The judge's side of one reset case: the constructor's state, the start, the mask, the seeded statistics, and what
    `reset(mask)` of the oracle leaves -- state, both agents' rows of ALL games (the oracle's dtype), statistics."""
    env = oracle.OracleEnv(case.n, reset_config(oracle, case))
    constructor = env.state.copy()
    start = start_state(oracle, case.start, case.n, case.seed, case.env_id_base)
    env.state[:] = start
    returns0, lengths0 = seeded_stats(case.n, case.seed)
    if case.stats:
        env.episode_returns[:] = returns0
        env.episode_lengths[:] = lengths0
    mask = case.mask_array()
    obs = [o.copy() for o in env.reset(mask)]
    out = SimpleNamespace(constructor=constructor, start=start, mask=mask, masked=case.masked(), state=env.state.copy(),
                          obs=obs, returns0=returns0, lengths0=lengths0,
                          returns=env.episode_returns.copy() if case.stats else None,
                          lengths=env.episode_lengths.copy() if case.stats else None)
    for a in (out.constructor, out.start, out.state):
        a.setflags(write=False)
    return out


# ---- pz_observe ---------------------------------------------------------------------------------------------------------
OBSERVE_FIXTURES = ("planted_random_states_human", "planted_random_states_both_computer",
                    "planted_random_states_p2_computer_random_serve", "planted_fast_balls_human",
                    "planted_fast_balls_both_computer")  # those of test_observe_over_the_planted_state_space
OBSERVE_PAD = 37  # stride - n of the observe cases: a pitch that is neither the batch size nor a multiple of the wave

_observe_cache = {}


def observe_states():
    """int32[44, m], m odd: plant_states' set and every state of the five committed planted fixtures"""
    if "states" not in _observe_cache:
        from conftest import load_golden

        parts = [plant_states(SimpleNamespace(seed=SEEDS[0], winning_score=WINNING_SCORE, matrix=False, n=200))[0]]
        for name in OBSERVE_FIXTURES:
            d = load_golden(name)
            parts += [d["planted"].astype(np.int32)] + [s.astype(np.int32) for s in d["states"]]
        states = np.ascontiguousarray(np.concatenate(parts, axis=1))
        if states.shape[1] % 2 == 0:
            states = np.ascontiguousarray(states[:, :-1])
        states.setflags(write=False)
        _observe_cache["states"] = states
    return _observe_cache["states"]


def observe_judgement(oracle, normalized):
    """[rows of player 1, rows of player 2] of observe_states(), int32 or the float32 NormalizeObservation quotient;
    computed once per kind and shared: no test writes them"""
    key = ("rows", bool(normalized))
    if key not in _observe_cache:
        states = observe_states()
        env = oracle.OracleEnv(states.shape[1], oracle.make_config(normalize_obs=bool(normalized)))
        env.state[:] = states
        _observe_cache[key] = list(env.observe())
    return _observe_cache[key]


@dataclass(frozen=True)
class ObserveCase:
    name: str
    packed: bool
    obs_format: int
    pointers: str = "both"


def observe_cases():
    names = ("i32", "f32norm", "i16", "f16", "bf16", "f16norm", "bf16norm")
    cases = [ObserveCase(f"{'packed' if packed else 'int32'}-{names[f]}", packed, f)
             for packed in (False, True) for f in FORMATS]
    return cases + [ObserveCase("int32-bf16-p1-only", False, 4, "p1"), ObserveCase("packed-f32norm-p2-only", True, 1, "p2")]


# ---- pz_init ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class InitCase:
    name: str
    n: int
    stride: int
    packed: bool
    env_id_base: int
    seed: int


def init_cases():
    """both state formats x the three id bases x two seeds, the batch sizes taken in turn"""
    out = []
    for packed in (False, True):
        for b, base in enumerate(ID_BASES):
            for s, seed in enumerate(SEEDS):
                n, stride = SIZES[(len(out) + 4) % len(SIZES)]
                out.append(InitCase(f"{'packed' if packed else 'int32'}-base{b}-seed{s}-n{n}", n, stride, packed, base, seed))
    return out


# ---- pz_random_actions --------------------------------------------------------------------------------------------------
RA_SIZES = (1, 255, 256, 257)               # the kernel's workgroup holds 256 games
RA_ACTIONS = (13, 18)
RA_FRAMES = (0, 2**32 - 1, 2**32 + 7)


def random_action_cases():
    """(n, n_actions, t, env_id_base)"""
    return [(n, a, t, base) for n in RA_SIZES for a in RA_ACTIONS for t in RA_FRAMES for base in ID_BASES]


def low_word_ids_actions(oracle, n, env_id_base, t, n_actions):
    """What a kernel that dropped the high word of the global id would draw: game i under id (env_id_base + i) mod 2^32"""
    a1, a2 = np.empty(n, np.int32), np.empty(n, np.int32)
    done = 0
    while done < n:  # runs of consecutive low words
        lo = (env_id_base + done) % 2**32
        run = min(n - done, 2**32 - lo)
        a1[done:done + run], a2[done:done + run] = oracle.random_actions(run, lo, ACTION_SEED, t, n_actions)
        done += run
    return a1, a2


# ---- the chain of launches ----------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_STRIDE, CHAIN_FRAMES = 200, 256, 40
CHAIN_ID_BASE = 2**32 - 100                 # the batch crosses 2^32 in its second wave


def chain_mask(term, seed=SEEDS[0]):
    """the masked reset of the chain: the finished games plus a random tenth"""
    extra = np.random.default_rng(seed ^ 0xC4A1).random(term.shape[0]) < 0.1
    return ((term != 0) | extra).astype(np.uint8)
