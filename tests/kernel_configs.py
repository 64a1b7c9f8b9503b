"""The runtime configurations of every step-kernel instantiation.

tests/kernel_matrix.py names each instantiation and launches it under ONE configuration: the template arguments pick
the kernel, everything else in `pz_config` is read at run time inside it (`shape_rewards`, `stats_update`, the frozen
path, the action loads, the Philox ids, the observation staging).  This module holds those runtime factors, their
levels, and which levels each instantiation can take, and generates a deterministic set of configurations so that

  * every instantiation receives every level of every factor that applies to it, in at least MIN_PER_KERNEL configs;
  * on each side of the size switch, every pair of levels of two factors occurs in some configuration;
  * every configuration dispatches the instantiation it is assigned to -- through `dispatch()`, which works the
    PLAIN-or-fused choice of a k-frame launch out of the configuration with `is_plain()` below (the restatement of
    `is_plain()` in pika-zoo_amd/csrc/pz_dispatch.hpp), so a configuration the host would send to the other form of a
    kernel (`episode_stats_mode != 0` with a NULL statistics pointer, say) is tested as such.

tests/test_cabi_and_host.py checks those three rules; tests/test_gpu_kernel_configs.py runs every configuration
through the C ABI against the oracle.  `PZ_CONFIG_SEED` draws another set of configurations (every set meets the rules).
`plant_states()` is the start of every such launch; tests/held_configs.py reuses the factors, the tables, the ids and that
recipe for the two frame-skip kernel families.
"""
from __future__ import annotations

import functools
import itertools
import os
import random
import zlib
from dataclasses import dataclass

import numpy as np

# enum pz_obs_format (include/pikazoo_hip.h)
OBS_I32, OBS_F32_NORM, OBS_I16, OBS_F16, OBS_BF16, OBS_F16_NORM, OBS_BF16_NORM = range(7)
NORMALIZED = (OBS_F32_NORM, OBS_F16_NORM, OBS_BF16_NORM)
ACTION_FORMATS = {"i32": 0, "i64": 1, "u8": 2, "i16": 3}  # enum pz_action_format


def config_fields(**over) -> dict:
    """The `pz_config` words the kernel choice reads (0 unless given); `dispatch()` takes them as a mapping."""
    f = dict(p1_computer=0, p2_computer=0, packed_state=0, normalize_obs=OBS_I32, simplify_action=0, ballpos_reward=0,
             normal_state_mode=0, episode_stats_mode=0)
    unknown = set(over) - set(f)
    assert not unknown, unknown
    f.update({k: int(v) for k, v in over.items()})
    return f


def is_plain(cfg, stats: bool) -> bool:
    """pz_dispatch.hpp `is_plain()`: no fused wrapper, no statistics, raw integer rows -- what the PLAIN k-frame
    kernels are compiled for.  `stats`: a statistics pointer is passed (a statistics mode without one is PLAIN)."""
    return (cfg["simplify_action"] == 0 and cfg["ballpos_reward"] == 0 and cfg["normal_state_mode"] == 0 and
            cfg["normalize_obs"] in (OBS_I32, OBS_I16) and (cfg["episode_stats_mode"] == 0 or not stats))


# ---- the runtime factors and their levels ---------------------------------------------------------------------------
FACTORS = {
    "winning_score": (1, 3, 15),
    "serve": ("winner", "alternate", "random"),
    "auto_reset": (1, 0),
    "simplify_action": (0, 1),
    # RewardByBallPosition: off, or (table, x_line, y_line) of SHAPING
    "shaping": ("off", "default", "shifted", "degenerate", "cancel"),
    "normal_state_mode": (0, 1, 2),
    "obs_format": tuple(range(7)),
    # RecordEpisodeStatistics: 0 off, 1 the env's reward, 2 the wrapped reward, "1-null" mode 1 without a pointer
    "episode_stats": (0, 1, 2, "1-null"),
    "action_format": tuple(ACTION_FORMATS),  # pz_step only: pz_step_many takes int32 tapes alone
    # (env_id_base, t0) of IDS: lanes from 2^20, or above 2^32 with the low id word wrapping inside the launch and t0
    # crossing 2^32 inside the k-frame launches
    "ids": ("small", "large"),
    "stride": ("n", "n+64"),
}
TABLE = (0.0, -0.01, 0.25, 0.01, -0.5, 0.01, 0.0, -0.01)  # the matrix's fused rows
SHAPING = {
    "off": None,
    "default": (TABLE, 216, 176),
    "shifted": ((0.5, -0.25, 0.0, 1.0, -1.0, 0.0, 0.25, -0.5), 300, 240),
    # x >= 0 and y > 252 hold for every ball and none: all balls in zone 2; y == 252 is every ground touch
    "degenerate": ((0.125, -0.125, 0.75, 0.5, -0.75, 0.5, -0.375, 0.25), 0, 252),
    # a ball on the ground right of the net is player 1's point (+1 / -1) and sits in zone 3, left of it player 2's in
    # zone 1: the table cancels the scoring reward to exactly 0, and the high zones add 0
    "cancel": ((0.0, 1.0, 0.0, -1.0, 0.0, -1.0, 0.0, 1.0), 216, 176),
}
NORMAL_STATE_REWARD = -0.25
IDS = {"small": (1 << 20, 1000), "large": ((5 << 32) + 0xFFFFFC00, (1 << 32) - 2)}
MIN_PER_KERNEL = 4


@dataclass(frozen=True)
class Config:
    """One launch: the structure that picks the kernel (from its tests/kernel_matrix.py row) and the runtime levels."""
    entry: str
    k: int
    above: bool
    packed: bool
    p1: bool
    p2: bool
    tables: str
    kernel: str             # the instantiation it must dispatch
    name: str               # test id
    seed: int               # pz_config.seed and the planted states' generator
    winning_score: int
    serve: str
    auto_reset: int
    simplify_action: int
    shaping: str
    normal_state_mode: int
    obs_format: int
    episode_stats: object
    action_format: str
    ids: str
    stride_pad: int
    matrix: bool = False    # a matrix row (its planted states: the generator's scores, no re-draw)

    @property
    def n(self) -> int:
        from kernel_matrix import N_ABOVE, N_BELOW

        return N_ABOVE if self.above else N_BELOW

    @property
    def stride(self) -> int:
        return self.n + self.stride_pad

    @property
    def plain_form(self) -> bool:
        return is_plain(self.fields(), self.stats_ptr)

    @property
    def stats_ptr(self) -> bool:
        return self.episode_stats in (1, 2)

    @property
    def stats_mode(self) -> int:
        return 1 if self.episode_stats == "1-null" else int(self.episode_stats)

    @property
    def env_id_base(self) -> int:
        return IDS[self.ids][0]

    @property
    def t0(self) -> int:
        return IDS[self.ids][1]

    @property
    def shaped(self) -> bool:
        return SHAPING[self.shaping] is not None

    def fields(self) -> dict:
        return config_fields(p1_computer=self.p1, p2_computer=self.p2, packed_state=self.packed,
                             normalize_obs=self.obs_format, simplify_action=self.simplify_action,
                             ballpos_reward=self.shaped, normal_state_mode=self.normal_state_mode,
                             episode_stats_mode=self.stats_mode)

    def oracle_kwargs(self) -> dict:
        """oracle.make_config's kwargs but env_id_base (the oracle's rows: int32, or float32 if normalized)"""
        table, x_line, y_line = SHAPING[self.shaping] or (None, 216, 176)
        return dict(winning_score=self.winning_score, serve=self.serve, is_player1_computer=self.p1,
                    is_player2_computer=self.p2, seed=self.seed, simplify_action=bool(self.simplify_action),
                    additional_reward=table, x_line=x_line, y_line=y_line, auto_reset=bool(self.auto_reset),
                    normal_state_reward=NORMAL_STATE_REWARD if self.normal_state_mode else None,
                    normal_state_outside=self.normal_state_mode == 2, normalize_obs=self.obs_format in NORMALIZED,
                    episode_stats=self.stats_mode)

    def levels(self) -> dict:
        """factor -> level, for the factors that apply to this configuration"""
        lv = dict(winning_score=self.winning_score, serve=self.serve, auto_reset=self.auto_reset,
                  simplify_action=self.simplify_action, shaping=self.shaping,
                  normal_state_mode=self.normal_state_mode, obs_format=self.obs_format,
                  episode_stats=self.episode_stats, ids=self.ids, stride="n" if self.stride_pad == 0 else "n+64")
        if self.entry == "pz_step":
            lv["action_format"] = self.action_format
        return lv


def random_valid_states(n, rng):
    """int32[44, n]: every attribute at random over its valid range (players' (y, y_velocity) from the pairs a jump or
    a dive passes through), half of the balls next to a player -- the whole state space, reachable or not."""
    st = np.zeros((44, n), np.int32)
    for base, lo, hi in ((0, 32, 184), (13, 248, 400)):
        st[base + 0] = rng.integers(lo, hi + 1, n)
        st[base + 3] = rng.integers(0, 5, n)
        steps = rng.integers(0, 33, n)
        v0 = np.where(rng.random(n) < 0.7, -16, -5)
        y, v = np.full(n, 244), v0.copy()
        for k in range(33):
            move = (k < steps) & (y + v <= 244)
            y, v = np.where(move, y + v, y), np.where(move, v + 1, v)
        ground = np.isin(st[base + 3], (0, 4)) & (rng.random(n) < 0.7)
        st[base + 1], st[base + 2] = np.where(ground, 244, y), np.where(ground, 0, v)
        st[base + 4] = rng.integers(0, 5, n)
        st[base + 5] = rng.choice([-1, 1], n)
        st[base + 6] = rng.integers(0, 6, n)
        st[base + 7] = rng.integers(-1, 2, n)
        st[base + 8] = rng.integers(-1, 4, n)
        st[base + 9] = rng.integers(0, 2, n)
        st[base + 10] = rng.integers(0, 5, n)
        st[base + 11] = rng.integers(0, 2, n)
        st[base + 12] = rng.integers(0, 2, n)
    near = rng.random(n) < 0.5
    who = rng.random(n) < 0.5
    px, py = np.where(who, st[0], st[13]), np.where(who, st[1], st[14])
    st[26] = np.where(near, np.clip(px + rng.integers(-40, 41, n), 20, 432), rng.integers(20, 433, n))
    st[27] = np.where(near, np.clip(py + rng.integers(-40, 41, n), 0, 252), rng.integers(0, 253, n))
    st[28] = rng.integers(-20, 21, n)
    st[29] = np.where(rng.random(n) < 0.8, rng.integers(-120, 121, n), rng.integers(-300, 301, n))
    st[30] = rng.integers(0, 2, n)
    st[31], st[32] = rng.integers(20, 433, n), rng.integers(-100, 253, n)
    st[33], st[34] = rng.integers(20, 433, n), rng.integers(-100, 253, n)
    st[35] = rng.integers(0, 51, n)
    st[36] = rng.integers(20, 433, n)
    st[37] = rng.integers(20, 433, n)
    st[38], st[39] = rng.integers(0, 3, n), rng.integers(0, 3, n)
    st[40] = rng.integers(0, 2, n)
    st[43] = rng.integers(4, 1 << 20, n)
    return st


def plant_states(c, n=None):
    """(planted int32[44, n], over bool[n]): the start of configuration `c`'s launch, drawn from `c.seed` --
    random_valid_states, then (but on the matrix rows) scores below the winning score with a quarter of the games one
    point from the end, and an eighth of the games over: a winner at the winning score, game_ended and round_ended set.
    Those are reset in place before their first frame, or stay frozen without auto_reset."""
    n = c.n if n is None else n
    rng = np.random.default_rng(c.seed)
    ws = c.winning_score
    planted = random_valid_states(n, rng)
    over = rng.random(n) < 0.125
    winner = np.where(rng.random(n) < 0.5, 38, 39)
    if not c.matrix:
        planted[38:40] = rng.integers(0, ws, (2, n))
        near = np.flatnonzero(rng.random(n) < 0.25)
        planted[38 + rng.integers(0, 2, near.size), near] = ws - 1
    planted[winner[over], np.flatnonzero(over)] = ws
    planted[41][over] = planted[42][over] = 1
    return planted, over


def _with(row, levels: dict, name: str, seed: int, tables=None) -> Config:
    lv = dict(levels)
    lv.setdefault("action_format", "i32")
    stride = lv.pop("stride")
    return Config(entry=row.entry, k=row.k, above=row.above, packed=row.packed, p1=row.p1, p2=row.p2,
                  tables=tables or row.tables, kernel=row.kernel, name=name, seed=seed,
                  stride_pad=0 if stride == "n" else 64, **lv)


def _dispatches(row, levels: dict) -> bool:
    import kernel_matrix as km

    c = _with(row, dict(levels, stride="n+64"), "", 0)
    return km.dispatch(c.entry, c.k, c.n, c.fields(), c.stats_ptr, c.tables) == row.kernel


# starting points of the domain search: a PLAIN configuration, and two fused ones that are fused through different
# factors (so every single level can be tried on a fused form)
_BASES = (dict(simplify_action=0, shaping="off", normal_state_mode=0, episode_stats=0),
          dict(simplify_action=1, shaping="off", normal_state_mode=0, episode_stats=0),
          dict(simplify_action=0, shaping="off", normal_state_mode=0, episode_stats=2))
_NEUTRAL = dict(winning_score=3, serve="winner", auto_reset=1, ids="small", stride="n+64")


def applicable(f: str, row) -> bool:
    return f != "action_format" or row.entry == "pz_step"


def domain(row) -> dict:
    """factor -> the levels of the factor some configuration of `row`'s structure takes to `row.kernel`"""
    dom = {}
    for f, levels in FACTORS.items():
        if not applicable(f, row):
            continue
        ok = []
        for lv in levels:
            for base, fmt in itertools.product(_BASES, (OBS_I32, OBS_I16)):
                cand = dict(_NEUTRAL, obs_format=fmt, **base)
                cand[f] = lv
                if _dispatches(row, cand):
                    ok.append(lv)
                    break
        dom[f] = tuple(ok)
    return dom


def _pairs(levels: dict):
    items = sorted(levels.items())
    return {((f, a), (g, b)) for (f, a), (g, b) in itertools.combinations(items, 2)}


def required_pairs(doms) -> set:
    """the level pairs some instantiation of one side of the switch can take in one configuration"""
    out = set()
    for dom in doms:
        fs = sorted(dom)
        for f, g in itertools.combinations(fs, 2):
            out |= {((f, a), (g, b)) for a in dom[f] for b in dom[g]}
    return out


def _kernels():
    """[(kernel, [matrix rows])] in matrix order: a kernel that runs on both table modes has two rows"""
    import kernel_matrix as km

    by = {}
    for r in km.ROWS:
        by.setdefault(r.kernel, []).append(r)
    return list(by.items())


def _seed(name: str) -> int:
    h = zlib.crc32(name.encode())
    return (h * 0x9E3779B97F4A7C15 + 0x5DEECE66D) & 0xFFFFFFFFFFFFFFFF  # a full 64-bit seed


def _generate(seed: int):
    rng = random.Random(seed)
    kernels = _kernels()
    doms = {kernel: domain(rows[0]) for kernel, rows in kernels}
    covered = {False: set(), True: set()}
    out = []

    def emit(kernel, rows, levels):
        i = sum(1 for c in out if c.kernel == kernel)
        row = rows[i % len(rows)]
        name = f"{kernel} [{row.tables}] #{i}" if len(rows) > 1 else f"{kernel} #{i}"
        out.append(_with(row, levels, name, _seed(f"{name}/{seed}"), tables=row.tables))
        covered[row.above] |= _pairs(out[-1].levels())

    def draw(dom, fixed, prefer):
        for _ in range(400):
            cand = {f: (rng.choice(prefer[f]) if prefer.get(f) and rng.random() < 0.85 else rng.choice(dom[f]))
                    for f in dom}
            cand.update(fixed)
            yield cand

    for kernel, rows in kernels:
        dom, above = doms[kernel], rows[0].above
        need = {f: set(v) for f, v in dom.items()}
        made = 0
        while any(need.values()) or made < MIN_PER_KERNEL:
            best, best_score = None, -1
            tried = 0
            for cand in draw(dom, {}, {f: sorted(v, key=str) for f, v in need.items()}):
                if not _dispatches(rows[0], cand):
                    continue
                score = 1000 * sum(cand[f] in need[f] for f in need) + len(_pairs(cand) - covered[above])
                if score > best_score:
                    best, best_score = cand, score
                tried += 1
                if tried == 24:
                    break
            assert best is not None, kernel
            emit(kernel, rows, best)
            for f in need:
                need[f].discard(best[f])
            made += 1

    # the pairs no kernel's own configurations brought: one more configuration each, on a kernel that takes both
    for above in (False, True):
        side = [(kernel, rows) for kernel, rows in kernels if rows[0].above == above]
        for pair in sorted(required_pairs([doms[kr] for kr, _ in side]) - covered[above], key=str):
            if pair in covered[above]:
                continue
            (f, a), (g, b) = pair
            for kernel, rows in side:
                dom = doms[kernel]
                if a not in dom.get(f, ()) or b not in dom.get(g, ()):
                    continue
                cand = next((c for c in draw(dom, {f: a, g: b}, {}) if _dispatches(rows[0], c)), None)
                if cand is not None:
                    emit(kernel, rows, cand)
                    break
            else:
                raise AssertionError(f"no instantiation takes {pair}")
    return tuple(out), doms


SEED = int(os.environ.get("PZ_CONFIG_SEED", "20261016"))


@functools.lru_cache(maxsize=None)
def generated(seed: int = SEED):
    """(configurations, {kernel: domain}) of `seed`"""
    return _generate(seed)


def configs(seed: int = SEED):
    return generated(seed)[0]
