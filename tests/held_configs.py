"""The runtime configurations of the two frame-skip kernel families: ``hold_kernel<AI1, AI2, PACKED>`` (8 instantiations,
behind ``pz_step_held``) and ``held_traj_kernel<AI1, AI2, MODE, PACKED, OBS16>`` (32, behind ``pz_step_many_held`` /
``pz_rollout_random_held``) -- the counterpart of tests/kernel_configs.py, whose factors, levels, tables, ids and planting
recipe it reuses unchanged.  Host only: nothing here needs a device.

Structure (picks the kernel and the entry point): the player mix, the state format, the entry point and -- in a trajectory
launch -- the row width.  ``pz_step_held`` holds for 2 / 4 / 7 frames, STEP_LAUNCHES launches in a row; the trajectory
launches take (hold, k) from {2, 3, 4, 8} x {1, 5, 20, 70} (hold = 1 stays with tests/held_rollout_cases.py; k = 70
crosses the 64-step tape chunk).  Runtime: kernel_configs.FACTORS (``action_format`` on ``pz_step_held`` alone, the row
format within the instantiation's width), and the flight-table mode wherever a computer player exists.  Every launch
starts from kernel_configs.plant_states: random valid states, a quarter of the games one point from the end, an eighth
over.  ``generated()`` is deterministic (kernel_configs.SEED) and such that

  * every instantiation receives every level of every factor that applies to it, in at least MIN_PER_KERNEL configurations;
  * across each family, every pair of levels of two factors occurs in some configuration;
  * each configuration's row format agrees with its instantiation's OBS16;
  * each configuration BITES on the CPU judge alone (``misses()``: games end inside the launch and inside a repeat, come
    back with auto_reset, a shaped launch puts a ball on a line, the cancelling table meets RewardInNormalState ...), and
    every instantiation has a configuration with an ending on a repeat's last frame, every pz_rollout_random_held one a
    configuration whose policy index t0 + t crosses 2^32.  A drawn configuration that misses is drawn again under the
    next seed.

All of that is at n = kernel_matrix.N_BELOW; ABOVE adds one configuration per entry point at N_ABOVE.
tests/test_held_configs_host.py holds the generator to these rules; tests/test_gpu_held_configs.py launches every
configuration through the C ABI against the judge.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import random

import numpy as np

import kernel_configs as kc
from held_rollout_cases import _name, held_traj_kernels, judge_counts, make_judge, policy
from kernel_configs import FACTORS, IDS, MIN_PER_KERNEL, NORMAL_STATE_REWARD, SEED, SHAPING  # noqa: F401 (reused as they are)

STEP_HOLDS = (2, 4, 7)          # pz_step_held's k
STEP_LAUNCHES = 3               # ... launched this often in a row, each into its own output slot
HOLDS, KS = (2, 3, 4, 8), (1, 5, 20, 70)
TABLE_MODES = ("both", "power_hit", "none")
FAMILIES = ("hold_kernel<", "held_traj_kernel<")
REDRAWS = 8                     # seeds tried on one set of levels before other levels are drawn


def hold_kernels():
    tf = ("false", "true")
    return {f"hold_kernel<{a}, {b}, {p}>" for a in tf for b in tf for p in tf}


KERNELS = frozenset(hold_kernels() | held_traj_kernels())


@dataclasses.dataclass(frozen=True)
class Structure:
    entry: str      # "held" (pz_step_held) / "many" (pz_step_many_held) / "rollout" (pz_rollout_random_held)
    p1: bool
    p2: bool
    packed: bool
    obs16: object   # None: hold_kernel takes every row format at run time
    kernel: str

    @property
    def family(self) -> str:
        return self.kernel.split("<")[0] + "<"


def structures():
    """One per instantiation: the 8 hold kernels, then the 32 trajectory kernels"""
    tf = (False, True)
    out = [Structure("held", a, b, p, None, f"hold_kernel<{str(a).lower()}, {str(b).lower()}, {str(p).lower()}>")
           for a, b, p in itertools.product(tf, tf, tf)]
    out += [Structure(entry, a, b, p, o, _name(a, b, 3 if entry == "many" else 2, p, o))
            for a, b, entry, p, o in itertools.product(tf, tf, ("rollout", "many"), tf, tf)]
    return out


def domain(s: Structure) -> dict:
    """factor -> the levels instantiation `s` takes"""
    dom = {f: lv for f, lv in FACTORS.items() if f != "action_format" or s.entry == "held"}
    if s.obs16 is not None:
        dom["obs_format"] = tuple(f for f in FACTORS["obs_format"] if (f >= 2) == s.obs16)
    if s.p1 or s.p2:
        dom["tables"] = TABLE_MODES
    if s.entry == "held":
        dom["hold"] = STEP_HOLDS
    else:
        dom["hold"], dom["k"] = HOLDS, KS
    return dom


@dataclasses.dataclass(frozen=True)
class HeldConfig(kc.Config):
    """One launch (pz_step_held: STEP_LAUNCHES of them): a kernel_configs.Config with the frames an action is held for.
    `k` counts policy steps -- slabs of a trajectory launch, launches of pz_step_held.  It answers what
    held_rollout_cases.Case answers, so tests/test_gpu_held_rollout.py's harness launches and judges both."""
    hold: int = 1

    preroll, bites, ends_twice = 0, False, False  # the start is planted; what must happen inside is held by misses()

    @property
    def id(self) -> str:
        return self.name

    @property
    def n_actions(self) -> int:
        return 13 if self.simplify_action else 18

    @property
    def action_seed(self) -> int:
        return self.seed ^ 0x5EED

    def oracle_kwargs(self, env_id_base=None) -> dict:
        return dict(super().oracle_kwargs(), env_id_base=self.env_id_base if env_id_base is None else env_id_base)

    def start_state(self):
        return _planted(self.seed, self.n, self.winning_score)

    def levels(self) -> dict:
        lv = super().levels()  # (no action_format: that is pz_step's there)
        lv["hold"] = self.hold
        if self.entry == "held":
            lv["action_format"] = self.action_format
        else:
            lv["k"] = self.k
        if self.p1 or self.p2:
            lv["tables"] = self.tables
        return lv


@functools.lru_cache(maxsize=2)
def _planted(seed, n, winning_score):
    c = kc.Config(entry="", k=0, above=False, packed=False, p1=False, p2=False, tables="none", kernel="", name="",
                  seed=seed, winning_score=winning_score, serve="winner", auto_reset=1, simplify_action=0, shaping="off",
                  normal_state_mode=0, obs_format=0, episode_stats=0, action_format="i32", ids="small", stride_pad=0)
    planted = kc.plant_states(c, n)[0]
    planted.setflags(write=False)
    return planted


def make(s: Structure, levels: dict, name: str, seed: int, above=False) -> HeldConfig:
    lv = dict(levels)
    lv.setdefault("action_format", "i32")
    stride = lv.pop("stride")
    return HeldConfig(entry=s.entry, k=lv.pop("k", STEP_LAUNCHES), above=above, packed=s.packed, p1=s.p1, p2=s.p2,
                      tables=lv.pop("tables", "none"), kernel=s.kernel, name=name, seed=seed,
                      stride_pad=0 if stride == "n" else 64, **lv)


# ---- what a configuration does on the judge alone -------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Facts:
    ended_inside: int      # games that ended on a frame before a repeat's last (the rest of the repeat is frozen)
    ended_last: int        # ... on a repeat's last frame
    revived: int           # terminated in slab t, running in slab t + 1
    on_line: bool          # a post-step ball of a non-frozen game exactly on x_line or y_line (shaped launches)
    cancelled: bool        # a frame whose point the cancelling table took to 0 and RewardInNormalState replaced


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


def frame_watch(po, c, seen: dict):
    """HeldOracle.on_frame for `c`: check_config's two in-launch conditions, frame by frame inside the judge.
    seen["on_line"]: the post-step ball of a game the frame did not find frozen sits exactly on a shaping line;
    seen["cancelled"] (the cancelling table under RewardInNormalState outside): a ball on the ground -- a point, +-1
    taken to exactly 0 by the table -- left both players RewardInNormalState's constant."""
    table, x_line, y_line = SHAPING[c.shaping] or (None, None, None)
    nsr = np.float32(NORMAL_STATE_REWARD)
    replaced = c.shaping == "cancel" and c.normal_state_mode == 2

    def on_frame(j, env, frozen):
        if table is None:
            return
        live = ~frozen
        bx, by = env.state[po.B_X], env.state[po.B_Y]
        seen["on_line"] = seen.get("on_line", False) or bool((live & ((bx == x_line) | (by == y_line))).any())
        if replaced:
            hit = live & (by == 252) & (env.rew[0] == nsr) & (env.rew[1] == nsr)
            seen["cancelled"] = seen.get("cancelled", False) or bool(hit.any())

    return on_frame


@functools.lru_cache(maxsize=None)
def measure(c: HeldConfig) -> Facts:
    """`c` on the CPU judge (tests/frame_skip_judge.py), every lane: 10 - 50 ms below the switch"""
    po = _oracle()
    judge = make_judge(po, c)
    seen = {}
    judge.on_frame = frame_watch(po, c, seen)
    terms = [judge.step(*policy(po, c, t))[2].copy() for t in range(c.k)]
    inside, last, revived, _ = judge_counts(judge, np.stack(terms))
    return Facts(inside, last, revived, seen.get("on_line", False), seen.get("cancelled", False))


def misses(c: HeldConfig, f: Facts) -> list:
    """The conditions of a below-switch configuration that `f` does not meet (empty: the configuration bites)"""
    out = []
    if f.ended_inside + f.ended_last == 0:
        out.append("no game terminates inside the launch")
    if c.hold >= 2 and f.ended_inside == 0:
        out.append("no game ends inside a repeat")
    if c.auto_reset and c.k >= 5 and f.revived == 0:
        out.append("no game terminated in one slab and running in the next")
    if c.shaped and not f.on_line:
        out.append("no post-step ball of a running game on a shaping line")
    if c.shaping == "cancel" and c.normal_state_mode == 2 and not f.cancelled:
        out.append("no point cancelled by the table and replaced by RewardInNormalState")
    if c.ids == "large":
        if (c.env_id_base + c.n - 1) >> 32 == c.env_id_base >> 32:
            out.append("the low id word does not wrap inside the launch")
        if c.entry == "rollout" and c.k >= 3 and not c.t0 < 1 << 32 <= c.t0 + c.k - 1:
            out.append("t0 + t does not cross 2^32 inside the launch")
    return out


# ---- the generator --------------------------------------------------------------------------------------------------
def _generate(seed: int):
    rng = random.Random(seed)
    structs = structures()
    doms = {s.kernel: domain(s) for s in structs}
    covered = {fam: set() for fam in FAMILIES}
    out = []

    def draw(dom, fixed, prefer):
        for _ in range(400):
            cand = {f: (rng.choice(prefer[f]) if prefer.get(f) and rng.random() < 0.85 else rng.choice(dom[f]))
                    for f in dom}
            cand.update(fixed)
            yield cand

    def emit(s, levels):
        """`levels` on `s` under the first of REDRAWS seeds that bites; None if none does"""
        name = f"{s.kernel} #{sum(1 for c in out if c.kernel == s.kernel)}"
        for attempt in range(REDRAWS):
            c = make(s, levels, name, kc._seed(f"{name}/{seed}/{attempt}"))
            if not misses(c, measure(c)):
                out.append(c)
                covered[s.family] |= kc._pairs(c.levels())
                return c
        return None

    for s in structs:
        dom = doms[s.kernel]
        need = {f: set(v) for f, v in dom.items()}
        made, last, crossed = 0, False, s.entry != "rollout"
        for _ in range(200):
            if not (any(need.values()) or made < MIN_PER_KERNEL or not last or not crossed):
                break
            # a rollout kernel whose own configurations never took the policy index across 2^32: one that does
            fixed = {} if crossed or any(need.values()) else dict(ids="large", k=rng.choice([k for k in KS if k >= 3]))
            best, best_score = None, -1
            for cand in itertools.islice(draw(dom, fixed, {f: sorted(v, key=str) for f, v in need.items()}), 24):
                score = 1000 * sum(cand[f] in need[f] for f in need) + len(kc._pairs(cand) - covered[s.family])
                if score > best_score:
                    best, best_score = cand, score
            c = emit(s, best)
            if c is None:
                continue  # these levels miss under every seed tried: the next draw differs (the stream moved on)
            for f in need:
                need[f].discard(best[f])
            made += 1
            last = last or measure(c).ended_last > 0
            crossed = crossed or (c.ids == "large" and c.k >= 3)
        else:
            raise AssertionError(f"{s.kernel}: no covering set of biting configurations")

    # the pairs no kernel's own configurations brought: one more configuration each, on a kernel that takes both
    for fam in FAMILIES:
        side = [s for s in structs if s.family == fam]
        for pair in sorted(kc.required_pairs([doms[s.kernel] for s in side]) - covered[fam], key=str):
            if pair in covered[fam]:
                continue
            (f, a), (g, b) = pair
            takers = [s for s in side if a in doms[s.kernel].get(f, ()) and b in doms[s.kernel].get(g, ())]
            assert takers, f"no instantiation takes {pair}"
            if not any(emit(s, cand) for s in takers
                       for cand in itertools.islice(draw(doms[s.kernel], {f: a, g: b}, {}), 4)):
                raise AssertionError(f"no biting configuration with {pair}")
    return tuple(out), doms


def _above(seed: int):
    """One configuration per entry point at N_ABOVE: short launches (the judge runs every lane of them)"""
    by_kernel = {s.kernel: s for s in structures()}
    levels = {
        "hold_kernel<false, true, false>": dict(
            hold=4, action_format="i64", obs_format=5, tables="power_hit", shaping="shifted", episode_stats=2,
            serve="random", normal_state_mode=1, stride="n"),
        "held_traj_kernel<false, true, 3, true, false>": dict(
            hold=2, k=5, obs_format=1, tables="none", shaping="cancel", episode_stats=1, serve="alternate",
            normal_state_mode=2, stride="n+64"),
        "held_traj_kernel<false, true, 2, false, true>": dict(
            hold=3, k=5, obs_format=4, tables="both", shaping="off", episode_stats="1-null", serve="random",
            normal_state_mode=0, stride="n"),
    }
    out = []
    for kernel, lv in levels.items():
        s = by_kernel[kernel]
        name = f"{s.kernel} @above"
        out.append(make(s, dict(lv, winning_score=3, auto_reset=1, simplify_action=1, ids="large"), name,
                        kc._seed(f"{name}/{seed}"), above=True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def generated(seed: int = SEED):
    """(configurations below the switch, {kernel: domain}) of `seed`"""
    return _generate(seed)


def configs(seed: int = SEED):
    """every configuration tests/test_gpu_held_configs.py launches: the generated ones, then ABOVE's three"""
    return generated(seed)[0] + _above(seed)
