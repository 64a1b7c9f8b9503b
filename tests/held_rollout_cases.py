"""The cases of the held-trajectory tests (tests/test_held_rollout_host.py, tests/test_gpu_held_rollout.py): a covering
selection of the launches ``pz_step_many_held`` / ``pz_rollout_random_held`` take -- not the full product of

    hold {1, 2, 3, 4, 8} x k {1, 5, 32, 70, 130} x players x table modes x state formats x observation formats 0 - 6
    x auto_reset x fused stacks x batch shapes

but every value of every axis, every instantiation of ``held_traj_kernel`` at least once, and both entry points on every
player mix.  Nothing here needs a device.
"""
import dataclasses
import itertools

import numpy as np

TABLE = (0.0, -0.01, 0.0, 0.01, 0.0, 0.01, 0.0, -0.01)
PLAYERS = {"hh": (False, False), "hc": (False, True), "ch": (True, False), "cc": (True, True)}
N_ABOVE = 393216  # the single-frame launches' size switch: three slices of 512 lanes are judged there
STACKS = {
    # name: oracle keywords of the fused wrapper stack
    "plain": {},
    "int": dict(simplify_action=True, episode_stats=1),                                   # int32 rewards, raw statistics
    "float": dict(simplify_action=True, additional_reward=TABLE, episode_stats=2),        # float32 rewards, shaped statistics
    "nsm": dict(additional_reward=TABLE, normal_state_reward=0.125, normal_state_outside=True, episode_stats=1),
    "nsm_in": dict(simplify_action=True, additional_reward=TABLE, normal_state_reward=0.125, episode_stats=2),
}


@dataclasses.dataclass(frozen=True)
class Case:
    entry: str            # "many" (pz_step_many_held) / "rollout" (pz_rollout_random_held)
    hold: int
    k: int
    players: str = "hh"
    tables: str = "none"  # "both" / "power_hit" / "none"
    packed: bool = False
    obs_format: int = 0   # pz_obs_format 0 - 6
    auto_reset: bool = True
    stack: str = "plain"
    n: int = 256
    stride_pad: int = 0
    winning_score: int = 2
    preroll: int = 0      # frames of random play on the CPU oracle before the launch (short launches start mid-game)
    ends_twice: bool = False  # asserts that some game ended twice or more inside the launch
    seed: int = 7
    action_seed: int = 11
    t0: int = 0
    env_id_base: int = 0

    @property
    def id(self):
        bits = [self.entry, f"hold{self.hold}", f"k{self.k}", self.players, self.tables, "packed" if self.packed else "int32",
                f"obs{self.obs_format}", "reset" if self.auto_reset else "noreset", self.stack, f"n{self.n}+{self.stride_pad}",
                f"ws{self.winning_score}"]
        return "-".join(bits)

    @property
    def n_actions(self):
        return 13 if STACKS[self.stack].get("simplify_action") else 18

    @property
    def bites(self):
        """hold > 1 and k >= 16: the case must see games end inside a repeat, on its last frame, and come back"""
        return self.hold > 1 and self.k >= 16

    @property
    def kernel(self):
        p1, p2 = PLAYERS[self.players]
        return _name(p1, p2, 3 if self.entry == "many" else 2, self.packed, self.obs_format >= 2)

    # what tests/held_configs.py varies and these cases leave alone
    action_format = "i32"

    @property
    def stats_ptr(self):
        """a statistics pointer is passed (here: whenever the stack records statistics)"""
        return "episode_stats" in STACKS[self.stack]

    def start_state(self):
        """no planted state: the launch starts from reset plus `preroll` frames of random play"""
        return None

    def oracle_kwargs(self, env_id_base=None):
        p1, p2 = PLAYERS[self.players]
        return dict(winning_score=self.winning_score, is_player1_computer=p1, is_player2_computer=p2,
                    auto_reset=self.auto_reset, seed=self.seed, normalize_obs=self.obs_format in (1, 5, 6),
                    env_id_base=self.env_id_base if env_id_base is None else env_id_base, **STACKS[self.stack])


def _name(p1, p2, mode, packed, obs16):
    tf = {False: "false", True: "true"}
    return f"held_traj_kernel<{tf[p1]}, {tf[p2]}, {mode}, {tf[packed]}, {tf[obs16]}>"


def held_traj_kernels():
    """The instantiations the host can reach: players x {rollout = 2, tape = 3} x state format x row width"""
    tf = (False, True)
    return {_name(a, b, m, p, o) for a, b, m, p, o in itertools.product(tf, tf, (2, 3), tf, tf)}


def _cases():
    cases = []
    # 1. the cases that must bite (checked on the judge alone in tests/test_held_rollout_host.py): 256 games from reset,
    #    env seed 7, action seed 11, (hold, k) from {(2, 32), (4, 32), (8, 16), (3, 70)}, human/human and player 2 =
    #    computer; winning score 1 makes games end twice and more per launch
    bite = [(2, 32), (4, 32), (8, 16), (3, 70)]
    for idx, ((hold, k), players) in enumerate(itertools.product(bite, ("hh", "hc"))):
        tables = ("none", "both", "power_hit")[idx % 3] if players == "hc" else "none"
        cases.append(Case(entry=("many", "rollout")[idx % 2], hold=hold, k=k, players=players, tables=tables,
                          packed=bool(idx & 2), obs_format=(0, 1, 2, 5, 3, 6, 4, 0)[idx], auto_reset=idx != 5,
                          stack=("plain", "float", "int", "nsm", "float", "plain", "nsm_in", "int")[idx],
                          winning_score=1 if idx in (1, 2, 6, 7) else 2, ends_twice=idx in (1, 2, 6, 7)))
    # 2. every instantiation once more, on ragged batches with stride > n, over the other holds / ks (130 and 70 cross the
    #    64-step tape chunk); short launches start mid-game
    tf = (False, True)
    shapes = [(200, 56, 1), (264, 24, 1), (200, 56, 5), (264, 24, 5), (256, 0, 70), (256, 64, 130), (264, 24, 32)]
    holds = [1, 2, 3, 4, 8]
    for idx, (players, entry, packed, obs16) in enumerate(itertools.product(PLAYERS, ("rollout", "many"), tf, tf)):
        n, pad, k = shapes[idx % len(shapes)]
        hold = holds[idx % len(holds)]
        if k == 130 and hold == 8:
            hold = 2
        if obs16 and k > 1 and n % 8:
            n, pad = 264, 24
        fmt = ((2, 3, 4, 5, 6)[idx % 5]) if obs16 else idx % 2
        stack = ("plain", "int", "float", "nsm", "nsm_in")[(idx // 2) % 5]
        tables = "none" if players == "hh" else ("both", "power_hit", "none")[idx % 3]
        cases.append(Case(entry=entry, hold=hold, k=k, players=players, tables=tables, packed=packed, obs_format=fmt,
                          auto_reset=idx % 4 != 3, stack=stack, n=n, stride_pad=pad,
                          winning_score=1 if players == "cc" else 1 + idx % 2,  # (two computer players rally for long)
                          preroll=420 if players == "cc" else (0 if hold > 1 and k >= 16 and n == 256 else 90),
                          seed=3 + idx, action_seed=100 + idx,
                          t0=idx * 1000, env_id_base=(0, 2 ** 20, 2 ** 33 + 5)[idx % 3]))
    # 3. at the size switch of the single-frame launches: first, middle and last 512 lanes
    cases.append(Case(entry="rollout", hold=4, k=32, players="hc", tables="both", stack="float", obs_format=1, n=N_ABOVE,
                      stride_pad=64, winning_score=1))
    cases.append(Case(entry="many", hold=2, k=32, players="hh", packed=True, n=N_ABOVE + 64, winning_score=1))
    return cases


CASES = _cases()
# the biting cases on a whole small batch: their counts are asserted on the judge without a device too
BITING = [c for c in CASES if c.bites and c.n <= 4096]


def make_judge(oracle, case, lo=0, hi=None, nthreads=8):
    """The judge of lanes [lo, hi) of `case` at the start of the launch: reset, then the case's planted state
    (tests/held_configs.py) or `preroll` single frames of random play (their own action stream) with the configured
    auto_reset -- games are under way, some are over."""
    from frame_skip_judge import HeldOracle

    hi = case.n if hi is None else hi
    base = case.env_id_base + lo
    judge = HeldOracle(oracle, hi - lo, case.hold, oracle.make_config(**case.oracle_kwargs(base)), nthreads=nthreads)
    judge.reset()
    planted = case.start_state()
    if planted is not None:
        judge.env.state[:] = planted[:, lo:hi]
    for f in range(case.preroll):
        judge.env.step(*oracle.random_actions(hi - lo, base, case.action_seed ^ 0xABCD, f, case.n_actions))
    return judge


def policy(oracle, case, t, lo=0, hi=None):
    """the actions of policy step t of the launch, lanes [lo, hi): stream action_seed, index t0 + t"""
    hi = case.n if hi is None else hi
    return oracle.random_actions(hi - lo, case.env_id_base + lo, case.action_seed, case.t0 + t, case.n_actions)


def judge_counts(judge, terms):
    """(ended inside a repeat, ended on a repeat's last frame, terminated in slab t and running in slab t + 1, games that
    ended twice or more) from the judge's counters and its ``terminated`` of every slab ([k][n]).  With auto_reset a
    terminated slab is one ending: the game is reset before the next policy step."""
    terms = np.asarray(terms) != 0
    revived = int((terms[:-1] & ~terms[1:]).sum())
    twice = int((terms.sum(0) >= 2).sum()) if judge.auto_reset else 0
    return judge.ended_inside, judge.ended_last, revived, twice

