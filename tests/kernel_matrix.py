"""The step-kernel matrix: one launch configuration per step-kernel instantiation of the product library.

The C ABI picks one of the `step_kernel` / `step_pair_kernel` / `rollout_pair_kernel` instantiations at run time
(`choose_step_kernel()` in pika-zoo_amd/csrc/pz_dispatch.hpp; the library builds exactly its image) from the entry
point, the batch size (below or at/above `kTwoWaveMaxLanes`), the state format, the observation row type, whether the
launch is PLAIN (no fused wrapper, no statistics: tests/kernel_configs.py `is_plain()`, worked out from the configuration
and the statistics pointer), the flight tables passed and the player mix.  `dispatch()` restates that choice
independently (tests/test_dispatch_host.py holds the C++ against it on the host); `ROWS` walks the configuration space
and keeps, for every instantiation reached, the first configuration that reaches it (below the switch where one does),
and for a computer-player kernel reached on the flight tables a second row on the power-hit table alone (the same
kernel, other paths inside it).

tests/test_gpu_kernel_matrix.py runs every row through the C ABI against the oracle, under the row's fixed recipe
(`Row.config()`), and checks the kernel it dispatched by name (tests/kernel_configs.py holds the other runtime
configurations of every instantiation); tests/test_cabi_and_host.py checks that the rows name exactly the
instantiations in the library.
Names are the demangled kernel names without `void `, `pz::` and the argument list (what tools/kernel_digest.py and
tools/kernel_notes.py print).
"""
from __future__ import annotations

import itertools
import zlib
from dataclasses import dataclass

from kernel_configs import Config, config_fields, is_plain

SWITCH = 393216                 # kTwoWaveMaxLanes: from here on the single-wave kernels
N_BELOW = 64 * 37 + 8           # ragged, a multiple of 8 (int16 rows of a k-frame launch)
N_ABOVE = SWITCH + 8            # the single-wave kernels' last workgroup is partial
STRIDE_PAD = 64

# (entry point, k): pz_step_random dispatches other kernels for k = 1 and k > 1; pz_step_many crosses the tape's
# 64-frame refill
ENTRIES = (("pz_step", 1), ("pz_step_random", 1), ("pz_step_random", 5), ("pz_rollout_random", 20),
           ("pz_step_many", 70))
MIXES = ((False, False), (False, True), (True, False), (True, True))  # (player 1, player 2) is a computer
TABLE_MODES = ("both", "power_hit", "none")

# template arguments (pz_kernels.hip: StepMode, pz_physics.hpp: ScoutMode)
_MODE = {"pz_step": 0, "pz_step_random": 1, "pz_rollout_random": 2, "pz_step_many": 3}
_K_ACTIONS, _K_RANDOM, _K_ROLLOUT, _K_TAPE = 0, 1, 2, 3
_NO_SCOUT, _SCOUT_LOADS, _SCOUT_POSTED = 0, 1, 2


def _b(v) -> str:
    return "true" if v else "false"


def _name(family: str, *args) -> str:
    return f"{family}<{', '.join(_b(a) if isinstance(a, bool) else str(a) for a in args)}>"


def dispatch(entry, k, n, cfg, stats, tables) -> str:
    """The instantiation `choose_step_kernel()` picks for this configuration (product build).  `cfg`: the pz_config
    words of kernel_configs.config_fields(); `stats`: a statistics pointer is passed; `tables`: TABLE_MODES."""
    mode = _MODE[entry]
    packed, obs16 = bool(cfg["packed_state"]), cfg["normalize_obs"] >= 2  # rows16(): formats 2 - 6
    plain = is_plain(cfg, stats)
    ai1, ai2 = bool(cfg["p1_computer"]), bool(cfg["p2_computer"])
    traj = mode in (_K_ROLLOUT, _K_TAPE)
    small = n < SWITCH
    hit = tables != "none"
    human = not (ai1 or ai2)
    # the pair kernel: one frame, below the switch or packed, on the tables or human vs human
    if (small or packed) and (hit or human) and (mode == _K_ACTIONS or (mode == _K_RANDOM and k == 1)):
        return _name("step_pair_kernel", ai1, ai2, packed, mode == _K_RANDOM)
    # the k-frame launches on two waves: a computer player on the tables, or human vs human on int16 rows
    if traj and small and ((hit and not human) or (human and obs16)):
        if packed:
            return _name("rollout_pair_kernel", ai1, ai2, mode, True, obs16, False)
        return _name("rollout_pair_kernel", ai1, ai2, mode, False, obs16, plain)
    if packed:  # one wave, the packed format: no scout, no PLAIN form
        return _name("step_kernel", ai1, ai2, mode, False, _NO_SCOUT, True, traj and obs16, False)
    sparse = mode in (_K_ACTIONS, _K_RANDOM)
    if small and not hit and not human:  # the scout wave computes the flights beside the frame
        scout = _SCOUT_LOADS if mode == _K_ACTIONS else _SCOUT_POSTED
        return _name("step_kernel", ai1, ai2, mode, sparse, scout, False, traj and obs16, False)
    # one wave; the k-frame launches have a PLAIN form, but for the human-vs-human rollout (measured slower there)
    plain_form = traj and plain and not (mode == _K_ROLLOUT and human)
    return _name("step_kernel", ai1, ai2, mode, sparse, _NO_SCOUT, False, traj and obs16, plain_form)


def recipe(packed, obs16, plain, p1, p2) -> dict:
    """The pz_config words of a matrix row: PLAIN (no wrapper, no statistics) or the fused recipe -- SimplifyAction,
    RewardByBallPosition, RecordEpisodeStatistics on the env's reward, NormalizeObservation where both players are of
    one kind and the rows are int32"""
    fused = not plain
    fmt = 2 if obs16 else (1 if fused and p1 == p2 else 0)
    return config_fields(p1_computer=p1, p2_computer=p2, packed_state=packed, normalize_obs=fmt, simplify_action=fused,
                         ballpos_reward=fused, episode_stats_mode=int(fused))


@dataclass(frozen=True)
class Row:
    entry: str
    k: int
    above: bool        # n at/above the switch
    packed: bool       # the packed state format
    obs16: bool        # int16 observation rows (normalize_obs == 2)
    plain: bool        # no fused wrapper, no statistics
    tables: str        # TABLE_MODES
    p1: bool           # player 1 is a computer
    p2: bool           # player 2 is a computer
    kernel: str        # the instantiation it must dispatch
    both_modes: bool   # the kernel runs a row on both tables and one on the power-hit table alone

    @property
    def n(self) -> int:
        return N_ABOVE if self.above else N_BELOW

    @property
    def stride(self) -> int:
        return self.n + STRIDE_PAD

    @property
    def id(self) -> str:
        return f"{self.kernel} [{self.tables}]" if self.both_modes else self.kernel

    @property
    def cfg(self) -> dict:
        return recipe(self.packed, self.obs16, self.plain, self.p1, self.p2)

    @property
    def stats(self) -> bool:
        return not self.plain  # the fused recipe passes a statistics pointer

    def config(self) -> Config:
        """The row as a kernel_configs.Config: winning score 3, random serve (fused) or the winner's, auto-reset, lanes
        from 2^20, stride n + STRIDE_PAD"""
        fused = not self.plain
        return Config(entry=self.entry, k=self.k, above=self.above, packed=self.packed, p1=self.p1, p2=self.p2,
                      tables=self.tables, kernel=self.kernel, name=self.id, seed=zlib.crc32(self.id.encode()),
                      winning_score=3, serve="random" if fused else "winner", auto_reset=1, simplify_action=int(fused),
                      shaping="default" if fused else "off", normal_state_mode=0,
                      obs_format=self.cfg["normalize_obs"], episode_stats=int(fused), action_format="i32", ids="small",
                      stride_pad=STRIDE_PAD, matrix=True)


def _rows():
    seen, rows = {}, []
    # below the switch first (cheap rows), fused before PLAIN (more of the kernel exercised where the form is the same)
    for above, (entry, k), packed, obs16, plain, tables, (ai1, ai2) in itertools.product(
            (False, True), ENTRIES, (False, True), (False, True), (False, True), TABLE_MODES, MIXES):
        if tables != "none" and not (ai1 or ai2):
            continue  # no computer player: the tables are never consulted
        n = N_ABOVE if above else N_BELOW
        name = dispatch(entry, k, n, recipe(packed, obs16, plain, ai1, ai2), not plain, tables)
        if name in seen:
            continue
        cfg = dict(entry=entry, k=k, above=above, packed=packed, obs16=obs16, plain=plain, p1=ai1, p2=ai2, kernel=name)
        if tables == "both":
            assert dispatch(entry, k, n, recipe(packed, obs16, plain, ai1, ai2), not plain, "power_hit") == name
            seen[name] = [Row(tables="both", both_modes=True, **cfg), Row(tables="power_hit", both_modes=True, **cfg)]
        else:
            seen[name] = [Row(tables=tables, both_modes=False, **cfg)]
        rows += seen[name]
    return rows


ROWS = _rows()
KERNELS = frozenset(r.kernel for r in ROWS)
FAMILIES = ("step_kernel<", "step_pair_kernel<", "rollout_pair_kernel<")
