"""The step-kernel matrix: one launch configuration per step-kernel instantiation of the product library.

The C ABI picks one of the `step_kernel` / `step_pair_kernel` / `rollout_pair_kernel` instantiations at run time
(`launch_step` / `launch_pair` / `launch_step_players` in pika-zoo_amd/csrc/pz_kernels.hip) from the entry point, the
batch size (below or at/above `kTwoWaveMaxLanes`), the state format, the observation row type, whether the launch is
PLAIN (no fused wrapper, no statistics), the flight tables passed and the player mix.  `dispatch()` restates that choice;
`ROWS` walks the configuration space and keeps, for every instantiation reached, the first configuration that reaches
it (below the switch where one does), and for a computer-player kernel reached on the flight tables a second row on the
power-hit table alone (the same kernel, other paths inside it).

tests/test_gpu_kernel_matrix.py runs every row through the C ABI against the oracle and checks the kernel it
dispatched by name; tests/test_cabi_and_host.py checks that the rows name exactly the instantiations in the library.
Names are the demangled kernel names without `void `, `pz::` and the argument list (what tools/kernel_digest.py and
tools/kernel_notes.py print).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass

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


def dispatch(entry, k, n, packed, obs16, plain, tables, ai1, ai2) -> str:
    """The instantiation `launch_step<MODE>` launches for this configuration (product build)."""
    mode = _MODE[entry]
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
    # one wave; the k-frame launches have a PLAIN form, but for the human-vs-human rollout (kHhRolloutGeneric)
    plain_form = traj and plain and not (mode == _K_ROLLOUT and human)
    return _name("step_kernel", ai1, ai2, mode, sparse, _NO_SCOUT, False, traj and obs16, plain_form)


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


def _rows():
    seen, rows = {}, []
    # below the switch first (cheap rows), fused before PLAIN (more of the kernel exercised where the form is the same)
    for above, (entry, k), packed, obs16, plain, tables, (ai1, ai2) in itertools.product(
            (False, True), ENTRIES, (False, True), (False, True), (False, True), TABLE_MODES, MIXES):
        if tables != "none" and not (ai1 or ai2):
            continue  # no computer player: the tables are never consulted
        n = N_ABOVE if above else N_BELOW
        name = dispatch(entry, k, n, packed, obs16, plain, tables, ai1, ai2)
        if name in seen:
            continue
        cfg = dict(entry=entry, k=k, above=above, packed=packed, obs16=obs16, plain=plain, p1=ai1, p2=ai2, kernel=name)
        if tables == "both":
            assert dispatch(entry, k, n, packed, obs16, plain, "power_hit", ai1, ai2) == name
            seen[name] = [Row(tables="both", both_modes=True, **cfg), Row(tables="power_hit", both_modes=True, **cfg)]
        else:
            seen[name] = [Row(tables=tables, both_modes=False, **cfg)]
        rows += seen[name]
    return rows


ROWS = _rows()
KERNELS = frozenset(r.kernel for r in ROWS)
FAMILIES = ("step_kernel<", "step_pair_kernel<", "rollout_pair_kernel<")
