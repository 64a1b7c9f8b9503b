"""League matchmaking on the device: the results of the games that ended on a step, accumulated per pair of pool members in
ONE launch, and a member per game drawn with integer weights from a counter in ONE launch.

    from pikazoo_amd import league, pool
    snapshots = pool.Snapshots(model, capacity=8)
    mm = league.Matchmaker(snapshots, num_envs=n, seed=0)
    plan = mm.rematch()                                          # PFSP weights -> draw -> pool.plan: opponents for every game
    head = snapshots.act(obs, {"player_1": None, "player_2": plan})
    obs, rewards, terminations, _, _ = env.step(actions)
    mm.record(terminations["player_1"], env.scores)              # right after env.step: the terminal frame's scores
    mm.win_rates()                                               # the learner's rate against each member, on the device

    table = league.tally(terminations, env.scores, members, P)   # int64 [P, P, 4]: games, wins of player_1, points, points
    members = league.draw(weights, n, seed=0, counter=c)         # int64 [n]; reproducible from (seed, counter, first_game)
    weights = league.pfsp_weights(table, active=P)               # prioritised fictitious self-play, or any int64 [P] of yours

ctypes binding of libpikazoo_league.so (C ABI and the definitions: include/pikazoo_league.h), a library of its own beside the
product library; nothing in the step path or in the other modules imports this one, and importing it loads nothing and imports
none of them (``Matchmaker`` imports ``pool`` when it is made).  There
is no torch fallback: a missing or stale library raises.  Both launches are integer arithmetic, fixed bit for bit by the
header; they allocate nothing and do not synchronise, so they can be captured in a graph, and a counter given as a device
tensor is read at run time.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _launch, _native
from ._launch import describe as _describe

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_league.so"
ABI_VERSION = 1
MAX_MEMBERS = 16
CELL_WORDS = 4
MAX_GAMES = 1 << 30
SCORE_FORMATS = {torch.int32: 0, torch.int16: 1}
# the VALUES of pz_pool_member_format (include/pikazoo_pool.h)
MEMBER_FORMATS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
KEY_XOR = (0x4C454147, 0x44524157)
WEIGHT_ONE = 1 << 20    # pfsp_weights: the weight of a member the learner never beats

_P = C.c_void_p

SIGNATURES = {
    "pz_league_abi_version": (C.c_int, []),
    "pz_league_build_id": (C.c_char_p, []),
    # (terminated, score_p1, score_p2, score_format, score_stride, members_p1, members_p2, member_format, n, num_members, table, errors, stream)
    "pz_league_tally": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]),
    # (weights, num_members, seed, counter, counter_dev, first_game, mask, members, member_format, n, errors, stream)
    "pz_league_draw": (C.c_int, [_P, C.c_int32, C.c_uint64, C.c_uint64, _P, C.c_int64, _P, _P, C.c_int32, C.c_int64, _P, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a count, a stride or a counter beyond the kernel's range", -3: "an unknown score or member format"}
_lib = None


def load():
    """Load libpikazoo_league.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_league.hip", SIGNATURES, "pz_league_abi_version", ABI_VERSION)
    return _lib


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def _num_members(num_members):
    if not _is_int(num_members) or not 1 <= num_members <= MAX_MEMBERS:
        raise ValueError(f"num_members must be an integer in 1..{MAX_MEMBERS}, got {num_members!r}")
    return num_members


def _flags(t, what, n=None):
    """a contiguous [n] bool or uint8 vector"""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous one-dimensional bool or uint8 tensor, got {_describe(t)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{what} must have {n} elements, got {t.shape[0]}")
    return t


def _member_vector(t, what, n):
    if not isinstance(t, torch.Tensor) or t.dtype not in MEMBER_FORMATS or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous one-dimensional {' or '.join(str(d) for d in MEMBER_FORMATS)} tensor, got {_describe(t)}")
    if t.shape[0] != n:
        raise ValueError(f"{what} must have {n} elements, got {t.shape[0]}")
    return t


def _one_device(tensors):
    dev = tensors[0][1].device
    for name, t in tensors:
        if t.device != dev:
            raise ValueError(f"every tensor must be on one device: {tensors[0][0]} is on {dev}, {name} on {t.device}")
    return dev


def _need_gpu(dev):
    if dev.type != "cuda":
        raise ValueError(f"the league launches run on the GPU: the tensors are on {dev}")


# ---- the tally -----------------------------------------------------------------------------------------------------------------
def tally(terminations, scores, members, num_members, table=None, members_p1=None, errors=None):
    """Add the results of the games that ended on this step to ``table``, in one launch (``pz_league_tally``): for every game
    ``g`` with ``terminations[g]``, with ``a = members_p1[g]`` (0 without ``members_p1``) and ``b = members[g]``, ``table[a, b]
    += (1, scores[g, 0] > scores[g, 1], scores[g, 0], scores[g, 1])``.  A game whose ``a`` or ``b`` lies outside ``[0,
    num_members)`` adds 1 to ``errors`` instead.  Returns ``table``.

    ``terminations``: ``[n]`` bool or uint8, contiguous.  ``scores``: ``env.scores`` of either state format, called right
    after ``env.step`` (with ``auto_reset`` the state still holds the terminal frame's scores then), or any ``[n, 2]`` int32 /
    int16 tensor: its two columns are read at the one element stride of its first dimension.  ``members`` / ``members_p1``:
    ``[n]`` uint8, int32 or int64 of one dtype, contiguous.  ``table``: int64 ``[num_members, num_members, 4]``, contiguous,
    ACCUMULATED (zeros are allocated when it is ``None``); ``errors``: int64 of one element, ACCUMULATED (optional: a word is
    allocated when it is ``None``, and dropped).  Scores and members of games that did not end are not looked at.

    No synchronisation; with ``table`` and ``errors`` given, no allocation.  Every shape, dtype, device or stride that the
    launch cannot take raises ``ValueError`` before any launch."""
    P = _num_members(num_members)
    _flags(terminations, "terminations")
    n = int(terminations.shape[0])
    if n > MAX_GAMES:
        raise ValueError(f"at most 2^30 games, got {n}")
    if not isinstance(scores, torch.Tensor) or scores.dtype not in SCORE_FORMATS or scores.dim() != 2 or tuple(scores.shape) != (n, 2):
        raise ValueError(f"scores must be an int32 or int16 [{n}, 2] tensor, got {_describe(scores)}")
    stride = int(scores.stride(0)) if n > 1 else max(1, int(scores.stride(0)))
    if stride < 1 or scores.stride(1) < 0:
        raise ValueError(f"scores: the games of a column must lie at one positive element stride, got strides {list(scores.stride())}")
    _member_vector(members, "members", n)
    if members_p1 is not None:
        _member_vector(members_p1, "members_p1", n)
        if members_p1.dtype != members.dtype:
            raise ValueError(f"members_p1 is {members_p1.dtype}, members is {members.dtype}: one dtype for both sides")
    if table is not None and (not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or tuple(table.shape) != (P, P, CELL_WORDS)
                              or not table.is_contiguous()):
        raise ValueError(f"table must be a contiguous int64 [{P}, {P}, {CELL_WORDS}] tensor, got {_describe(table)}")
    if errors is not None and (not isinstance(errors, torch.Tensor) or errors.dtype != torch.int64 or errors.numel() != 1):
        raise ValueError(f"errors must be one int64 element, got {_describe(errors)}")
    given = [("terminations", terminations), ("scores", scores), ("members", members)] + [
        (name, t) for name, t in (("members_p1", members_p1), ("table", table), ("errors", errors)) if t is not None]
    dev = _one_device(given)
    outputs = [(name, t) for name, t in (("table", table), ("errors", errors)) if t is not None]
    if outputs:
        _launch.no_alias(outputs, [(name, t) for name, t in given if name not in ("table", "errors")])
    _need_gpu(dev)
    if table is None:
        table = torch.zeros((P, P, CELL_WORDS), dtype=torch.int64, device=dev)
    if errors is None:
        errors = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return table
    _launch.launch(load().pz_league_tally, _ERRORS, dev, terminations.data_ptr(), scores.data_ptr(),
                   scores.data_ptr() + int(scores.stride(1)) * scores.element_size(), SCORE_FORMATS[scores.dtype], stride,
                   members_p1.data_ptr() if members_p1 is not None else None, members.data_ptr(), MEMBER_FORMATS[members.dtype], n, P,
                   table.data_ptr(), errors.data_ptr())
    return table


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def draw(weights, n, seed, counter=0, first_game=0, mask=None, out=None, dtype=torch.int64, errors=None):
    """A pool member per game, drawn with integer weights, in one launch (``pz_league_draw``; the definition is
    include/pikazoo_league.h's): game ``g`` gets member ``p`` with probability ``weights[p] / sum(weights)``, from the Philox
    block of ``(seed, counter, first_game + g)``.  The same arguments give the same members, on any device, in any sharding.

    ``weights``: int64 ``[P]`` on the GPU, ``1 <= P <= 16``, every weight in ``[0, 2^32)`` and not all zero -- otherwise the
    launch writes NO member and sets ``errors`` (an int32 device tensor of one element, never cleared here) to 1.  A member of
    weight 0 is never drawn.  ``counter``: an int in ``[0, 2^62)`` or an int64 device tensor of one element that the kernel
    reads when it runs (the form for a captured graph: increment it between replays).  ``first_game``: the global id of game
    0, so that a shard draws what the whole batch draws.  ``mask``: ``[n]`` bool or uint8; only games with ``mask[g] != 0``
    are drawn, the others keep what ``out`` holds.  ``out=``: a contiguous ``[n]`` uint8, int32 or int64 tensor to draw into
    (nothing is allocated then but the ``errors`` word when it is ``None``); without it an ``[n]`` tensor of ``dtype`` is
    allocated (zeros, when there is a mask).  Returns the members.

    No synchronisation.  Every shape, dtype, device or range that the launch cannot take raises ``ValueError`` before any
    launch."""
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.int64 or weights.dim() != 1 or not weights.is_contiguous() \
            or not 1 <= weights.shape[0] <= MAX_MEMBERS:
        raise ValueError(f"weights must be a contiguous int64 [P] tensor with 1 <= P <= {MAX_MEMBERS}, got {_describe(weights)}")
    P = int(weights.shape[0])
    if not _is_int(n) or not 0 <= n <= MAX_GAMES:
        raise ValueError(f"n must be an integer in [0, 2^30], got {n!r}")
    if not _is_int(seed):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    counter_dev = None
    if isinstance(counter, torch.Tensor):
        if counter.dtype != torch.int64 or counter.numel() != 1:
            raise ValueError(f"a counter on the device must be one int64 element, got {_describe(counter)}")
        counter_dev, counter = counter, 0
    elif not _is_int(counter) or not 0 <= counter < 1 << 62:
        raise ValueError(f"counter must be an integer in [0, 2^62) or an int64 device tensor of one element, got {counter!r}")
    if not _is_int(first_game) or not -(1 << 63) <= first_game < 1 << 63:
        raise ValueError(f"first_game must be an integer that fits int64, got {first_game!r}")
    if mask is not None:
        _flags(mask, "mask", n)
    if out is not None:
        _member_vector(out, "out", n)
    elif dtype not in MEMBER_FORMATS:
        raise ValueError(f"dtype must be {' or '.join(str(d) for d in MEMBER_FORMATS)}, got {dtype!r}")
    if errors is not None and (not isinstance(errors, torch.Tensor) or errors.dtype != torch.int32 or errors.numel() != 1):
        raise ValueError(f"errors must be one int32 element, got {_describe(errors)}")
    given = [("weights", weights)] + [(name, t) for name, t in (("counter", counter_dev), ("mask", mask), ("out", out), ("errors", errors))
                                      if t is not None]
    dev = _one_device(given)
    outputs = [(name, t) for name, t in (("out", out), ("errors", errors)) if t is not None]
    if outputs:
        _launch.no_alias(outputs, [(name, t) for name, t in given if name not in ("out", "errors")])
    _need_gpu(dev)
    if out is None:
        out = (torch.zeros if mask is not None else torch.empty)(n, dtype=dtype, device=dev)
    if errors is None:
        errors = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    _launch.launch(load().pz_league_draw, _ERRORS, dev, weights.data_ptr(), P, seed & 0xFFFFFFFFFFFFFFFF, counter,
                   counter_dev.data_ptr() if counter_dev is not None else None, first_game, mask.data_ptr() if mask is not None else None,
                   out.data_ptr(), MEMBER_FORMATS[out.dtype], n, errors.data_ptr())
    return out


# ---- the one policy choice ---------------------------------------------------------------------------------------------------
def pfsp_weights(table, active, power=2.0, prior_games=8.0, row=0):
    """Prioritised fictitious self-play: int64 ``[P]`` weights for :func:`draw` from a :func:`tally` table, on the table's
    device, without a synchronisation (a handful of torch operations on ``P`` elements: not a kernel of this library).

    In float64, from the side of member ``row`` as ``player_1``: ``w = (wins + prior_games / 2) / (games + prior_games)`` is
    its smoothed win rate against each member, and the weight is ``max(1, round((1 - w) ** power * 2^20))`` for members below
    ``active`` and 0 from there on: members that ``row`` loses to are drawn more often, a member without games counts as an
    even match, and no active member is ever starved.  Any other int64 weights serve :func:`draw` as well."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.dim() != 3 or table.shape[0] != table.shape[1] \
            or table.shape[2] != CELL_WORDS or not 1 <= table.shape[0] <= MAX_MEMBERS:
        raise ValueError(f"table must be an int64 [P, P, {CELL_WORDS}] tensor with 1 <= P <= {MAX_MEMBERS}, got {_describe(table)}")
    P = int(table.shape[0])
    if not _is_int(active) or not 1 <= active <= P:
        raise ValueError(f"active must be an integer in 1..{P}, got {active!r}")
    if not _is_int(row) or not 0 <= row < P:
        raise ValueError(f"row must be an integer in 0..{P - 1}, got {row!r}")
    if isinstance(power, bool) or not isinstance(power, (int, float)) or not power >= 0:
        raise ValueError(f"power must be a number >= 0, got {power!r}")
    if isinstance(prior_games, bool) or not isinstance(prior_games, (int, float)) or not prior_games > 0:
        raise ValueError(f"prior_games must be a number > 0, got {prior_games!r}")
    games = table[row, :, 0].to(torch.float64)
    wins = table[row, :, 1].to(torch.float64)
    rate = (wins + prior_games / 2) / (games + prior_games)
    weights = torch.round((1.0 - rate).clamp(0.0, 1.0) ** power * WEIGHT_ONE).to(torch.int64).clamp_(min=1)
    weights[active:] = 0
    return weights


# ---- the matchmaker ----------------------------------------------------------------------------------------------------------
class Matchmaker:
    """Results and opponents of a league around a ``pool.Snapshots``: ``player_1`` of every game is the learner (member 0),
    ``player_2`` the member this object drew for that game.

    It owns ``table`` (int64 ``[capacity, capacity, 4]``, zeros), ``members`` (int64 ``[num_envs]``, zeros: everyone plays
    the learner until the first :meth:`rematch`), a device ``counter`` (int64 ``[1]``), an errors word per launch
    (``tally_errors`` int64, ``draw_errors`` int32) and one ``pool.Plan`` per pool size.

    :meth:`record` is one launch; :meth:`rematch` is a handful of torch operations on ``capacity`` elements, one draw launch
    and one ``pool.plan``.  The plan is the expensive part: one workgroup walks all ``num_envs`` members twice, 8.9-11.2 us
    at 4 096 games, 105-108 us at 65 536 and 893-901 us at 524 288 on the MI355X (README's row of the pool), against a pool
    forward of 20 / 45-61 / 298-327 us at those sizes.  So ``rematch(mask=terminations)`` on every step -- a new opponent as
    soon as a game ends -- suits small batches, and ``rematch()`` once per iteration suits large ones.  Everything but :meth:`check` is free of synchronisation
    and can be captured in a graph: the counter lives on the device and advances inside the capture, the launches allocate
    nothing, and after the first call per pool size only the weights' ``capacity``-element temporaries come from torch's
    caching allocator."""

    def __init__(self, snapshots, num_envs, seed, first_game=0, power=2.0, prior_games=8.0):
        from . import pool

        if not isinstance(snapshots, pool.Snapshots):
            raise ValueError(f"snapshots must be a pool.Snapshots, got {type(snapshots).__name__}")
        if not _is_int(num_envs) or not 1 <= num_envs <= MAX_GAMES:
            raise ValueError(f"num_envs must be an integer in 1..2^30, got {num_envs!r}")
        if not _is_int(seed):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        if not _is_int(first_game) or not 0 <= first_game < 1 << 62:
            raise ValueError(f"first_game must be an integer in [0, 2^62), got {first_game!r}")
        if isinstance(power, bool) or not isinstance(power, (int, float)) or not power >= 0:
            raise ValueError(f"power must be a number >= 0, got {power!r}")
        if isinstance(prior_games, bool) or not isinstance(prior_games, (int, float)) or not prior_games > 0:
            raise ValueError(f"prior_games must be a number > 0, got {prior_games!r}")
        self.snapshots, self.num_envs, self.seed, self.first_game = snapshots, num_envs, seed, first_game
        self.power, self.prior_games = power, prior_games
        dev = snapshots.model.parameter_tensors()[0].device
        P = snapshots.capacity
        self.table = torch.zeros((P, P, CELL_WORDS), dtype=torch.int64, device=dev)
        self.members = torch.zeros(num_envs, dtype=torch.int64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.tally_errors = torch.zeros(1, dtype=torch.int64, device=dev)
        self.draw_errors = torch.zeros(1, dtype=torch.int32, device=dev)
        self.plans = {}

    def record(self, terminations, scores):
        """:func:`tally` of one step into ``table`` with ``player_1`` on member 0: call it right after ``env.step``"""
        return tally(terminations, scores, self.members, self.snapshots.capacity, table=self.table, errors=self.tally_errors)

    def weights(self):
        """the PFSP weights of the members the pool serves now (zero beyond ``len(snapshots)``)"""
        return pfsp_weights(self.table, len(self.snapshots), self.power, self.prior_games)

    def rematch(self, mask=None):
        """Draw a new opponent for every game (``mask``: for the games with ``mask[g] != 0`` only, e.g. the step's
        terminations) by PFSP over the current pool, group the games by member and advance the counter.  Returns the
        ``pool.Plan`` for ``player_2`` of ``snapshots.act``: one object per pool size, overwritten in place."""
        from . import pool

        P = len(self.snapshots)
        draw(self.weights(), self.num_envs, self.seed, counter=self.counter, first_game=self.first_game, mask=mask, out=self.members,
             errors=self.draw_errors)
        self.counter += 1
        plan = self.plans[P] = pool.plan(self.members, P, out=self.plans.get(P))
        return plan

    def push(self):
        """``snapshots.push()``, then the table's row and column of that slot are zeroed: the member that the ring overwrote
        does not bequeath its results.  Returns the member index."""
        slot = self.snapshots.push()
        self.table[slot].zero_()
        self.table[:, slot].zero_()
        return slot

    def win_rates(self):
        """float64 ``[capacity]`` on the device: the learner's share of won games against each member (NaN without a game)"""
        return self.table[0, :, 1].to(torch.float64) / self.table[0, :, 0].to(torch.float64)

    def check(self):
        """Read both errors words -- the one synchronisation of this class -- and raise ``ValueError`` if a finished game
        named a member outside the table or a draw met unusable weights."""
        bad, unusable = int(self.tally_errors.item()), int(self.draw_errors.item())
        if bad:
            raise ValueError(f"{bad} finished games named a member outside [0, {self.snapshots.capacity})")
        if unusable:
            raise ValueError("a draw met weights outside [0, 2^32) or of sum 0: it wrote no member")
        return self
