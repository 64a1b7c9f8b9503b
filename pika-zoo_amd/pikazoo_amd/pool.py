"""Self-play against a pool of snapshots at rollout speed: the policy net's forward in ONE launch in which every row runs
through the parameter set of its own pool member.

    from pikazoo_amd import net, pool
    model = net.ActorCritic().to("cuda")
    league = pool.Snapshots(model, capacity=8)                  # member 0 is the live model, 1.. are frozen copies
    league.push()                                               # (every few iterations)
    members = torch.randint(len(league), (n,), device="cuda")   # each game draws its opponent
    plan = pool.plan(members, len(league))                      # rows grouped by member: once per re-assignment
    head = league.act(obs, {"player_1": None, "player_2": plan})    # one launch per policy step, both agents
    out = league.act_sample(obs, {"player_1": None, "player_2": plan}, seed=7, step=t, stats={"player_1"})   # ... with the draw

    pool.forward(obs, member_params, plans)                     # the same launch on any P parameter sets

ctypes binding of libpikazoo_pool.so (C ABI and the definition: include/pikazoo_pool.h), a library of its own beside the
product library; nothing in the step path or in the other modules imports this one (``league`` does, on first use).  There is no torch fallback: a missing or
stale library raises.  A row's result holds exactly the bits ``net.forward`` gives it with its member's parameters.  The
parameters are read in place from up to 16 sets of ``nn.Linear`` tensors, so an optimizer step on member 0 is seen by the
next launch, and by the next replay of a captured graph.  The arguments are checked by ``net``'s own check, a member's name in
front of its tensor's; the launch plumbing is ``_launch``'s.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _launch, _native, net

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_pool.so"
ABI_VERSION = 1
MAX_MEMBERS = 16
GROUP_ROWS = 128
MAX_ROWS = 1 << 30
MEMBER_FORMATS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}

_P = C.c_void_p


class Member(C.Structure):
    """pz_pool_member"""
    _fields_ = [("w1", _P), ("b1", _P), ("w2", _P), ("b2", _P), ("w3", _P), ("b3", _P)]


SIGNATURES = {
    "pz_pool_abi_version": (C.c_int, []),
    "pz_pool_build_id": (C.c_char_p, []),
    # (n, num_members)
    "pz_pool_capacity": (C.c_int64, [C.c_int64, C.c_int32]),
    # (members, member_format, n, num_members, order, first, errors, stream)
    "pz_pool_plan": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    # (obs_p1, obs_p2, obs_format, n, in_features, obs_pitch, hidden, out_features, activation, members, num_members, order_p1,
    #  first_p1, order_p2, first_p2, out_p1, out_p2, out_format, out_pitch, stream)
    "pz_mlp_forward_pool": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Member),
                                      C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch or the number of members beyond the kernel's range", -3: "an unknown format or activation"}
_lib = None


def load():
    """Load libpikazoo_pool.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_pool.hip", SIGNATURES, "pz_pool_abi_version", ABI_VERSION)
    return _lib


def capacity(n: int, num_members: int) -> int:
    """the int32 words of a plan's ``order``: ``(n // 128 + num_members) * 128`` (include/pikazoo_pool.h proves the bound)"""
    return (n // GROUP_ROWS + num_members) * GROUP_ROWS


# ---- the plan ------------------------------------------------------------------------------------------------------------------
class Plan:
    """The rows of one agent grouped by pool member (``pz_pool_plan``): ``order`` int32 ``[capacity(n, num_members)]``, ``first``
    int32 ``[num_members + 1]``, ``errors`` int32 ``[1]`` (the number of rows whose member is outside ``[0, num_members)``: they
    are in no group, and the forward neither reads nor writes them), and the ``n`` and ``num_members`` it was made for."""

    def __init__(self, order, first, errors, n, num_members):
        self.order, self.first, self.errors, self.n, self.num_members = order, first, errors, n, num_members

    def check(self):
        """Read ``errors`` -- the one synchronisation of this module -- and raise ``ValueError`` if rows had no valid member."""
        bad = int(self.errors.item())
        if bad:
            raise ValueError(f"{bad} of {self.n} rows name a member outside [0, {self.num_members})")
        return self


def plan(members, num_members, out=None) -> Plan:
    """Group the rows of one agent by pool member, in one launch (``pz_pool_plan``): a stable counting sort on the device.

    ``members``: ``[n]`` uint8, int32 or int64, contiguous, on the GPU: the pool member each row plays, ``0 <= members[i] <
    num_members <= 16``.  A row with another value is left out of every group and counted in ``Plan.errors``
    (:meth:`Plan.check` reads it).  ``out=`` a previous :class:`Plan` of the same ``n`` and ``num_members`` makes the call
    allocation-free: it is overwritten and returned, which is how opponents are re-drawn between replays of a captured graph.
    No synchronisation.  Shape, dtype, device and range errors raise ``ValueError`` before any launch."""
    if not isinstance(members, torch.Tensor):
        raise ValueError(f"members must be a tensor, got {type(members).__name__}")
    if members.dim() != 1 or not members.is_contiguous():
        raise ValueError(f"members must be a contiguous one-dimensional tensor, got shape {list(members.shape)}, strides {list(members.stride())}")
    if members.dtype not in MEMBER_FORMATS:
        raise ValueError(f"members must be {' or '.join(str(d) for d in MEMBER_FORMATS)}, got {members.dtype}")
    if isinstance(num_members, bool) or not isinstance(num_members, int) or not 1 <= num_members <= MAX_MEMBERS:
        raise ValueError(f"num_members must be an integer in 1..{MAX_MEMBERS}, got {num_members!r}")
    n, dev = int(members.shape[0]), members.device
    if n > MAX_ROWS:
        raise ValueError(f"members: at most 2^30 rows, got {n}")
    cap = capacity(n, num_members)
    if out is not None:
        if not isinstance(out, Plan):
            raise ValueError(f"out must be a previous Plan, got {type(out).__name__}")
        if out.n != n or out.num_members != num_members:
            raise ValueError(f"out is a plan of {out.n} rows and {out.num_members} members, not of {n} and {num_members}")
        for name, t, size in (("order", out.order, cap), ("first", out.first, num_members + 1), ("errors", out.errors, 1)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (size,) or not t.is_contiguous()
                    or t.device != dev):
                raise ValueError(f"out.{name} must be a contiguous int32 [{size}] tensor on {dev}")
        _launch.no_alias([("out.order", out.order), ("out.first", out.first), ("out.errors", out.errors)], [("members", members)])
    if dev.type != "cuda":
        raise ValueError(f"the plan is built on the GPU: members are on {dev}")
    if out is None:
        out = Plan(torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(num_members + 1, dtype=torch.int32, device=dev),
                   torch.empty(1, dtype=torch.int32, device=dev), n, num_members)
    _launch.launch(load().pz_pool_plan, _ERRORS, dev, members.data_ptr() if n else None, MEMBER_FORMATS[members.dtype], n, num_members,
                   out.order.data_ptr(), out.first.data_ptr(), out.errors.data_ptr())
    return out


# ---- the forward ---------------------------------------------------------------------------------------------------------------
def _member_sets(member_params):
    if isinstance(member_params, (torch.Tensor, dict)) or not hasattr(member_params, "__len__"):
        raise ValueError(f"member_params must be a sequence of parameter sets, got {type(member_params).__name__}")
    if not 1 <= len(member_params) <= MAX_MEMBERS:
        raise ValueError(f"a pool holds 1..{MAX_MEMBERS} members, got {len(member_params)}")
    sets = []
    for m, ps in enumerate(member_params):
        if isinstance(ps, torch.Tensor) or not hasattr(ps, "__len__") or len(ps) != 6:
            raise ValueError(f"member_params[{m}] must be a sequence of six tensors (W1, b1, W2, b2, W3, b3)")
        for p in ps:
            if not isinstance(p, torch.Tensor):
                raise ValueError(f"member_params[{m}]: a parameter must be a tensor, got {type(p).__name__}")
        sets.append([p.data for p in ps])
    return sets


def _agent_plans(plans, keys, sides, n, P, dev):
    if isinstance(plans, dict):
        if keys is None or list(plans) != keys:
            raise ValueError(f"plans must name the agents of obs in their order: {keys}, got {list(plans)}")
        per = list(plans.values())
    elif keys is not None:
        raise ValueError(f"plans must be an {{agent: Plan or None}} dict over {keys}: obs is a dict")
    else:
        per = [plans]
    for s, p in enumerate(per):
        if p is None:
            continue
        if not isinstance(p, Plan):
            raise ValueError(f"a plan must be a Plan or None, got {type(p).__name__}")
        if p.n != n or p.num_members != P:
            raise ValueError(f"plans[{s}] was made for {p.n} rows and {p.num_members} members; obs has {n} rows and the pool {P} members")
        for name, t, size in (("order", p.order, capacity(n, P)), ("first", p.first, P + 1)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (size,) or not t.is_contiguous()
                    or t.device != dev):
                raise ValueError(f"plans[{s}].{name} must be a contiguous int32 [{size}] tensor on {dev}")
    return per


def forward(obs, member_params, plans, activation: str = "tanh", out=None, out_dtype=torch.float32):
    """``net.forward`` for a pool: every observation row of one or both agents through the parameter set of its own pool
    member, in one launch (``pz_mlp_forward_pool``).  A row's result holds exactly the bits ``net.forward`` gives it with
    its member's parameters.

    ``obs``, ``activation``, ``out`` and ``out_dtype`` are :func:`pikazoo_amd.net.forward`'s, with its rules and errors.
    ``member_params``: a sequence of ``P <= 16`` sequences ``(W1, b1, W2, b2, W3, b3)`` of one shape, float32, contiguous,
    on the obs' device, read in place; both agents share the pool, and two members may be the same tensors.  ``plans``: a
    :class:`Plan` or ``None`` for a tensor ``obs``, an ``{agent: Plan | None}`` dict over the agents of a dict ``obs``;
    ``None`` runs every row of that agent on member 0.  A plan must have been made for the ``n`` of ``obs`` and for ``P``
    members.  Rows that the plan counted as errors are not written.

    The launch goes to the current stream without a synchronisation and can be captured.  Shape, dtype, device and range
    errors raise ``ValueError`` before any launch."""
    keys, xs, n, K, dev, obs_pitch = net._observations(obs, activation)
    sets = _member_sets(member_params)
    H, O, _ = net._box(sets, K, dev, "member {}: ")
    per = _agent_plans(plans, keys, len(xs), n, len(sets), dev)
    ys, out_pitch = net._outputs(out, out_dtype, keys, n, O, dev)
    if dev.type != "cuda":
        raise ValueError(f"the policy net runs on the GPU: obs are on {dev}")
    if ys is None:
        ys = [torch.empty((n, O), dtype=out_dtype, device=dev) for _ in xs]
        out = _launch.shape(keys, ys)
    _launch.no_alias([(f"out[{s}]", y) for s, y in enumerate(ys)],
                     [(f"obs[{s}]", x) for s, x in enumerate(xs)] + [(f"member {m} {name}", p) for m, ps in enumerate(sets) for name, p in zip(net.NAMES, ps)]
                     + [(f"plans[{s}].{name}", t) for s, p in enumerate(per) if p is not None for name, t in (("order", p.order), ("first", p.first))])
    if n == 0:
        return out
    array = (Member * MAX_MEMBERS)()
    for m, ps in enumerate(sets):
        array[m] = Member(*[p.data_ptr() for p in ps])
    plan_ptrs = []
    for s in range(2):
        p = per[s] if s < len(per) else None
        plan_ptrs += [p.order.data_ptr(), p.first.data_ptr()] if p is not None else [None, None]
    _launch.launch(load().pz_mlp_forward_pool, _ERRORS, dev, *_launch.ptrs(xs), net.OBS_FORMATS[xs[0].dtype], n, K, obs_pitch, H, O,
                   net.ACTIVATIONS[activation], array, len(sets), *plan_ptrs, *_launch.ptrs(ys), net.OUT_FORMATS[ys[0].dtype], out_pitch)
    return out


# ---- the snapshots -------------------------------------------------------------------------------------------------------------
class Snapshots:
    """A pool around a live ``net.ActorCritic``: member 0 is the module's own parameter tensors, members ``1 .. capacity - 1`` are
    frozen copies that this object owns, filled by :meth:`push` in a ring (the oldest copy is overwritten once all are full).

    The copies are allocated once, so a member's tensors never move: a captured :meth:`act` stays valid across pushes and
    optimizer steps, and sees both.  ``len()`` is the number of members that :meth:`act` serves now: 1 plus the filled slots."""

    def __init__(self, model, capacity: int):
        if not isinstance(model, net.ActorCritic):
            raise ValueError(f"model must be a net.ActorCritic, got {type(model).__name__}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= MAX_MEMBERS:
            raise ValueError(f"capacity must be an integer in 1..{MAX_MEMBERS}, got {capacity!r}")
        self.model, self.capacity = model, capacity
        self.slots = [[torch.empty_like(p.data) for p in model.parameter_tensors()] for _ in range(capacity - 1)]
        self.filled, self.pushes = 0, 0

    def __len__(self):
        return 1 + self.filled

    def push(self):
        """Copy the live parameters into the next slot of the ring (six ``copy_``: not hot).  Returns the member index that
        now holds them."""
        if not self.slots:
            raise ValueError("a pool of capacity 1 holds the live model only: there is no slot to push into")
        slot = self.pushes % len(self.slots)
        with torch.no_grad():
            for dst, src in zip(self.slots[slot], self.model.parameter_tensors()):
                dst.copy_(src.data)
        self.pushes += 1
        self.filled = min(self.filled + 1, len(self.slots))
        return 1 + slot

    def member_params(self):
        """the live module's own tensors as member 0, then the filled slots: what :func:`forward` takes"""
        return [self.model.parameter_tensors()] + self.slots[:self.filled]

    def act(self, obs, plans, out=None, out_dtype=torch.float32):
        """the ``[N, num_actions + 1]`` head of every row under its own member, in one launch: :func:`forward` on
        :meth:`member_params` (plans are made for ``len(self)`` members)"""
        with torch.no_grad():
            return forward(obs, self.member_params(), plans, self.model.activation, out=out, out_dtype=out_dtype)

    def act_sample(self, obs, plans, seed: int, step=0, first_game: int = 0, stats=None, head=False, out=None):
        """:meth:`act` and ``policy.sample`` on its logits in ONE launch (``pool_act.sample``, imported on first use: nothing
        loads libpikazoo_pool_act.so before): ``{"actions", "log_probs", "entropy", "values"}``, every row under its own
        member, the bits of the two calls from the same Philox stream.  ``stats``: the agents whose log-probabilities,
        entropies and values are wanted (``None``: all; a league passes the learner alone); ``head``: those that also get the
        ``[N, num_actions + 1]`` head"""
        from . import pool_act

        with torch.no_grad():
            return pool_act.sample(obs, self.member_params(), plans, self.model.num_actions, seed, step=step, first_game=first_game,
                                   activation=self.model.activation, stats=stats, head=head, out=out)
