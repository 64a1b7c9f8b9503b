"""A league rollout step's policy side in ONE launch: from ``env.step()``'s observation rows straight to the action, its
log-probability, the entropy and the value, every row through the net of its own pool member -- ``pool.forward`` and
``policy.sample`` without the ``[N, A + 1]`` head's round trip through memory and without the second launch.

    from pikazoo_amd import net, pool
    league = pool.Snapshots(net.ActorCritic().to("cuda"), capacity=8)
    plan = pool.plan(members, len(league))
    out = league.act_sample(obs, {"player_1": None, "player_2": plan}, seed=7, step=t, stats={"player_1"})
    env.step(out["actions"])                                      # both agents' int64 (or int32) actions, read as they are
    out["log_probs"]["player_1"], out["entropy"]["player_1"], out["values"]["player_1"]      # float32 [N]: the learner's only

It returns exactly the bits of the two launches it replaces and draws from the same Philox stream, so a trainer can switch
between the routes in the middle of a run.  ``stats=`` names the agents whose log-probabilities, entropies and values are
wanted: a league's update reads the learner's only, and the frozen opponents' side then skips the log-prob and stores nothing
but its actions.  WHICH ROUTE TO USE (``tools/time_pool_act.py``, ``profiles/pool_act.log``, 35-64-64-19, ``player_1`` unplanned
beside a planned ``player_2``, 1 / 4 / 16 members, against ``Snapshots.act`` + ``policy.sample``): this launch saves 2.0-2.3 us
per step at 4 096 rows per agent and 1.0-4.3 us at 65 536 (most with one member); at 524 288 rows it is 2.4-5.4 % SLOWER.  With
``head=`` it saves 0.9-1.2 us at 4 096 rows, is level at 65 536 with one member and SLOWER there with 4 or 16 (5.3-8.0 %), and
8-12 % slower at 524 288.  So use it without the head up to 65 536 rows per agent and the two launches at 524 288; the
crossover between those sizes is not measured.  The two launches stay the default of ``examples/ppo_league.py``;
``--fused-act`` takes this one.

ctypes binding of libpikazoo_pool_act.so (C ABI and the definition, by reference to the two launches:
include/pikazoo_pool_act.h), a library of its own beside the product library; nothing in the step path, ``pool``, ``league``,
``act`` or ``net`` imports this module (``Snapshots.act_sample`` does, on first use).  There is no torch fallback: a missing or
stale library raises.  The argument checks are ``net``'s, ``policy``'s and ``pool``'s own; the launch plumbing is ``_launch``'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _launch, _native, net, policy, pool

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_pool_act.so"
ABI_VERSION = 1
OBS_FORMATS, ACTIVATIONS, ACTION_FORMATS = net.OBS_FORMATS, net.ACTIVATIONS, policy.ACTION_FORMATS
MAX_ACTIONS = 32
MAX_MEMBERS = pool.MAX_MEMBERS
Member = pool.Member
STATS = ("log_probs", "entropy", "values")

_P = C.c_void_p
SIGNATURES = {
    "pz_pool_act_abi_version": (C.c_int, []),
    "pz_pool_act_build_id": (C.c_char_p, []),
    # (obs_p1, obs_p2, obs_format, n, in_features, obs_pitch, hidden, out_features, activation, members, num_members, order_p1,
    #  first_p1, order_p2, first_p2, num_actions, seed, first_game, step, step_dev, action_format, act_p1, act_p2, logp_p1, logp_p2,
    #  ent_p1, ent_p2, val_p1, val_p2, head_p1, head_p2, head_pitch, stream)
    "pz_mlp_act_pool": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Member),
                                  C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_uint64, C.c_int64, C.c_uint64, _P, C.c_int32, _P, _P, _P, _P,
                                  _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch, the number of members, a game id or a step beyond the kernel's range",
           -3: "an unknown format or activation"}
_lib = None


def load():
    """Load libpikazoo_pool_act.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_pool_act.hip", SIGNATURES, "pz_pool_act_abi_version", ABI_VERSION)
    return _lib


def _agents(which, what, keys, sides, everyone):
    """per agent whether it is in `which`: None (`everyone`), a bool, or a collection of agent names of a dict ``obs``"""
    if which is None:
        return [everyone] * sides
    if isinstance(which, bool):
        return [which] * sides
    if isinstance(which, (str, torch.Tensor, dict)) or not hasattr(which, "__iter__"):
        raise ValueError(f"{what} must be None, a bool or a collection of agent names, got {type(which).__name__}")
    names = list(which)
    if keys is None:
        raise ValueError(f"{what} names agents, but obs is a tensor: pass None or a bool")
    for name in names:
        if name not in keys:
            raise ValueError(f"{what} names {name!r}, which is no agent of obs: {keys}")
    return [k in names for k in keys]


def sample(obs, member_params, plans, num_actions: int, seed: int, step=0, first_game: int = 0, activation: str = "tanh",
           action_dtype=torch.int64, stats=None, head=False, out: Optional[dict] = None):
    """``pool.forward`` and one sampled action per game with its log-probability, the entropy and the value, for one or both
    agents, every row under its own pool member, in one launch (``pz_mlp_act_pool``).

    ``obs``, ``member_params``, ``plans`` and ``activation`` as in :func:`pool.forward`; the net's ``O`` outputs are
    ``num_actions`` logits (``2 <= num_actions <= 32``, ``num_actions <= O <= 40``) and, where ``O > num_actions``, the value in
    column ``num_actions``.  ``seed``, ``step`` (an int, or a 1-element int64 / uint64 device tensor that the launch reads),
    ``first_game`` and ``action_dtype`` as in :func:`act.sample`: the draw of game ``g`` is the one ``policy.sample`` makes
    from the head of ``pool.forward``, bit for bit, and so are the log-probability and the entropy.  Rows that a plan counted
    as errors are not written, in any output.

    ``stats``: the agents that get ``log_probs``, ``entropy`` and ``values`` -- ``None`` (all of them), a bool, or a collection
    of agent names of a dict ``obs``.  An agent outside it gets its actions only, the same bits.  ``head``: ``False``, ``True``
    or a collection of agent names: those agents also get the float32 ``[N, O]`` head that ``pool.forward`` returns.

    Returns ``{"actions", "log_probs", "entropy", "values"[, "head"]}``: ``action_dtype`` and float32 ``[N]``; with a dict
    ``obs`` each is a dict over the agents that have it, and a name that no agent has is absent (as is ``"values"`` when
    ``O == num_actions``).  ``out=`` a previous result of the same arguments makes the call allocation-free; an output must not
    overlap an input or another output.  The launch goes to the current stream without a synchronisation and can be captured.
    Shape, dtype, device and range errors raise ``ValueError`` before any launch."""
    keys, xs, n, K, dev, obs_pitch = net._observations(obs, activation)
    sets = pool._member_sets(member_params)
    H, O, _ = net._box(sets, K, dev, "member {}: ")
    per = pool._agent_plans(plans, keys, len(xs), n, len(sets), dev)
    A = int(num_actions)
    if not 2 <= A <= MAX_ACTIONS:
        raise ValueError(f"2 <= num_actions <= {MAX_ACTIONS}, got {A}")
    if O < A:
        raise ValueError(f"the net has {O} outputs: fewer than num_actions = {A}")
    seed, first_game = int(seed), int(first_game)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    if not 0 <= first_game < 1 << 62:
        raise ValueError(f"first_game must lie in [0, 2^62), got {first_game}")
    step_dev = None
    if isinstance(step, torch.Tensor):
        if step.numel() != 1 or step.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or step.device != dev:
            raise ValueError(f"a step tensor holds one int64 or uint64 on {dev}, got {step.dtype} {list(step.shape)} on {step.device}")
        step_dev, step = step, 0
    else:
        step = int(step)
        if not 0 <= step < 1 << 62:
            raise ValueError(f"step must lie in [0, 2^62), got {step}")
    if action_dtype not in ACTION_FORMATS:
        raise ValueError(f"action_dtype must be {' or '.join(str(d) for d in ACTION_FORMATS)}, got {action_dtype}")
    sides = len(xs)
    with_stats = _agents(stats, "stats", keys, sides, True)
    with_head = _agents(head, "head", keys, sides, False)
    # which agents hold which name, in the order of the result
    has = {"actions": [True] * sides}
    for name in STATS:
        has[name] = with_stats if name != "values" or O > A else [False] * sides
    has["head"] = with_head
    names = [name for name, on in has.items() if any(on)]
    agents_of = lambda name: [s for s in range(sides) if has[name][s]]  # noqa: E731
    sub = lambda name: None if keys is None else [keys[s] for s in agents_of(name)]  # noqa: E731
    dtype_of = lambda name: action_dtype if name == "actions" else torch.float32  # noqa: E731
    head_pitch = O
    if out is not None:
        if not isinstance(out, dict) or sorted(out) != sorted(names):
            raise ValueError(f"out must be a previous result with the keys {names}, got {sorted(out) if isinstance(out, dict) else type(out).__name__}")
        held = {}
        for name in names:
            if (keys is None) == isinstance(out[name], dict) or (keys is not None and list(out[name]) != sub(name)):
                raise ValueError(f"out[{name!r}] must be {'a tensor' if keys is None else f'a dict over {sub(name)}'}, got "
                                 f"{list(out[name]) if isinstance(out[name], dict) else type(out[name]).__name__}")
            if name == "head":
                _, held[name] = _launch.sides(out[name], "out['head']")
                head_pitch = net._rows(held[name], "out['head']", n, O, (torch.float32,), dev)
            else:
                held[name] = policy._vectors(out[name], f"out[{name!r}]", sub(name), n, (dtype_of(name),), dev)
    if dev.type != "cuda":
        raise ValueError(f"the policy net runs on the GPU: obs are on {dev}")
    if out is None:
        held = {name: [torch.empty((n, O) if name == "head" else n, dtype=dtype_of(name), device=dev) for _ in agents_of(name)] for name in names}
        out = {name: _launch.shape(sub(name), ts) for name, ts in held.items()}
    outputs = [(f"out[{name!r}][{s}]", t) for name, ts in held.items() for s, t in zip(agents_of(name), ts)]
    inputs = [(f"obs[{s}]", x) for s, x in enumerate(xs)] + [(f"member {m} {name}", p) for m, ps in enumerate(sets) for name, p in zip(net.NAMES, ps)]
    inputs += [(f"plans[{s}].{name}", t) for s, p in enumerate(per) if p is not None for name, t in (("order", p.order), ("first", p.first))]
    if step_dev is not None:
        inputs.append(("step", step_dev))
    _launch.no_alias(outputs, inputs)
    if n == 0:
        return out
    array = (Member * MAX_MEMBERS)()
    for m, ps in enumerate(sets):
        array[m] = Member(*[p.data_ptr() for p in ps])
    plan_ptrs = []
    for s in range(2):
        p = per[s] if s < len(per) else None
        plan_ptrs += [p.order.data_ptr(), p.first.data_ptr()] if p is not None else [None, None]

    def pair(name):
        at = dict(zip(agents_of(name), held.get(name, [])))
        return [at[s].data_ptr() if s in at else None for s in (0, 1)]

    _launch.launch(load().pz_mlp_act_pool, _ERRORS, dev, *_launch.ptrs(xs), OBS_FORMATS[xs[0].dtype], n, K, obs_pitch, H, O,
                   ACTIVATIONS[activation], array, len(sets), *plan_ptrs, A, seed, first_game, step,
                   step_dev.data_ptr() if step_dev is not None else None, ACTION_FORMATS[action_dtype], *pair("actions"), *pair("log_probs"),
                   *pair("entropy"), *pair("values"), *pair("head"), head_pitch)
    return out
