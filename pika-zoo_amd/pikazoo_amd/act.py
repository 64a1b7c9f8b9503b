"""A rollout step's policy side in ONE launch: from ``env.step()``'s observation rows straight to the action, its
log-probability, the entropy and the value -- ``net.forward`` and ``policy.sample`` without the ``[N, A + 1]`` head's round
trip through memory and without the second launch.

    from pikazoo_amd import net
    model = net.ActorCritic(in_features=35, hidden=64, num_actions=18).to("cuda")
    out = model.act_sample(obs, seed=7, step=t)                   # or act.sample(obs, params, 18, seed=7, step=t)
    env.step(out["actions"])                                      # int64 (or int32) actions, read as they are
    out["log_probs"]["player_1"], out["entropy"]["player_1"], out["values"]["player_1"]      # float32 [N]

It returns exactly the bits of the two launches it replaces and draws from the same Philox stream, so a trainer can switch
between the routes in the middle of a run.  WHICH ROUTE TO USE (``tools/time_act.py``, ``profiles/act.log``, 35-64-64-19, both
agents, against ``model.act`` + ``policy.sample``): this launch saves 2.6 us per step at 4 096 rows per agent, 4.1-5.5 us at
65 536 and 1.2-3.7 us at 131 072; at 262 144 rows it is 0.9-3.0 % SLOWER on normalised observations (1.5 % faster on raw int32)
and at 524 288 rows 3.7-5.7 % slower (level on raw int32).  With ``head=True`` it saves 0.5-2.0 us at 65 536 rows and is SLOWER
from 131 072 (2.3-5.7 %; 4.0-8.8 % at 262 144; 5.8-11.1 % at 524 288).  So use it up to 131 072 rows per agent (65 536 with
the head) and the two launches from 262 144 (131 072 with the head); the crossover between those sizes is not measured.

ctypes binding of libpikazoo_act.so (C ABI and the definition, by reference to the two launches: include/pikazoo_act.h), a
library of its own beside the product library; nothing in the step path, ``net`` or ``policy`` imports this module
(``ActorCritic.act_sample`` does, on first use).  There is no torch fallback: a missing or stale library raises.  The
argument checks are ``net``'s and ``policy``'s own; the launch plumbing is ``_launch``'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _launch, _native, net, policy

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_act.so"
ABI_VERSION = 1
OBS_FORMATS, ACTIVATIONS, ACTION_FORMATS = net.OBS_FORMATS, net.ACTIVATIONS, policy.ACTION_FORMATS
MAX_ACTIONS = 32

_P = C.c_void_p
SIGNATURES = {
    "pz_act_abi_version": (C.c_int, []),
    "pz_act_build_id": (C.c_char_p, []),
    # (obs_p1, obs_p2, obs_format, n, in_features, obs_pitch, hidden, out_features, activation, w1_p1, b1_p1, w2_p1, b2_p1, w3_p1,
    #  b3_p1, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2, num_actions, seed, first_game, step, step_dev, action_format, act_p1, act_p2,
    #  logp_p1, logp_p2, ent_p1, ent_p2, val_p1, val_p2, head_p1, head_p2, head_pitch, stream)
    "pz_mlp_act": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                             _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_uint64, C.c_int64, C.c_uint64, _P, C.c_int32, _P, _P,
                             _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch, a game id or a step beyond the kernel's range", -3: "an unknown format or activation"}
_lib = None


def load():
    """Load libpikazoo_act.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_act.hip", SIGNATURES, "pz_act_abi_version", ABI_VERSION)
    return _lib


def sample(obs, params, num_actions: int, seed: int, step=0, first_game: int = 0, activation: str = "tanh", action_dtype=torch.int64,
           head: bool = False, out: Optional[dict] = None):
    """The policy net's forward and one sampled action per game with its log-probability, the entropy and the value, for
    one or both agents, in one launch (``pz_mlp_act``).

    ``obs``, ``params`` and ``activation`` as in :func:`net.forward` (shared weights: one sequence with a two-agent
    ``obs``); the net's ``O`` outputs are ``num_actions`` logits (``2 <= num_actions <= 32``, ``num_actions <= O <= 40``)
    and, where ``O > num_actions``, the value in column ``num_actions``.  ``seed``, ``step`` (an int, or a 1-element int64 /
    uint64 device tensor that the launch reads), ``first_game`` and ``action_dtype`` as in :func:`policy.sample`: the draw
    of game ``g`` is the one ``policy.sample`` makes from the head of ``net.forward``, bit for bit, and so are the
    log-probability and the entropy.

    Returns ``{"actions", "log_probs", "entropy", "values"}`` -- ``action_dtype`` and float32 ``[N]``, dicts when ``obs`` is
    a dict; ``"values"`` is absent when ``O == num_actions`` -- plus ``"head"`` (float32 ``[N, O]``, what ``net.forward``
    returns) with ``head=True``; the other outputs do not depend on it.  ``out=`` a previous result makes the call
    allocation-free (it must hold ``"head"`` exactly when ``head`` is asked for); an output must not overlap an input or
    another output.  The launch goes to the current stream without a synchronisation.  Shape, dtype, device and range
    errors raise ``ValueError`` before any launch."""
    keys, xs, n, K, dev, obs_pitch = net._observations(obs, activation)
    sets = net._parameter_sets(params, keys, len(xs))
    H, O, _ = net._box(sets, K, dev)
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
    names = ["actions", "log_probs", "entropy"] + (["values"] if O > A else []) + (["head"] if head else [])
    hs, head_pitch = None, O
    if out is not None:
        if not isinstance(out, dict) or sorted(out) != sorted(names):
            raise ValueError(f"out must be a previous result with the keys {names}, got {sorted(out) if isinstance(out, dict) else type(out).__name__}")
        vec = {name: policy._vectors(out[name], f"out[{name!r}]", keys, n, (action_dtype if name == "actions" else torch.float32,), dev)
               for name in names if name != "head"}
        if head:
            hkeys, hs = _launch.sides(out["head"], "out['head']")
            if hkeys != keys:
                raise ValueError(f"out['head'] must name the agents of obs in their order: {keys}, got {hkeys}")
            head_pitch = net._rows(hs, "out['head']", n, O, (torch.float32,), dev)
    if dev.type != "cuda":
        raise ValueError(f"the policy net runs on the GPU: obs are on {dev}")
    if out is None:
        vec = {name: [torch.empty(n, dtype=action_dtype if name == "actions" else torch.float32, device=dev) for _ in xs]
               for name in names if name != "head"}
        out = {name: _launch.shape(keys, ts) for name, ts in vec.items()}
        if head:
            hs = [torch.empty((n, O), dtype=torch.float32, device=dev) for _ in xs]
            out["head"] = _launch.shape(keys, hs)
    outputs = [(f"out[{name!r}][{s}]", t) for name, ts in vec.items() for s, t in enumerate(ts)]
    outputs += [(f"out['head'][{s}]", t) for s, t in enumerate(hs or [])]
    inputs = [(f"obs[{s}]", x) for s, x in enumerate(xs)] + [(f"{name}[{s}]", p) for s, ps in enumerate(sets) for name, p in zip(net.NAMES, ps)]
    if step_dev is not None:
        inputs.append(("step", step_dev))
    _launch.no_alias(outputs, inputs)
    if n == 0:
        return out
    none = (None, None)
    second = [p.data_ptr() for p in sets[1]] if len(xs) == 2 else [None] * 6
    _launch.launch(load().pz_mlp_act, _ERRORS, dev, *_launch.ptrs(xs), OBS_FORMATS[xs[0].dtype], n, K, obs_pitch, H, O, ACTIVATIONS[activation],
                   *[p.data_ptr() for p in sets[0]], *second, A, seed, first_game, step,
                   step_dev.data_ptr() if step_dev is not None else None, ACTION_FORMATS[action_dtype], *_launch.ptrs(vec["actions"]),
                   *_launch.ptrs(vec["log_probs"]), *_launch.ptrs(vec["entropy"]), *(_launch.ptrs(vec["values"]) if O > A else none),
                   *(_launch.ptrs(hs) if head else none), head_pitch)
    return out
