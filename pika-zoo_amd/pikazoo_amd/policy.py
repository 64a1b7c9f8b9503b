"""What a trainer does on every policy step, between the policy net's last ``Linear`` and ``env.step()``: the categorical
head over ``[N, A]`` logits in ONE launch.

    from pikazoo_amd import policy
    out = policy.sample({"player_1": logits_1, "player_2": logits_2}, seed=7, step=env.steps_done)   # or env.sample_actions(...)
    env.step(out["actions"])                                      # int64 (or int32) actions, read as they are
    out["log_probs"]["player_1"], out["entropy"]["player_1"]      # float32 [N]
    logp, ent = policy.log_probs(logits, actions)                 # the update side: differentiable w.r.t. the logits

ctypes binding of libpikazoo_policy.so (C ABI, the definition of the draw and the arithmetic: include/pikazoo_policy.h), a
library of its own beside the product library; nothing in the step path imports this module.  There is no torch
fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _launch, _native
from ._launch import ptrs as _ptrs, shape as _shape

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_policy.so"
ABI_VERSION = 1
LOGIT_FORMATS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACTION_FORMATS = {torch.int32: 0, torch.int64: 1}
MAX_ACTIONS = 32

_P = C.c_void_p
SIGNATURES = {
    "pz_policy_abi_version": (C.c_int, []),
    "pz_policy_build_id": (C.c_char_p, []),
    # (logits_p1, logits_p2, logit_format, num_actions, n, logit_pitch, seed, first_game, step, step_dev, action_format,
    #  act_p1, act_p2, logp_p1, logp_p2, ent_p1, ent_p2, stream)
    "pz_sample_actions": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_uint64, _P,
                                    C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    # (logits_p1, logits_p2, logit_format, num_actions, n, logit_pitch, action_format, act_p1, act_p2, logp_p1, logp_p2,
    #  ent_p1, ent_p2, stream)
    "pz_action_log_probs": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    # (the same logits and actions, glogp_p1, glogp_p2, gent_p1, gent_p2, grad_p1, grad_p2, grad_pitch, stream)
    "pz_action_log_probs_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P,
                                               _P, _P, _P, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch, a game id or a step beyond the kernel's range", -3: "an unknown format"}
_lib = None


def load():
    """Load libpikazoo_policy.so (once).  Raises, as ``learn.load()`` does, if it has not been built or was built from
    other sources than the ones in this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_policy.hip", SIGNATURES, "pz_policy_abi_version", ABI_VERSION)
    return _lib


def _check_logits(logits):
    """(keys, tensors, n, A, pitch, device) of the logits of one or two agents"""
    keys, ls = _launch.sides(logits, "logits")
    l0 = ls[0]
    if l0.dim() != 2:
        raise ValueError(f"logits must have shape [N, A], got {tuple(l0.shape)}")
    n, A = int(l0.shape[0]), int(l0.shape[1])
    if not 2 <= A <= MAX_ACTIONS:
        raise ValueError(f"logits: 2 <= A <= {MAX_ACTIONS} actions, got {A}")
    if l0.dtype not in LOGIT_FORMATS:
        raise ValueError(f"logits must be {' or '.join(str(d) for d in LOGIT_FORMATS)}, got {l0.dtype}")
    pitches = set()
    for t in ls:
        if tuple(t.shape) != (n, A) or t.dtype != l0.dtype or t.device != l0.device:
            raise ValueError(f"both agents' logits must be {l0.dtype} {[n, A]} on {l0.device}, got {t.dtype} {list(t.shape)} on {t.device}")
        if t.stride(1) != 1:
            raise ValueError(f"logits: the last dimension must be contiguous (stride {t.stride(1)})")
        if n > 1 and t.stride(0) < A:
            raise ValueError(f"logits: rows overlap (row stride {t.stride(0)} < {A})")
        pitches.add(int(t.stride(0)) if n > 1 else A)
    if len(pitches) != 1:
        raise ValueError(f"logits: both agents' tensors must have the same row stride, got {sorted(pitches)}")
    if l0.device.type != "cuda":
        raise ValueError(f"the policy head runs on the GPU: logits are on {l0.device}")
    return keys, ls, n, A, pitches.pop(), l0.device


def _vectors(x, what, keys, n, dtypes, dev):
    """the [n] tensors of `x` (in the shape of the logits: a dict with the same agents, or one tensor), contiguous"""
    xkeys, ts = _launch.sides(x, what)
    if xkeys != keys:
        raise ValueError(f"{what} must name the agents of the logits in their order: {keys}, got {xkeys}")
    for t in ts:
        if tuple(t.shape) != (n,) or t.dtype not in dtypes or t.dtype != ts[0].dtype or t.device != dev:
            raise ValueError(f"{what} must be {' or '.join(str(d) for d in dtypes)} [{n}] on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
        if n > 1 and t.stride(0) != 1:
            raise ValueError(f"{what} must be contiguous (stride {t.stride(0)})")
    return ts


def sample(logits, seed: int, step=0, first_game: int = 0, action_dtype=torch.int64, out: Optional[dict] = None):
    """Sample one action per game from ``Categorical(logits=...)`` and return it with its log-probability and the
    entropy of the distribution, for one or both agents, in one launch (``pz_sample_actions``).

    ``logits``: ``[N, A]`` float32, float16 or bfloat16, ``2 <= A <= 32`` -- a tensor, or an ``{agent: tensor}`` dict of
    one or two agents.  The last dimension is contiguous; any row stride >= A goes (a ``[:, :18]`` view of a 19-wide
    actor-critic output), and both agents share it.  A ``-inf`` logit masks its action.  The draw of game ``g`` is a
    function of ``(seed, first_game + g, step, agent position)`` alone -- a counter-based Philox stream apart from the
    env's own even under the env's seed (include/pikazoo_policy.h) -- so a rank that holds rows ``[g0, N)`` passes
    ``first_game=g0`` and draws what the whole batch would.  ``step``: an int, or a 1-element int64 / uint64 device
    tensor that the launch reads (a by-value step is frozen into a captured graph: capture ``counter.add_(1)`` with it).

    Returns ``{"actions", "log_probs", "entropy"}``: ``action_dtype`` (int64 or int32: ``env.step`` reads both as they
    are) and float32 ``[N]``, dicts when given a dict.  The launch goes to the caller's current stream without a
    synchronisation, and without an allocation when ``out`` is the previous result.  Shape, dtype, device and range
    errors raise ``ValueError`` before any launch."""
    keys, ls, n, A, pitch, dev = _check_logits(logits)
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
    if out is not None:
        act = _vectors(out.get("actions"), "out['actions']", keys, n, (action_dtype,), dev)
        logp = _vectors(out.get("log_probs"), "out['log_probs']", keys, n, (torch.float32,), dev)
        ent = _vectors(out.get("entropy"), "out['entropy']", keys, n, (torch.float32,), dev)
    else:
        act = [torch.empty(n, dtype=action_dtype, device=dev) for _ in ls]
        logp = [torch.empty(n, dtype=torch.float32, device=dev) for _ in ls]
        ent = [torch.empty(n, dtype=torch.float32, device=dev) for _ in ls]
        out = {"actions": _shape(keys, act), "log_probs": _shape(keys, logp), "entropy": _shape(keys, ent)}
    if n == 0:
        return out
    _launch.launch(load().pz_sample_actions, _ERRORS, dev, *_ptrs(ls), LOGIT_FORMATS[ls[0].dtype], A, n, pitch, seed, first_game, step,
                   step_dev.data_ptr() if step_dev is not None else None, ACTION_FORMATS[action_dtype], *_ptrs(act), *_ptrs(logp), *_ptrs(ent))
    return out


def _forward(ls, act, n, A, pitch, dev):
    logp = [torch.empty(n, dtype=torch.float32, device=dev) for _ in ls]
    ent = [torch.empty(n, dtype=torch.float32, device=dev) for _ in ls]
    if n:
        _launch.launch(load().pz_action_log_probs, _ERRORS, dev, *_ptrs(ls), LOGIT_FORMATS[ls[0].dtype], A, n, pitch,
                       ACTION_FORMATS[act[0].dtype], *_ptrs(act), *_ptrs(logp), *_ptrs(ent))
    return logp, ent


class _LogProbs(torch.autograd.Function):
    """(n, A, pitch, sides, actions..., logits...) -> (logp..., entropy...); saves the logits and the actions only"""

    @staticmethod
    def forward(ctx, n, A, pitch, sides, *tensors):
        act, ls = list(tensors[:sides]), list(tensors[sides:])
        logp, ent = _forward(ls, act, n, A, pitch, ls[0].device)
        ctx.save_for_backward(*tensors)
        ctx.geometry = (n, A, pitch, sides)
        return (*logp, *ent)

    @staticmethod
    def backward(ctx, *grads):
        n, A, pitch, sides = ctx.geometry
        act, ls = list(ctx.saved_tensors[:sides]), list(ctx.saved_tensors[sides:])
        dev = ls[0].device

        def upstream(gs):  # the pair is there for both agents or for none: an agent's missing one counts as zeros
            if all(g is None for g in gs):
                return None
            return [torch.zeros(n, dtype=torch.float32, device=dev) if g is None else g.to(torch.float32).contiguous() for g in gs]

        glogp, gent = upstream(grads[:sides]), upstream(grads[sides:])
        if glogp is None and gent is None:
            return (None,) * (4 + 2 * sides)
        grad = [torch.empty((n, A), dtype=l.dtype, device=dev) for l in ls]
        if n:
            none = (None, None)
            _launch.launch(load().pz_action_log_probs_backward, _ERRORS, dev, *_ptrs(ls), LOGIT_FORMATS[ls[0].dtype], A, n, pitch,
                           ACTION_FORMATS[act[0].dtype], *_ptrs(act), *(_ptrs(glogp) if glogp is not None else none),
                           *(_ptrs(gent) if gent is not None else none), *_ptrs(grad), A)
        return (None, None, None, None, *([None] * sides), *grad)


def log_probs(logits, actions):
    """``(log_probs, entropy)`` of given actions under ``Categorical(logits=...)``: float32 ``[N]`` each, dicts when
    given dicts -- what ``.log_prob(actions)`` and ``.entropy()`` return, in one launch (``pz_action_log_probs``), and
    differentiable with respect to the logits: the backward is one launch too (``pz_action_log_probs_backward``), which
    recomputes the probabilities from the saved logits and actions and returns the gradient in the logits' dtype.

    ``logits`` as in :func:`sample`; ``actions``: int64 or int32 ``[N]`` in the same shape (a dict with the same agents,
    or one tensor).  An action outside ``[0, A)`` gives a NaN log-probability and no ``[i == a]`` term in the gradient.
    Errors as in :func:`sample`."""
    keys, ls, n, A, pitch, dev = _check_logits(logits)
    act = _vectors(actions, "actions", keys, n, tuple(ACTION_FORMATS), dev)
    sides = len(ls)
    if torch.is_grad_enabled() and any(t.requires_grad for t in ls):
        res = _LogProbs.apply(n, A, pitch, sides, *act, *ls)
        logp, ent = list(res[:sides]), list(res[sides:])
    else:
        logp, ent = _forward(ls, act, n, A, pitch, dev)
    return _shape(keys, logp), _shape(keys, ent)
