"""What a trainer does with a minibatch between the policy net's output and ``backward()``: the PPO loss, its logging
statistics and its gradients with respect to the logits and the values from ONE pass over the logit rows.

    from pikazoo_amd import ppo
    loss, stats = ppo.loss(logits, values, actions, old_log_probs, advantages, returns)    # differentiable; then loss.backward()
    out = ppo.loss_and_grad(head=head_out, num_actions=18, actions=..., ...)                # or: head_out.backward(out["grad_head"])

ctypes binding of libpikazoo_ppo.so (C ABI and the definition: include/pikazoo_ppo.h), a library of its own beside the
product library; nothing in the step path, ``learn`` or ``policy`` imports this module.  There is no torch fallback: a
missing or stale library raises.  The reductions are deterministic (no floating-point atomics): two calls on the same
inputs return the same bits.  ``_check_logits`` and ``_vectors`` are ``policy``'s, the launch plumbing is ``_launch``'s.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _launch, _native
from ._launch import ptrs as _ptrs, shape as _shape, sides as _sides
from .policy import ACTION_FORMATS, LOGIT_FORMATS, _check_logits, _vectors

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_ppo.so"
ABI_VERSION = 1
VALUE_FORMATS = LOGIT_FORMATS
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")
ROWS_PER_PARTIAL = 64      # csrc/pz_ppo.hip: one wave's rows give one partial sum per term ...
FINISH_THREADS = 256       # ... and the finishing launch sums them with this many threads
MOMENT_ROWS = 4096         # rows per partial of pz_ppo_moments

_P = C.c_void_p
SIGNATURES = {
    "pz_ppo_abi_version": (C.c_int, []),
    "pz_ppo_build_id": (C.c_char_p, []),
    "pz_ppo_workspace_bytes": (C.c_int64, [C.c_int64]),
    # (x_p1, x_p2, n, eps, out, workspace, stream)
    "pz_ppo_moments": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P, _P, _P]),
    # (logits_p1, logits_p2, logit_format, num_actions, n, logit_pitch, action_format, act_p1, act_p2, old_logp_p1, old_logp_p2,
    #  adv_p1, adv_p2, ret_p1, ret_p2, values_p1, values_p2, value_format, value_pitch, old_values_p1, old_values_p2,
    #  old_value_format, adv_norm, clip, value_clip, vf_coef, ent_coef, grad_logits_p1, grad_logits_p2, grad_pitch,
    #  grad_values_p1, grad_values_p2, grad_value_pitch, stats, workspace, stream)
    "pz_ppo_loss": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                              C.c_int32, C.c_int64, _P, _P, C.c_int32, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P,
                              C.c_int64, _P, _P, C.c_int64, _P, _P, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size or a pitch beyond the kernel's range", -3: "an unknown format or a coefficient outside its range"}
_lib = None


def load():
    """Load libpikazoo_ppo.so (once).  Raises, as ``policy.load()`` does, if it has not been built or was built from other
    sources than the ones in this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_ppo.hip", SIGNATURES, "pz_ppo_abi_version", ABI_VERSION)
    return _lib


def workspace_bytes(n: int) -> int:
    """bytes of scratch ``pz_ppo_moments`` and ``pz_ppo_loss`` need for ``n`` rows (the C entry point's own formula: no
    library is loaded for it)"""
    if not 0 < n <= 1 << 30:
        return 0
    loss = 2 * 5 * (-(-n // ROWS_PER_PARTIAL)) * 4
    mom = 2 * 2 * (-(-n // MOMENT_ROWS)) * 8
    return (max(loss, mom) + 15) & ~15


def _workspace(n, dev):
    return torch.empty(max(workspace_bytes(n), 16), dtype=torch.uint8, device=dev)


def moments(advantages, eps: float = 1e-8, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``[sides, 2]`` float32 on the device: ``(mean, 1 / (std + eps))`` of each agent's float32 ``[N]`` vector, ``std`` the
    unbiased deviation -- what ``(adv - adv.mean()) / (adv.std() + 1e-8)`` uses (``pz_ppo_moments``; accumulated in float64
    about the first element, in a fixed order: deterministic, and a mean far above the spread costs nothing).
    ``advantages``: a tensor (any shape, contiguous: it is read flat) or an ``{agent: tensor}`` dict of one or two agents.
    No allocation when ``out`` and ``workspace`` are given."""
    keys, xs = _sides(advantages, "advantages")
    x0 = xs[0]
    n, dev = x0.numel(), x0.device
    for x in xs:
        if x.dtype != torch.float32 or x.numel() != n or x.device != dev or not x.is_contiguous():
            raise ValueError(f"advantages must be contiguous float32 tensors of {n} elements on {dev}, got {x.dtype} {list(x.shape)} on {x.device}")
    if dev.type != "cuda":
        raise ValueError(f"the moments run on the GPU: advantages are on {dev}")
    if n < 2:
        raise ValueError(f"the unbiased deviation needs at least 2 elements, got {n}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    if out is None:
        out = torch.empty((len(xs), 2), dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (len(xs), 2) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{len(xs)}, 2] tensor on {dev}")
    ws = _workspace(n, dev) if workspace is None else _launch.check_workspace(workspace, workspace_bytes(n), dev)
    _launch.no_alias([("out", out), ("workspace", ws)], [("advantages", x) for x in xs])
    _launch.launch(load().pz_ppo_moments, _ERRORS, dev, *_ptrs(xs), n, eps, out.data_ptr(), ws.data_ptr())
    return out


def _values(x, what, keys, n, dev, dtype=None):
    """one element per row: [n] or [n, 1] tensors of a value format at any row stride >= 1, both agents alike -> (tensors, pitch)"""
    xkeys, ts = _sides(x, what)
    if xkeys != keys:
        raise ValueError(f"{what} must name the agents of the logits in their order: {keys}, got {xkeys}")
    pitches = set()
    for t in ts:
        if tuple(t.shape) not in ((n,), (n, 1)) or t.dtype not in VALUE_FORMATS or t.dtype != ts[0].dtype or t.device != dev:
            raise ValueError(f"{what} must be float32, float16 or bfloat16 [{n}] or [{n}, 1] on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
        if dtype is not None and t.dtype != dtype:
            raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
        if n > 1 and t.stride(0) < 1:
            raise ValueError(f"{what}: rows overlap (row stride {t.stride(0)})")
        pitches.add(int(t.stride(0)) if n > 1 else 1)
    if len(pitches) != 1:
        raise ValueError(f"{what}: both agents' tensors must have the same row stride, got {sorted(pitches)}")
    return ts, pitches.pop()


def _coefficient(x, what, low_open=False, high=None):
    x = float(x)
    if not math.isfinite(x) or x < 0 or (low_open and x == 0) or (high is not None and x >= high):
        raise ValueError(f"{what} must be finite and {'>' if low_open else '>='} 0{f' and < {high}' if high is not None else ''}, got {x}")
    return x


def loss_and_grad(logits=None, values=None, actions=None, old_log_probs=None, advantages=None, returns=None, old_values=None,
                  clip: float = 0.2, value_clip: Optional[float] = None, vf_coef: float = 0.5, ent_coef: float = 0.01,
                  normalize_advantages: bool = True, out: Optional[dict] = None, head=None, num_actions: Optional[int] = None):
    """The clipped PPO loss of a minibatch, its statistics and its gradients, for one or both agents (``pz_ppo_loss``, after
    ``pz_ppo_moments`` on the same stream when ``normalize_advantages``).

    ``logits``: ``[N, A]`` float32, float16 or bfloat16 as in :func:`pikazoo_amd.policy.sample`; ``values``: ``[N]`` or
    ``[N, 1]`` of a float format of its own at any row stride; ``actions``: int64 or int32 ``[N]``; ``old_log_probs``,
    ``advantages``, ``returns``: float32 ``[N]`` (what ``policy.sample`` and ``learn.gae`` produced, flattened and indexed
    by the minibatch); ``old_values``: ``[N]``, required iff ``value_clip`` is a positive number.  Tensors, or
    ``{agent: tensor}`` dicts of one or two agents, all alike.

    THE FUSED HEAD: ``head=`` the ``[N, A + 1]`` output of one ``Linear`` (logits and value together) with
    ``num_actions=A`` replaces ``logits`` and ``values``; the result then holds one ``grad_head`` of the same shape and
    dtype with every column written, for ``head_out.backward(grad_head)``.

    Returns ``{"loss", "stats", "grad_logits", "grad_values"}`` (``"grad_head"`` in place of the last two): the gradients
    of ``loss`` in the logits' and the values' dtypes; ``stats`` a dict of ``loss, policy_loss, value_loss, entropy,
    approx_kl, clip_fraction``, each a 0-dim float32 view (per agent, when given dicts); ``loss`` is ``stats["loss"]``.
    The definition, NaN rows included, is include/pikazoo_ppo.h's.  The result also carries the workspace and the
    moments: passed back as ``out=`` the call allocates nothing and can be captured into a graph.  Launches go to the
    current stream without a synchronisation.  Shape, dtype, device, range and aliasing errors raise ``ValueError`` before
    any launch."""
    fused = head is not None
    if fused:
        if logits is not None or values is not None:
            raise ValueError("give either head= (with num_actions=) or logits and values, not both")
        hkeys, hs = _sides(head, "head")
        A = int(num_actions) if num_actions is not None else -1
        for h in hs:
            if h.dim() != 2 or h.shape[1] != A + 1:
                raise ValueError(f"head must have shape [N, num_actions + 1] = [N, {A + 1}], got {tuple(h.shape)}")
        logits = _shape(hkeys, [h[:, :A] for h in hs])
        values = _shape(hkeys, [h[:, A] for h in hs])
    elif logits is None or values is None:
        raise ValueError("logits and values (or head= and num_actions=) are required")
    for what, x in (("actions", actions), ("old_log_probs", old_log_probs), ("advantages", advantages), ("returns", returns)):
        if x is None:
            raise ValueError(f"{what} is required")
    keys, ls, n, A, pitch, dev = _check_logits(logits)
    sides = len(ls)
    vs, value_pitch = _values(values, "values", keys, n, dev)
    act = _vectors(actions, "actions", keys, n, tuple(ACTION_FORMATS), dev)
    old_lp = _vectors(old_log_probs, "old_log_probs", keys, n, (torch.float32,), dev)
    adv = _vectors(advantages, "advantages", keys, n, (torch.float32,), dev)
    ret = _vectors(returns, "returns", keys, n, (torch.float32,), dev)
    clip = _coefficient(clip, "clip", low_open=True, high=1.0)
    value_clip = 0.0 if value_clip is None else _coefficient(value_clip, "value_clip")
    vf_coef, ent_coef = _coefficient(vf_coef, "vf_coef"), _coefficient(ent_coef, "ent_coef")
    if value_clip > 0:
        if old_values is None:
            raise ValueError("value_clip > 0 needs old_values")
        old_vs = _vectors(old_values, "old_values", keys, n, tuple(VALUE_FORMATS), dev)
    else:
        old_vs = None
    if normalize_advantages and n < 2:
        raise ValueError(f"normalize_advantages needs at least 2 rows, got {n}")
    grad_dtype, value_dtype = ls[0].dtype, vs[0].dtype
    if out is not None:
        if not isinstance(out, dict) or "_stats" not in out or "workspace" not in out or "adv_norm" not in out:
            raise ValueError("out must be the result of an earlier call")
        raw, ws, norm = out["_stats"], _launch.check_workspace(out["workspace"], workspace_bytes(n), dev), out["adv_norm"]
        if raw.dtype != torch.float32 or tuple(raw.shape) != (2, 8) or raw.device != dev or not raw.is_contiguous():
            raise ValueError(f"out['_stats'] must be a contiguous float32 [2, 8] tensor on {dev}")
        if norm.dtype != torch.float32 or tuple(norm.shape) != (2, 2) or norm.device != dev or not norm.is_contiguous():
            raise ValueError(f"out['adv_norm'] must be a contiguous float32 [2, 2] tensor on {dev}")
        if fused:
            gh = _sides(out.get("grad_head"), "out['grad_head']")
            if gh[0] != keys or any(tuple(g.shape) != (n, A + 1) or g.dtype != grad_dtype or g.device != dev or not g.is_contiguous() for g in gh[1]):
                raise ValueError(f"out['grad_head'] must hold contiguous {grad_dtype} [{n}, {A + 1}] tensors on {dev} for the agents {keys}")
            heads = gh[1]
        else:
            gl = _sides(out.get("grad_logits"), "out['grad_logits']")
            if gl[0] != keys or any(tuple(g.shape) != (n, A) or g.dtype != grad_dtype or g.device != dev or not g.is_contiguous() for g in gl[1]):
                raise ValueError(f"out['grad_logits'] must hold contiguous {grad_dtype} [{n}, {A}] tensors on {dev} for the agents {keys}")
            gls = gl[1]
            gvs = _vectors(out.get("grad_values"), "out['grad_values']", keys, n, (value_dtype,), dev)
    else:
        raw = torch.zeros((2, 8), dtype=torch.float32, device=dev)
        norm = torch.zeros((2, 2), dtype=torch.float32, device=dev)
        ws = _workspace(n, dev)
        if fused:
            heads = [torch.empty((n, A + 1), dtype=grad_dtype, device=dev) for _ in ls]
        else:
            gls = [torch.empty((n, A), dtype=grad_dtype, device=dev) for _ in ls]
            gvs = [torch.empty(n, dtype=value_dtype, device=dev) for _ in ls]
        stats = {name: _shape(keys, [raw[s, q] for s in range(sides)]) for q, name in enumerate(STAT_NAMES)}
        out = {"loss": stats["loss"], "stats": stats}
        if fused:
            out["grad_head"] = _shape(keys, heads)
        else:
            out["grad_logits"], out["grad_values"] = _shape(keys, gls), _shape(keys, gvs)
        out.update({"workspace": ws, "adv_norm": norm, "_stats": raw})
    if fused:
        gls, gvs = [h[:, :A] for h in heads], [h[:, A] for h in heads]
        grad_pitch = grad_value_pitch = A + 1
        outputs = [(f"grad_head[{s}]", h) for s, h in enumerate(heads)]
    else:
        grad_pitch, grad_value_pitch = A, 1
        outputs = [(f"grad_logits[{s}]", g) for s, g in enumerate(gls)] + [(f"grad_values[{s}]", g) for s, g in enumerate(gvs)]
    outputs += [("stats", raw), ("workspace", ws), ("adv_norm", norm)]
    inputs = [(what, t) for what, ts in (("logits", ls), ("values", vs), ("actions", act), ("old_log_probs", old_lp), ("advantages", adv),
                                         ("returns", ret), ("old_values", old_vs or [])) for t in ts]
    _launch.no_alias(outputs, inputs)
    if n == 0:
        return out
    lib = load()
    index = _launch.device_index(dev)
    none = (None, None)
    with torch.cuda.device(index):  # (both launches under one guard, on one stream)
        stream = _launch.raw_stream(index)
        if normalize_advantages:
            _launch.check(lib.pz_ppo_moments(*_ptrs(adv), n, 1e-8, norm.data_ptr(), ws.data_ptr(), stream), "pz_ppo_moments", _ERRORS)
        code = lib.pz_ppo_loss(*_ptrs(ls), LOGIT_FORMATS[grad_dtype], A, n, pitch, ACTION_FORMATS[act[0].dtype], *_ptrs(act), *_ptrs(old_lp),
                               *_ptrs(adv), *_ptrs(ret), *_ptrs(vs), VALUE_FORMATS[value_dtype], value_pitch,
                               *(_ptrs(old_vs) if old_vs is not None else none), VALUE_FORMATS[old_vs[0].dtype] if old_vs is not None else 0,
                               norm.data_ptr() if normalize_advantages else None, clip, value_clip, vf_coef, ent_coef, *_ptrs(gls),
                               grad_pitch, *_ptrs(gvs), grad_value_pitch, raw.data_ptr(), ws.data_ptr(), stream)
    _launch.check(code, "pz_ppo_loss", _ERRORS)
    return out


class _Loss(torch.autograd.Function):
    """(options, sides, differentiable tensors ...) -> the [2, 8] statistics; the forward IS the launch and saves the
    gradients it already has, the backward scales them by the upstream gradient of each agent's loss"""

    @staticmethod
    def forward(ctx, kwargs, fused, keys, *leaves):
        sides = len(leaves) if fused else len(leaves) // 2
        detached = [t.detach() for t in leaves]
        if fused:
            res = loss_and_grad(head=_shape(keys, detached), **kwargs)
            grads = _sides(res["grad_head"], "grad_head")[1]
        else:
            res = loss_and_grad(logits=_shape(keys, detached[:sides]), values=_shape(keys, detached[sides:]), **kwargs)
            grads = _sides(res["grad_logits"], "grad_logits")[1] + _sides(res["grad_values"], "grad_values")[1]
        ctx.save_for_backward(*grads)
        ctx.sides, ctx.shapes = sides, [t.shape for t in leaves]
        return res["_stats"]

    @staticmethod
    def backward(ctx, gstats):
        grads = ctx.saved_tensors
        out = []
        for i, g in enumerate(grads):
            up = gstats[i % ctx.sides, 0]  # d / d loss of this tensor's agent; the other statistics are for logging
            out.append((g * up.to(g.dtype)).reshape(ctx.shapes[i]))
        return (None, None, None, *out)


def loss(logits=None, values=None, actions=None, old_log_probs=None, advantages=None, returns=None, head=None, **options):
    """:func:`loss_and_grad` as a ``torch.autograd.Function``: returns ``(loss, stats)`` with ``loss`` (a 0-dim tensor, or
    an ``{agent: tensor}`` dict) differentiable with respect to the logits and the values, or the head.  The forward is
    the launch and saves the gradients it already has; the backward returns them multiplied by the upstream gradient --
    no second pass over the rows.  ``stats`` is detached.  Options as in :func:`loss_and_grad` (without ``out``).

    A training step captured into a graph should call :func:`loss_and_grad` with ``out=`` and then
    ``tensor.backward(grad)`` itself: this function allocates its results on every call."""
    if "out" in options:
        raise ValueError("ppo.loss takes no out=: use loss_and_grad for an allocation-free call")
    kwargs = dict(actions=actions, old_log_probs=old_log_probs, advantages=advantages, returns=returns, **options)
    fused = head is not None
    if fused:
        if logits is not None or values is not None:
            raise ValueError("give either head= (with num_actions=) or logits and values, not both")
        keys, leaves = _sides(head, "head")
    else:
        if logits is None or values is None:
            raise ValueError("logits and values (or head= and num_actions=) are required")
        keys, ls = _sides(logits, "logits")
        vkeys, vs = _sides(values, "values")
        if vkeys != keys:
            raise ValueError(f"values must name the agents of the logits in their order: {keys}, got {vkeys}")
        leaves = ls + vs
    raw = _Loss.apply(kwargs, fused, keys, *leaves)
    sides = len(leaves) if fused else len(leaves) // 2
    stats = {name: _shape(keys, [raw[s, q].detach() for s in range(sides)]) for q, name in enumerate(STAT_NAMES)}
    return _shape(keys, [raw[s, 0] for s in range(sides)]), stats
