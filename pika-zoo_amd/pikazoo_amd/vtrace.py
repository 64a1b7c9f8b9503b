"""V-trace targets for samples that are no longer on-policy: off-policy returns and advantages in ONE launch.

    from pikazoo_amd import policy, vtrace
    target, _ = policy.log_probs(logits_now, actions)                            # the CURRENT parameters on the stored actions
    out = vtrace.targets(rewards, values_now, terminations, stored_log_probs, target, gamma=0.99, lam=0.95)
    out["advantages"]["player_1"], out["returns"]["player_1"]                    # float32 [k, N]: ppo.loss takes them as they are

ctypes binding of libpikazoo_vtrace.so (C ABI and the exact arithmetic: include/pikazoo_vtrace.h), a library of its own;
nothing else imports this module.  Where the two log-prob tensors hold the same bits and the clips are >= 1 the result is
``learn.gae``'s, bit for bit.  There is no torch fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _launch, _native

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_vtrace.so"
ABI_VERSION = 1
REWARD_FORMATS = {torch.int32: 0, torch.float32: 1}
VALUE_FORMATS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

_P = C.c_void_p
SIGNATURES = {
    "pz_vtrace_abi_version": (C.c_int, []),
    "pz_vtrace_build_id": (C.c_char_p, []),
    # (rew_p1, rew_p2, reward_format, terminated, val_p1, val_p2, value_format, lpb_p1, lpb_p2, lpt_p1, lpt_p2, k, n, the five
    #  pitches, gamma, lam, clip_rho, clip_c, clip_pg_rho, vs_p1, vs_p2, pg_p1, pg_p2, stream)
    "pz_vtrace": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                            C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch or a tensor too large for the kernel's addressing",
           -3: "an unknown format, gamma / lam outside [0, 1], or a clip that is negative or not finite"}
_lib = None


def load():
    """Load libpikazoo_vtrace.so (once).  Raises, as ``_native.load()`` does, if it has not been built or was built from
    other sources than the ones in this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_vtrace.hip", SIGNATURES, "pz_vtrace_abi_version", ABI_VERSION)
    return _lib


def _pitch(ts, rows, n, what):
    """the row pitch, in elements, that the tensors of `ts` ([rows, n], last dimension contiguous) share"""
    pitches = set()
    for t in ts:
        if n > 1 and t.stride(1) != 1:
            raise ValueError(f"{what}: the last dimension must be contiguous (stride {t.stride(1)})")
        pitches.add(max(int(t.stride(0)), n) if rows > 1 else n)
        if rows > 1 and t.stride(0) < n:
            raise ValueError(f"{what}: rows overlap (row stride {t.stride(0)} < {n})")
    if len(pitches) != 1:
        raise ValueError(f"{what}: the tensors must share one row stride, got {sorted(pitches)}")
    return pitches.pop()


def targets(rewards, values, terminations, behaviour_log_probs, target_log_probs, gamma: float = 0.99, lam: float = 1.0,
            clip_rho: float = 1.0, clip_c: float = 1.0, clip_pg_rho: float = 1.0, out: Optional[dict] = None):
    """V-trace value targets and policy-gradient advantages of one or both agents in one launch (``pz_vtrace``).

    ``rewards``: ``[k, N]`` int32 or float32; ``values``: ``[k + 1, N]`` float32, float16 or bfloat16, the values of the
    CURRENT parameters (row k the bootstrap); ``behaviour_log_probs``: ``[k, N]`` float32, what the policy that acted gave
    the stored action (``policy.sample`` / ``act.sample``); ``target_log_probs``: ``[k, N]`` float32, what the current
    parameters give it (``policy.log_probs``) -- tensors, or ``{agent: tensor}`` dicts with the same one or two agents;
    ``terminations``: ``[k, N]`` bool or uint8, shared by the agents (a dict: every entry must be that one tensor's).  The
    last dimension is contiguous, any row stride >= N goes; the four log-prob tensors share theirs.  Returns
    ``{"advantages": ..., "returns": ...}`` -- ``learn.gae``'s keys: ``returns`` is the v-trace target ``vs``,
    ``advantages`` the clipped-weight advantage ``pg_adv`` -- float32 ``[k, N]``, in the shape of ``rewards``.

    The arithmetic is pinned (include/pikazoo_vtrace.h): float32, round to nearest even, no fused multiply-add, nothing
    crosses an episode end; the importance weight's ``expf`` is the one operation not pinned to the bit, and it is skipped
    where the two log-probs are equal.  The launch goes to the caller's current stream without a synchronisation, and
    without an allocation when ``out`` is the previous result of the same shapes: it can be captured into a graph.  Shape,
    dtype, device, stride, range and agent-set errors raise ``ValueError`` before any launch.  The outputs must not alias
    the inputs."""
    keys, rew = _launch.sides(rewards, "rewards")
    rest = []
    for name, x in (("values", values), ("behaviour_log_probs", behaviour_log_probs), ("target_log_probs", target_log_probs)):
        other, ts = _launch.sides(x, name)
        if other != keys:
            raise ValueError(f"rewards and {name} must name the same agents in the same order: {keys} and {other}")
        rest.append(ts)
    val, lpb, lpt = rest
    if isinstance(terminations, dict):
        flags = list(terminations.values())
        if not flags or any(not isinstance(f, torch.Tensor) for f in flags) or any(
                f.data_ptr() != flags[0].data_ptr() or f.shape != flags[0].shape or f.stride() != flags[0].stride()
                for f in flags[1:]):
            raise ValueError("terminations: the agents share one tensor of flags")
        term = flags[0]
    else:
        term = terminations
    if not isinstance(term, torch.Tensor):
        raise ValueError(f"terminations must be a tensor, got {type(term).__name__}")
    r0 = rew[0]
    if r0.dim() != 2 or r0.shape[0] < 1:
        raise ValueError(f"rewards must have shape [k, N] with k >= 1, got {tuple(r0.shape)}")
    k, n = int(r0.shape[0]), int(r0.shape[1])
    dev = r0.device
    if dev.type != "cuda":
        raise ValueError(f"targets() runs on the GPU: rewards are on {dev}")
    for name, ts, shape, dtypes in (("rewards", rew, (k, n), (r0.dtype,) if r0.dtype in REWARD_FORMATS else tuple(REWARD_FORMATS)),
                                    ("values", val, (k + 1, n), (val[0].dtype,) if val[0].dtype in VALUE_FORMATS else tuple(VALUE_FORMATS)),
                                    ("behaviour_log_probs", lpb, (k, n), (torch.float32,)),
                                    ("target_log_probs", lpt, (k, n), (torch.float32,)),
                                    ("terminations", [term], (k, n), (torch.bool, torch.uint8))):
        for t in ts:
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} are on {t.device}, rewards on {dev}")
    gamma, lam, clip_rho, clip_c, clip_pg_rho = float(gamma), float(lam), float(clip_rho), float(clip_c), float(clip_pg_rho)
    for name, x in (("gamma", gamma), ("lam", lam)):
        if not (math.isfinite(x) and 0.0 <= x <= 1.0):
            raise ValueError(f"{name} must lie in [0, 1], got {x}")
    for name, x in (("clip_rho", clip_rho), ("clip_c", clip_c), ("clip_pg_rho", clip_pg_rho)):
        if not (math.isfinite(x) and 0.0 <= x <= 3.4028234663852886e38):
            raise ValueError(f"{name} must be a finite float32 >= 0, got {x}")
    rew_pitch, val_pitch = _pitch(rew, k, n, "rewards"), _pitch(val, k + 1, n, "values")
    term_pitch = _pitch([term], k, n, "terminations")
    lp_pitch = _pitch(lpb + lpt, k, n, "behaviour_log_probs and target_log_probs")

    if out is not None:
        if not isinstance(out, dict):
            raise ValueError(f"out= must be a previous result, got {type(out).__name__}")
        akeys, pg = _launch.sides(out.get("advantages"), "out['advantages']")
        rkeys, vs = _launch.sides(out.get("returns"), "out['returns']")
        if akeys != keys or rkeys != keys or len(pg) != len(rew) or len(vs) != len(rew):
            raise ValueError(f"out= holds the agents {akeys} / {rkeys}, the call {keys}")
        for t in pg + vs:
            if tuple(t.shape) != (k, n) or t.dtype != torch.float32 or t.device != dev:
                raise ValueError(f"out= must hold float32 [{k}, {n}] tensors on {dev}")
        out_pitch = _pitch(pg + vs, k, n, "out=")
        _launch.no_alias([("out['advantages']", t) for t in pg] + [("out['returns']", t) for t in vs],
                         [(name, t) for name, ts in (("rewards", rew), ("values", val), ("behaviour_log_probs", lpb),
                                                     ("target_log_probs", lpt), ("terminations", [term])) for t in ts])
    else:
        pg = [torch.empty((k, n), dtype=torch.float32, device=dev) for _ in rew]
        vs = [torch.empty((k, n), dtype=torch.float32, device=dev) for _ in rew]
        out_pitch = n
        out = {"advantages": _launch.shape(keys, pg), "returns": _launch.shape(keys, vs)}
    if n == 0:
        return out
    ptrs = _launch.ptrs
    _launch.launch(load().pz_vtrace, _ERRORS, dev, *ptrs(rew), REWARD_FORMATS[r0.dtype], term.data_ptr(), *ptrs(val),
                   VALUE_FORMATS[val[0].dtype], *ptrs(lpb), *ptrs(lpt), k, n, rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch,
                   gamma, lam, clip_rho, clip_c, clip_pg_rho, *ptrs(vs), *ptrs(pg))
    return out
