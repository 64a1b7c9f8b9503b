"""V-trace targets for samples that are no longer on-policy: off-policy returns and advantages in ONE launch.

    from pikazoo_amd import policy, vtrace
    target, _ = policy.log_probs(logits_now, actions)                            # the CURRENT parameters on the stored actions
    out = vtrace.targets(rewards, values_now, terminations, stored_log_probs, target, gamma=0.99, lam=0.95)
    out["advantages"]["player_1"], out["returns"]["player_1"]                    # float32 [k, N]: ppo.loss takes them as they are

ctypes binding of libpikazoo_vtrace.so (C ABI and the exact arithmetic: include/pikazoo_vtrace.h), a library of its own;
nothing else imports this module, and it takes the argument checks of the trajectory tensors from ``learn``.  Where the two
log-prob tensors hold the same bits and the clips are >= 1 the result is ``learn.gae``'s, bit for bit.  There is no torch
fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _launch, _native
from .learn import REWARD_FORMATS, VALUE_FORMATS, _agents, _check_tensors, _flags, _outputs, _pitch, _rows, _unit

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_vtrace.so"
ABI_VERSION = 1

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
    val, lpb, lpt = (_agents(keys, x, name) for name, x in (("values", values), ("behaviour_log_probs", behaviour_log_probs),
                                                            ("target_log_probs", target_log_probs)))
    term = _flags(terminations)
    k, n, dev = _rows(rew[0], "targets")
    inputs = (("rewards", rew, (k, n), REWARD_FORMATS), ("values", val, (k + 1, n), VALUE_FORMATS),
              ("behaviour_log_probs", lpb, (k, n), (torch.float32,)), ("target_log_probs", lpt, (k, n), (torch.float32,)),
              ("terminations", [term], (k, n), (torch.bool, torch.uint8)))
    for name, ts, shape, dtypes in inputs:
        _check_tensors(name, ts, shape, dtypes, dev)
    gamma, lam, clip_rho, clip_c, clip_pg_rho = float(gamma), float(lam), float(clip_rho), float(clip_c), float(clip_pg_rho)
    _unit(gamma=gamma, lam=lam)
    for name, x in (("clip_rho", clip_rho), ("clip_c", clip_c), ("clip_pg_rho", clip_pg_rho)):
        if not (math.isfinite(x) and 0.0 <= x <= 3.4028234663852886e38):
            raise ValueError(f"{name} must be a finite float32 >= 0, got {x}")
    rew_pitch, val_pitch = _pitch(rew, k, n, "rewards"), _pitch(val, k + 1, n, "values")
    term_pitch = _pitch([term], k, n, "terminations")
    lp_pitch = _pitch(lpb + lpt, k, n, "behaviour_log_probs and target_log_probs")
    fresh = out is None
    out, pg, vs, out_pitch = _outputs(out, keys, len(rew), k, n, dev)
    if not fresh:
        _launch.no_alias([("out['advantages']", t) for t in pg] + [("out['returns']", t) for t in vs],
                         [(name, t) for name, ts, _, _ in inputs for t in ts])
    if n == 0:
        return out
    ptrs = _launch.ptrs
    _launch.launch(load().pz_vtrace, _ERRORS, dev, *ptrs(rew), REWARD_FORMATS[rew[0].dtype], term.data_ptr(), *ptrs(val),
                   VALUE_FORMATS[val[0].dtype], *ptrs(lpb), *ptrs(lpt), k, n, rew_pitch, term_pitch, val_pitch, lp_pitch, out_pitch,
                   gamma, lam, clip_rho, clip_c, clip_pg_rho, *ptrs(vs), *ptrs(pg))
    return out
