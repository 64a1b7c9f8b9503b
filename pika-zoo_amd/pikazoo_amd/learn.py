"""What a trainer does first with the trajectory tensors of a k-step launch: GAE(gamma, lambda) in ONE launch.

    from pikazoo_amd import learn
    traj = env.rollout_random(action_seed, k=32)
    out = learn.gae(traj["rewards"], values, traj["terminations"], gamma=0.99, lam=0.95)     # or env.gae(traj, values)
    out["advantages"]["player_1"], out["returns"]["player_1"]                                # float32 [k, N]

ctypes binding of libpikazoo_learn.so (C ABI and the exact arithmetic: include/pikazoo_learn.h), a library of its own
beside the product library; nothing in the step path imports this module.  It is the base module of the bindings over the
trajectory tensors: ``vtrace`` imports its argument checks and format tables from here, which loads no library.  There is
no torch fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _launch, _native

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_learn.so"
ABI_VERSION = 1
REWARD_FORMATS = {torch.int32: 0, torch.float32: 1}
VALUE_FORMATS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

_P = C.c_void_p
SIGNATURES = {
    "pz_learn_abi_version": (C.c_int, []),
    "pz_learn_build_id": (C.c_char_p, []),
    # (rew_p1, rew_p2, reward_format, terminated, val_p1, val_p2, value_format, k, n, the four pitches, gamma, lam,
    #  adv_p1, adv_p2, ret_p1, ret_p2, stream)
    "pz_gae": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                         C.c_int64, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size, a pitch or a tensor too large for the kernel's addressing",
           -3: "an unknown format, or gamma / lam outside [0, 1]"}
_lib = None


def load():
    """Load libpikazoo_learn.so (once).  Raises, as ``_native.load()`` does, if it has not been built or was built from
    other sources than the ones in this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_learn.hip", SIGNATURES, "pz_learn_abi_version", ABI_VERSION)
    return _lib


# ---- what every binding over the trajectory tensors checks (``vtrace`` imports these: this is the family's base module) ----
def _agents(keys, x, name):
    """the tensors of `x`, which must name the agents that ``rewards`` names (`keys`)"""
    other, ts = _launch.sides(x, name)
    if other != keys:
        raise ValueError(f"rewards and {name} must name the same agents in the same order: {keys} and {other}")
    return ts


def _flags(terminations):
    """the one tensor of flags that the agents share"""
    if isinstance(terminations, dict):
        flags = list(terminations.values())
        if not flags or any(not isinstance(f, torch.Tensor) for f in flags) or any(
                f.data_ptr() != flags[0].data_ptr() or f.shape != flags[0].shape or f.stride() != flags[0].stride()
                for f in flags[1:]):
            raise ValueError("terminations: the agents share one tensor of flags")
        terminations = flags[0]
    if not isinstance(terminations, torch.Tensor):
        raise ValueError(f"terminations must be a tensor, got {type(terminations).__name__}")
    return terminations


def _rows(r0, fn):
    """(k, n, device) of the first agent's rewards, for the function named `fn`"""
    if r0.dim() != 2 or r0.shape[0] < 1:
        raise ValueError(f"rewards must have shape [k, N] with k >= 1, got {tuple(r0.shape)}")
    if r0.device.type != "cuda":
        raise ValueError(f"{fn}() runs on the GPU: rewards are on {r0.device}")
    return int(r0.shape[0]), int(r0.shape[1]), r0.device


def _check_tensors(name, ts, shape, dtypes, dev):
    """every tensor of `ts` has `shape`, lies on `dev` and is of one of `dtypes` -- given a format table, of the first one's
    dtype where the table knows it"""
    if isinstance(dtypes, dict):
        dtypes = (ts[0].dtype,) if ts[0].dtype in dtypes else tuple(dtypes)
    for t in ts:
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
        if t.dtype not in dtypes:
            raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.device != dev:
            raise ValueError(f"{name} are on {t.device}, rewards on {dev}")


def _unit(**factors):
    for name, x in factors.items():
        if not (math.isfinite(x) and 0.0 <= x <= 1.0):
            raise ValueError(f"{name} must lie in [0, 1], got {x}")


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


def _outputs(out, keys, agents, k, n, dev):
    """(result, its advantages, its returns, their pitch): `out` -- a previous result of the same agents and shapes -- or, for
    None, fresh float32 [k, n] tensors in the shape of `keys`"""
    if out is None:
        adv = [torch.empty((k, n), dtype=torch.float32, device=dev) for _ in range(agents)]
        ret = [torch.empty((k, n), dtype=torch.float32, device=dev) for _ in range(agents)]
        return {"advantages": _launch.shape(keys, adv), "returns": _launch.shape(keys, ret)}, adv, ret, n
    if not isinstance(out, dict):
        raise ValueError(f"out= must be a previous result, got {type(out).__name__}")
    akeys, adv = _launch.sides(out.get("advantages"), "out['advantages']")
    rkeys, ret = _launch.sides(out.get("returns"), "out['returns']")
    if akeys != keys or rkeys != keys:
        raise ValueError(f"out= holds the agents {akeys} / {rkeys}, the call {keys}")
    for t in adv + ret:
        if tuple(t.shape) != (k, n) or t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"out= must hold float32 [{k}, {n}] tensors on {dev}")
    return out, adv, ret, _pitch(adv + ret, k, n, "out=")


def gae(rewards, values, terminations, gamma: float = 0.99, lam: float = 0.95, out: Optional[dict] = None):
    """GAE(gamma, lam) advantages and returns of one or both agents in one launch (``pz_gae``).

    ``rewards``: ``[k, N]`` int32 or float32, ``values``: ``[k + 1, N]`` float32, float16 or bfloat16 (row t is the value
    of the observation the action of step t was chosen on, row k the bootstrap) -- tensors, or ``{agent: tensor}`` dicts
    with the same one or two agents; ``terminations``: ``[k, N]`` bool or uint8, shared by the agents (a dict: every
    entry must be that one tensor's).  The last dimension is contiguous, any row stride >= N goes.  Returns
    ``{"advantages": ..., "returns": ...}``, float32 ``[k, N]``, in the shape of ``rewards`` (dicts for dicts).

    The arithmetic is pinned (include/pikazoo_learn.h): float32, round to nearest even, no fused multiply-add, nothing
    crosses an episode end.  The launch goes to the caller's current stream without a synchronisation, and without an
    allocation when ``out`` is the previous result of the same shapes: it can be captured into a graph.  Shape, dtype,
    device and range errors raise ``ValueError`` before any launch.  The outputs must not alias the inputs."""
    keys, rew = _launch.sides(rewards, "rewards")
    val = _agents(keys, values, "values")
    term = _flags(terminations)
    k, n, dev = _rows(rew[0], "gae")
    _check_tensors("rewards", rew, (k, n), REWARD_FORMATS, dev)
    _check_tensors("values", val, (k + 1, n), VALUE_FORMATS, dev)
    _check_tensors("terminations", [term], (k, n), (torch.bool, torch.uint8), dev)
    gamma, lam = float(gamma), float(lam)
    _unit(gamma=gamma, lam=lam)
    rew_pitch, val_pitch = _pitch(rew, k, n, "rewards"), _pitch(val, k + 1, n, "values")
    term_pitch = _pitch([term], k, n, "terminations")
    out, adv, ret, out_pitch = _outputs(out, keys, len(rew), k, n, dev)
    if n == 0:
        return out
    ptrs = _launch.ptrs
    _launch.launch(load().pz_gae, _ERRORS, dev, *ptrs(rew), REWARD_FORMATS[rew[0].dtype], term.data_ptr(), *ptrs(val), VALUE_FORMATS[val[0].dtype],
                   k, n, rew_pitch, term_pitch, val_pitch, out_pitch, gamma, lam, *ptrs(adv), *ptrs(ret))
    return out
