"""Egocentric observations: the row a player would be handed in the game mirrored about the court's centre line, so that
``player_2`` sees the court as ``player_1`` does, and the matching map of the 18 absolute actions, ONE launch each.

    from pikazoo_amd import ego
    ego.mirror(obs["player_2"], out=buf_obs[t])          # into a slot of a rollout buffer: the launch replaces the copy_
    ego.mirror(traj_obs, normalized=True, out=traj_obs)  # a whole [k, n, 35] float16 slab, in place
    ego.mirror_actions(actions, out=actions)             # left <-> right on Discrete(18); other values pass through

    from pikazoo_amd.wrappers import EgocentricObservation, NormalizeObservation, SimplifyAction
    env = EgocentricObservation(NormalizeObservation(SimplifyAction(env)))   # one net, either side

ctypes binding of libpikazoo_ego.so (C ABI and the definitions: include/pikazoo_ego.h), a library of its own beside the
product library; nothing in the step path or in the other modules imports this one, and importing it loads nothing.  There is
no torch fallback: a missing or stale library raises.  The result is fixed bit for bit by the header in every row format; the
launches allocate nothing with ``out=`` and do not synchronise, so they can be captured in a graph.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _launch, _native
from ._launch import describe as _describe

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_ego.so"
ABI_VERSION = 1
OBS_DIM = _native.OBS_DIM
COURT_WIDTH = 432
# the columns of a row that are mirrored: out = 432 - v (normalised: c - s) and out = 0 - v (normalised: 1 - s)
COURT_COLUMNS = (0, 13, 26, 28, 30)
SIGN_COLUMNS = (3, 16, 32)
# left <-> right on the 18 absolute actions
PI = (0, 1, 2, 4, 3, 5, 7, 6, 9, 8, 10, 12, 11, 13, 15, 14, 17, 16)
# (dtype, normalised) -> enum pz_obs_format (include/pikazoo_hip.h)
ROW_FORMATS = {(torch.int32, False): 0, (torch.float32, True): 1, (torch.int16, False): 2, (torch.float16, False): 3,
               (torch.bfloat16, False): 4, (torch.float16, True): 5, (torch.bfloat16, True): 6}
ROW_DTYPES = (torch.int32, torch.float32, torch.int16, torch.float16, torch.bfloat16)
ACTION_FORMATS = {torch.int32: 0, torch.int64: 1, torch.uint8: 2, torch.int16: 3}  # enum pz_action_format

_P = C.c_void_p

SIGNATURES = {
    "pz_ego_abi_version": (C.c_int, []),
    "pz_ego_build_id": (C.c_char_p, []),
    "pz_ego_error_string": (C.c_char_p, [C.c_int]),
    # (in, out, format, rows, in_pitch, out_pitch, stream)
    "pz_ego_rows": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _P]),
    # (in, out, action_format, n, stream)
    "pz_ego_actions": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a count, a pitch or an extent beyond the kernel's range", -3: "an unknown row or action format",
           -5: "the input and output ranges overlap without being the same rows"}
_lib = None


def load():
    """Load libpikazoo_ego.so (once).  Raises if it has not been built or was built from other sources than the ones in this
    tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_ego.hip", SIGNATURES, "pz_ego_abi_version", ABI_VERSION)
    return _lib


def row_format(dtype, normalized=None) -> int:
    """the ``pz_obs_format`` of rows of `dtype`: float32 rows are always normalised, the integer rows never, and float16 /
    bfloat16 rows are either, so they need ``normalized=``"""
    if dtype not in ROW_DTYPES:
        raise ValueError(f"rows must be {', '.join(str(d) for d in ROW_DTYPES)}, got {dtype}")
    if normalized is not None and not isinstance(normalized, bool):
        raise ValueError(f"normalized must be True, False or None, got {normalized!r}")
    if dtype == torch.float32:
        if normalized is False:
            raise ValueError("float32 rows are always normalised: there is no raw float32 row format")
        return 1
    if dtype in (torch.int32, torch.int16):
        if normalized:
            raise ValueError(f"{dtype} rows are never normalised")
        return ROW_FORMATS[dtype, False]
    if normalized is None:
        raise ValueError(f"{dtype} rows are raw or normalised: say which with normalized=")
    return ROW_FORMATS[dtype, normalized]


def _pitch(t, what):
    """(rows, pitch in elements) of a [..., 35] tensor whose leading dimensions collapse to one stride"""
    if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[-1] != OBS_DIM:
        raise ValueError(f"{what} must be a [..., {OBS_DIM}] tensor, got {_describe(t)}")
    if t.dtype not in ROW_DTYPES:
        raise ValueError(f"{what} must be {', '.join(str(d) for d in ROW_DTYPES)}, got {t.dtype}")
    rows = 1
    for s in t.shape[:-1]:
        rows *= int(s)
    if rows == 0:
        return 0, OBS_DIM
    if t.stride(-1) != 1:
        raise ValueError(f"{what}: the 35 elements of a row must lie back to back, got strides {list(t.stride())}")
    lead = [(int(s), int(st)) for s, st in zip(t.shape[:-1], t.stride()[:-1]) if s != 1]
    if not lead:
        return 1, OBS_DIM
    pitch = lead[-1][1]
    for (_, outer), (size, inner) in zip(lead[:-1], lead[1:]):
        if outer != inner * size:
            raise ValueError(f"{what}: the leading dimensions must collapse to one pitch, got strides {list(t.stride())}")
    if pitch < OBS_DIM:
        raise ValueError(f"{what}: rows must lie at a pitch of at least {OBS_DIM} elements, got strides {list(t.stride())}")
    return rows, pitch


def _extent(t, rows, pitch):
    return t.data_ptr(), t.data_ptr() + ((rows - 1) * pitch + OBS_DIM) * t.element_size()


def mirror(rows, normalized=None, out=None):
    """The egocentric view of observation rows, in one launch (``pz_ego_rows``; the definition is include/pikazoo_ego.h's):
    columns 0, 13, 26, 28, 30 (the x coordinates) become ``432 - v``, columns 3, 16, 32 (the diving directions and the ball's x
    velocity) ``-v``, in normalised rows ``c - s``; the other 27 columns are copied.  Returns ``out``.

    ``rows``: any ``[..., 35]`` int32, int16, float32, float16 or bfloat16 tensor whose rows lie at ONE pitch of at least 35
    elements (a contiguous tensor, a ``[k, n, 35]`` slab, a slot of one, a slice of rows, the front of a wider tensor).
    ``normalized``: float32 rows are always normalised and the integer rows never; float16 and bfloat16 rows are either, so
    they need the argument.  ``out=``: such a view of the same shape and dtype (allocated when ``None``, contiguous); ``rows``
    itself is allowed, a view that overlaps it in any other way raises.  Elements of ``out`` outside the rows' 35 columns are
    never written.

    No synchronisation; with ``out=`` no allocation.  Every shape, dtype, device or stride that the launch cannot take raises
    ``ValueError`` before any launch."""
    n, in_pitch = _pitch(rows, "rows")
    fmt = row_format(rows.dtype, normalized)
    if out is None:
        out_pitch = OBS_DIM
    else:
        m, out_pitch = _pitch(out, "out")
        if out.dtype != rows.dtype or tuple(out.shape) != tuple(rows.shape):
            raise ValueError(f"out must be {rows.dtype} {list(rows.shape)} like rows, got {_describe(out)}")
        if out.device != rows.device:
            raise ValueError(f"every tensor must be on one device: rows is on {rows.device}, out on {out.device}")
        if n and not (out.data_ptr() == rows.data_ptr() and in_pitch == out_pitch):
            (lo, hi), (olo, ohi) = _extent(rows, n, in_pitch), _extent(out, n, out_pitch)
            if lo < ohi and olo < hi:
                raise ValueError("out overlaps rows without being the same rows: mirror into rows itself or into memory apart from it")
    if rows.device.type != "cuda":
        raise ValueError(f"the ego launches run on the GPU: the tensors are on {rows.device}")
    if out is None:
        out = torch.empty(rows.shape, dtype=rows.dtype, device=rows.device)
    if n == 0:
        return out
    _launch.launch(load().pz_ego_rows, _ERRORS, rows.device, rows.data_ptr(), out.data_ptr(), fmt, n, in_pitch, out_pitch)
    return out


def mirror_actions(actions, out=None):
    """Left and right swapped on the 18 absolute actions, in one launch (``pz_ego_actions``): ``out[i] = PI[actions[i]]`` for
    ``0 <= actions[i] < 18``, any other value unchanged (the env's range check still sees it).  ``actions``: a contiguous
    int32, int64, uint8 or int16 tensor; ``out=``: a contiguous tensor of the same shape and dtype (allocated when ``None``),
    ``actions`` itself is allowed, any other overlap raises.  Returns ``out``.  Not for ``Discrete(13)``: the fused
    ``SimplifyAction`` already maps those per side.

    No synchronisation; with ``out=`` no allocation; ``ValueError`` before any launch for what the launch cannot take."""
    if not isinstance(actions, torch.Tensor) or actions.dtype not in ACTION_FORMATS or not actions.is_contiguous():
        raise ValueError(f"actions must be a contiguous {' or '.join(str(d) for d in ACTION_FORMATS)} tensor, got {_describe(actions)}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != actions.dtype or tuple(out.shape) != tuple(actions.shape) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {actions.dtype} {list(actions.shape)} tensor like actions, got {_describe(out)}")
        if out.device != actions.device:
            raise ValueError(f"every tensor must be on one device: actions is on {actions.device}, out on {out.device}")
        if out.data_ptr() != actions.data_ptr():
            _launch.no_alias([("out", out)], [("actions", actions)])
    if actions.device.type != "cuda":
        raise ValueError(f"the ego launches run on the GPU: the tensors are on {actions.device}")
    if out is None:
        out = torch.empty_like(actions)
    n = actions.numel()
    if n == 0:
        return out
    _launch.launch(load().pz_ego_actions, _ERRORS, actions.device, actions.data_ptr(), out.data_ptr(), ACTION_FORMATS[actions.dtype], n)
    return out
