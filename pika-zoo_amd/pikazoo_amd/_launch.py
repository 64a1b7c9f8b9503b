"""What stands between a learner binding's own argument checks and its C call, defined once: the device index and the raw
stream of a launch, the launch itself with its error text, the overlap check of outputs against inputs, the tensor-or-dict
convention of the two agents, and the workspace check.  ``learn``, ``policy``, ``ppo``, ``net``, ``netgrad``, ``optim``,
``batch``, ``pool``, ``league``, ``act``, ``pool_act`` and ``vtrace`` use it (``env`` takes :func:`raw_stream` alone); it imports none of
them and loads no library.  A helper that belongs to one family of bindings stays in that family's base module
(``net._rows``, ``policy._check_logits``, ``learn._pitch``): this module knows nothing of any kernel."""
from __future__ import annotations

import torch

from ._native import PikazooNativeError

# the two texts that every binding's table shares; a module adds its own -2 and -3
ERRORS = {-1: "a required pointer is NULL", -4: "a pointer not aligned to its element"}

# torch.cuda.current_stream(...).cuda_stream builds a Stream object per call (2.8 us); the raw getter behind it costs 0.08 us
_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def raw_stream(index: int) -> int:
    """the current stream of device `index` as the address a C entry point takes"""
    if _get_raw_stream is not None:
        return _get_raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def device_index(dev) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def check(code, name, errors):
    if code != 0:
        raise PikazooNativeError(f"{name} failed: {errors.get(code, 'HIP error')} (code {code})")


def launch(fn, errors, dev, *args):
    """``fn(*args, stream)`` -- one C entry point of a loaded library -- on the current stream of `dev`, with `dev` the
    current device; a non-zero code raises ``PikazooNativeError`` in the words of `errors`"""
    index = device_index(dev)
    with torch.cuda.device(index):
        code = fn(*args, raw_stream(index))
    if code != 0:
        check(code, fn.__name__, errors)


def span(t):
    """[first byte, last byte + 1) of the memory a tensor's elements lie in"""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    return t.data_ptr(), t.data_ptr() + (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def no_alias(outputs, inputs):
    """no output overlaps an input or an earlier output; both are lists of (name, tensor)"""
    spans = [(what, span(t)) for what, t in inputs]
    for i, (what, t) in enumerate(outputs):
        lo, hi = span(t)
        for other, (olo, ohi) in spans + [(w, span(u)) for w, u in outputs[:i]]:
            if lo < ohi and olo < hi:
                raise ValueError(f"{what} overlaps {other}: outputs must not alias an input or each other")


def sides(x, what):
    """(keys or None, [tensor, ...]) of a tensor or an {agent: tensor} dict of one or two agents"""
    if isinstance(x, dict):
        if not 1 <= len(x) <= 2:
            raise ValueError(f"{what}: a dict of one or two agents, got {len(x)}")
        keys, vals = list(x), list(x.values())
    else:
        keys, vals = None, [x]
    for v in vals:
        if not isinstance(v, torch.Tensor):
            raise ValueError(f"{what} must be a tensor or a dict of tensors, got {type(v).__name__}")
    return keys, vals


def shape(keys, ts):
    """:func:`sides` undone: the dict over `keys`, or the one tensor"""
    return dict(zip(keys, ts)) if keys is not None else ts[0]


def ptrs(ts):
    """the two pointers a C entry point takes for one or two agents' tensors"""
    return ts[0].data_ptr(), (ts[1].data_ptr() if len(ts) == 2 else None)


def describe(t):
    """what an error message says it got"""
    return f"{t.dtype} {list(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__


def check_workspace(ws, need, dev):
    if (not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous() or ws.device != dev
            or ws.numel() < need or ws.data_ptr() % 16):
        raise ValueError(f"the workspace must be a contiguous uint8 tensor of at least {need} bytes on {dev}, aligned to 16")
    return ws
