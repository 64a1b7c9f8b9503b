"""The last step of a PPO update: the global gradient norm, the clip and the Adam / AdamW update of every parameter tensor of
one or two nets, with the moments and the step count, in ONE launch on parameters that ``net.forward`` reads in place.

    from pikazoo_amd import net, optim
    model = net.ActorCritic().to("cuda")
    optimizer = optim.Adam(model.parameters(), lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    loss.backward()
    optimizer.step()                                  # clip_grad_norm_(..., 0.5) + torch.optim.Adam.step(), one launch
    optimizer.stats["grad_norm"], optimizer.steps     # 0-dim views of what the launch wrote

    optim.adam_step(params, grads, exp_avg, exp_avg_sq, step, lr=3e-4, max_grad_norm=0.5)     # the same without the class

ctypes binding of libpikazoo_optim.so (C ABI and the definition: include/pikazoo_optim.h), a library of its own beside the
product library; nothing in the step path, ``learn``, ``policy``, ``ppo``, ``net`` or ``netgrad`` imports this module, and it
imports none of them.  There is no torch fallback: a missing or stale library raises.  The launch allocates nothing and does not synchronise: a captured graph
can hold a whole minibatch update, the step count included (it lives in device memory), and a learning rate given as a device
tensor is read at run time.  No atomics: the bits depend on the inputs only.  DEPARTURE from ``clip_grad_norm_``: gradients are
read only; the clipped gradient is never written back to ``.grad``.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _launch, _native

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_optim.so"
ABI_VERSION = 1
MAX_TENSORS = 16
MAX_GROUPS = 2
MAX_ELEMENTS = 1 << 20

_P = C.c_void_p


class Tensor(C.Structure):
    """pz_optim_tensor"""
    _fields_ = [("numel", C.c_int64), ("param", _P), ("grad", _P), ("exp_avg", _P), ("exp_avg_sq", _P)]


class Group(C.Structure):
    """pz_optim_group"""
    _fields_ = [("count", C.c_int32), ("tensors", Tensor * MAX_TENSORS), ("step", _P), ("stats", _P), ("lr_device", _P)]


class Config(C.Structure):
    """pz_adam_config"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double), ("decoupled", C.c_int32), ("skip_nonfinite", C.c_int32)]


SIGNATURES = {
    "pz_optim_abi_version": (C.c_int, []),
    "pz_optim_build_id": (C.c_char_p, []),
    # (groups, n_groups, cfg, stream)
    "pz_adam_step": (C.c_int, [C.POINTER(Group), C.c_int32, C.POINTER(Config), _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a group, tensor or element count beyond the kernel's range", -3: "a hyperparameter out of range"}
_lib = None


def load():
    """Load libpikazoo_optim.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_optim.hip", SIGNATURES, "pz_optim_abi_version", ABI_VERSION)
    return _lib


def _config(lr, betas, eps, weight_decay, decoupled, max_grad_norm, skip_nonfinite):
    """(Config, the device tensor of the learning rate or None); every range error of a host value"""
    lr_tensor = None
    if isinstance(lr, torch.Tensor):
        if lr.numel() != 1 or lr.dim() > 1 or lr.dtype != torch.float32:
            raise ValueError(f"lr as a tensor must be one float32 element on the device, got {lr.dtype} {list(lr.shape)}")
        lr_tensor, lr = lr, 0.0
    lr = float(lr)
    if not lr >= 0.0 or math.isinf(lr):
        raise ValueError(f"lr must be a finite number >= 0, got {lr}")
    if isinstance(betas, (int, float)) or len(betas) != 2:
        raise ValueError(f"betas must be a pair, got {betas!r}")
    b1, b2 = float(betas[0]), float(betas[1])
    for name, b in (("betas[0]", b1), ("betas[1]", b2)):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"{name} must be in [0, 1), got {b}")
    eps, weight_decay = float(eps), float(weight_decay)
    if not eps >= 0.0 or math.isinf(eps):
        raise ValueError(f"eps must be a finite number >= 0, got {eps}")
    if not weight_decay >= 0.0 or math.isinf(weight_decay):
        raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay}")
    if max_grad_norm is None:
        max_grad_norm = 0.0
    max_grad_norm = float(max_grad_norm)
    if math.isnan(max_grad_norm):
        raise ValueError("max_grad_norm must be a number or None (no clipping), got NaN")
    return Config(lr, b1, b2, eps, weight_decay, max_grad_norm, int(bool(decoupled)), int(bool(skip_nonfinite))), lr_tensor


def _sets(x, what, keys, groups):
    """the tensor sequences of `x`, one per group: a sequence, or an {agent: sequence} dict under the keys of `params`"""
    if isinstance(x, dict):
        if keys is None or list(x) != keys:
            raise ValueError(f"{what} must name the agents of params in their order: {keys}, got {list(x) if isinstance(x, dict) else None}")
        seqs = list(x.values())
    else:
        if keys is not None:
            raise ValueError(f"{what} must be a dict over {keys}, as params is")
        seqs = [x]
    out = []
    for seq in seqs:
        if isinstance(seq, torch.Tensor) or not hasattr(seq, "__len__"):
            raise ValueError(f"{what} must be a sequence of tensors, got {type(seq).__name__}")
        out.append(list(seq))
    if len(out) != groups:
        raise ValueError(f"{what}: {len(out)} groups, params has {groups}")
    return out


def _words(x, what, keys, groups, dtype, dev):
    """one contiguous two-element tensor of `dtype` per group (a tensor, or a dict of them)"""
    if isinstance(x, dict):
        if keys is None or list(x) != keys:
            raise ValueError(f"{what} must name the agents of params in their order: {keys}, got {list(x)}")
        ts = list(x.values())
    else:
        if keys is not None:
            raise ValueError(f"{what} must be a dict over {keys}, as params is")
        ts = [x]
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (2,) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of two elements on {dev}, got {_launch.describe(t)}")
    return ts


def _plan(params, grads, exp_avg, exp_avg_sq, step, stats, cfg, lr_tensor):
    """Every check that needs no library, then (Group array, number of groups, device).  The ctypes structs hold addresses
    only: the caller keeps the tensors alive."""
    if isinstance(params, dict):
        keys = list(params)
        if not 1 <= len(keys) <= MAX_GROUPS:
            raise ValueError(f"params: a dict of one or two agents, got {len(keys)}")
    else:
        keys = None
    n_groups = len(keys) if keys is not None else 1
    ps = _sets(params, "params", keys, n_groups)
    gs, ms, vs = (_sets(x, what, keys, n_groups) for x, what in ((grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")))
    first = ps[0][0] if ps[0] else None
    if not isinstance(first, torch.Tensor):
        raise ValueError("params: a group must hold at least one tensor")
    dev = first.device
    for a in range(n_groups):
        count = len(ps[a])
        if not 1 <= count <= MAX_TENSORS:
            raise ValueError(f"a group holds 1..{MAX_TENSORS} tensors, got {count}")
        for what, seq in (("grads", gs[a]), ("exp_avg", ms[a]), ("exp_avg_sq", vs[a])):
            if len(seq) != count:
                raise ValueError(f"{what}: {len(seq)} tensors for {count} parameters")
        total = 0
        for i in range(count):
            for what, t in (("params", ps[a][i]), ("grads", gs[a][i]), ("exp_avg", ms[a][i]), ("exp_avg_sq", vs[a][i])):
                if not isinstance(t, torch.Tensor):
                    raise ValueError(f"{what}[{i}] must be a tensor, got {type(t).__name__}")
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() < 1:
                    raise ValueError(f"{what}[{i}] must be a contiguous float32 tensor of at least one element on {dev}, got {t.dtype} "
                                     f"{list(t.shape)} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
                if tuple(t.shape) != tuple(ps[a][i].shape):
                    raise ValueError(f"{what}[{i}] has shape {list(t.shape)}, its parameter {list(ps[a][i].shape)}")
            total += ps[a][i].numel()
        if total > MAX_ELEMENTS:
            raise ValueError(f"a group holds at most 2^20 elements, got {total}")
    steps = _words(step, "step", keys, n_groups, torch.int64, dev)
    stat = _words(stats, "stats", keys, n_groups, torch.float32, dev) if stats is not None else [None] * n_groups
    if lr_tensor is not None and lr_tensor.device != dev:
        raise ValueError(f"lr as a tensor must be on {dev}, got {lr_tensor.device}")
    outputs = [(f"{what}[{a}][{i}]", t) for a in range(n_groups) for what, seqs in (("params", ps), ("exp_avg", ms), ("exp_avg_sq", vs))
               for i, t in enumerate(seqs[a])]
    outputs += [(f"step[{a}]", t) for a, t in enumerate(steps)] + [(f"stats[{a}]", t) for a, t in enumerate(stat) if t is not None]
    inputs = [(f"grads[{a}][{i}]", t) for a in range(n_groups) for i, t in enumerate(gs[a])]
    if lr_tensor is not None:
        inputs.append(("lr", lr_tensor))
    _launch.no_alias(outputs, inputs)
    if dev.type != "cuda":
        raise ValueError(f"the optimizer step runs on the GPU: the parameters are on {dev}")
    array = (Group * MAX_GROUPS)()
    for a in range(n_groups):
        g = array[a]
        g.count = len(ps[a])
        for i, (p, gr, m, v) in enumerate(zip(ps[a], gs[a], ms[a], vs[a])):
            g.tensors[i] = Tensor(p.numel(), p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr())
        g.step = steps[a].data_ptr()
        g.stats = stat[a].data_ptr() if stat[a] is not None else None
        g.lr_device = lr_tensor.data_ptr() if lr_tensor is not None else None
    return array, n_groups, dev


def _run(array, n_groups, cfg, dev):
    """the launch of a checked plan: what ``Adam.step()`` pays on every call"""
    lib = load()
    index = _launch.device_index(dev)
    with torch.cuda.device(index):
        code = lib.pz_adam_step(array, n_groups, C.byref(cfg), _launch.raw_stream(index))
    if code != 0:
        _launch.check(code, "pz_adam_step", _ERRORS)


def adam_step(params, grads, exp_avg, exp_avg_sq, step, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
              max_grad_norm=None, skip_nonfinite=False, stats=None):
    """One Adam / AdamW step with the gradient clip in front of it, in one launch (``pz_adam_step``; the definition is
    include/pikazoo_optim.h's): ``clip_grad_norm_(params, max_grad_norm)`` and ``torch.optim.Adam(...).step()`` (``decoupled``:
    ``AdamW``) on ``params`` in place, except that ``grads`` are read only.

    ``params``, ``grads``, ``exp_avg`` and ``exp_avg_sq`` are sequences of 1..16 contiguous float32 device tensors of equal
    shapes, at most 2^20 elements together -- one net, with one gradient norm and one step count -- or ``{agent: sequence}``
    dicts of two for two separate nets in the same launch.  ``step``: a contiguous int64 tensor ``[t, skipped]`` on the device
    (a dict of them for two nets); ``stats``: optionally a float32 tensor of two that receives ``[grad_norm, clip_coef]``.
    ``lr`` is a float or a one-element float32 device tensor that the kernel reads when it runs (change it between replays of
    a captured graph).  ``max_grad_norm=None`` (or <= 0, or inf): no clipping.  ``skip_nonfinite``: a group whose gradient norm
    is not finite is left untouched and ``skipped`` counts it.

    Allocates nothing and does not synchronise.  Outputs must not overlap each other or a gradient.  Shape, dtype, stride,
    alias and range errors raise ``ValueError`` before the library is needed."""
    cfg, lr_tensor = _config(lr, betas, eps, weight_decay, decoupled, max_grad_norm, skip_nonfinite)
    array, n_groups, dev = _plan(params, grads, exp_avg, exp_avg_sq, step, stats, cfg, lr_tensor)
    _run(array, n_groups, cfg, dev)


_OPTIONS = ("lr", "betas", "eps", "weight_decay", "decoupled", "max_grad_norm", "skip_nonfinite")


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (``decoupled=True``: ``AdamW``) with ``clip_grad_norm_(..., max_grad_norm)`` in front of it, one
    launch per :meth:`step` for one or two param groups of equal options (param groups whose options differ get a launch
    each).  A param group is a group of include/pikazoo_optim.h: one net, one gradient norm, one step count.

    Parameters whose ``.grad`` is None are left out of the launch and of the norm.  The moments (``exp_avg``, ``exp_avg_sq``
    in ``state[p]``) and the step words (``state[first parameter of the group]["step"]``: int64 ``[t, skipped]`` on the device)
    are allocated on the first :meth:`step`; ``state_dict`` / ``load_state_dict`` round-trip them.  ``lr`` may be a float or a
    one-element float32 device tensor.  ``.grad`` is never modified."""

    def __init__(self, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None,
                 skip_nonfinite=False):
        _config(lr, betas, eps, weight_decay, decoupled, max_grad_norm, skip_nonfinite)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled=bool(decoupled),
                                      max_grad_norm=max_grad_norm, skip_nonfinite=bool(skip_nonfinite)))
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} param groups (two nets), got {len(self.param_groups)}")
        self._stats = {}
        self._plans = {}

    def _words_of(self, group):
        """(step words, statistics) of a param group, allocated on first use"""
        first = group["params"][0]
        state = self.state[first]
        if "step" not in state:
            state["step"] = torch.zeros(2, dtype=torch.int64, device=first.device)
        if id(first) not in self._stats:
            self._stats[id(first)] = torch.zeros(2, dtype=torch.float32, device=first.device)
        return state["step"], self._stats[id(first)]

    def _views(self, which, index):
        views = [self._words_of(g)[which][index] for g in self.param_groups]
        return views[0] if len(views) == 1 else views

    @property
    def stats(self):
        """``{"grad_norm", "clip_coef"}`` of the last step as 0-dim views (lists of two for two param groups)"""
        return {"grad_norm": self._views(1, 0), "clip_coef": self._views(1, 1)}

    @property
    def steps(self):
        """the number of updates made: a 0-dim int64 view (a list of two for two param groups)"""
        return self._views(0, 0)

    @property
    def skipped(self):
        """the number of steps skipped for a non-finite gradient norm: a 0-dim int64 view"""
        return self._views(0, 1)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans.clear()
        for group in self.param_groups:
            state = self.state[group["params"][0]]
            if "step" in state:
                state["step"] = state["step"].to(device=group["params"][0].device, dtype=torch.int64).contiguous()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if ps:
                live.append((group, ps))
        if not live:
            return loss
        options = [tuple((k, g[k] if not isinstance(g[k], torch.Tensor) else id(g[k])) for k in _OPTIONS) for g, _ in live]
        batches = [live] if all(o == options[0] for o in options) else [[entry] for entry in live]
        for b, batch in enumerate(batches):
            key = tuple((p.data_ptr(), p.grad.data_ptr()) for _, ps in batch for p in ps) + (len(batch), options[b])
            plan = self._plans.get(key)
            if plan is None:
                plan = self._plans[key] = self._make_plan(batch)
                if len(self._plans) > 8:  # (gradients that move every step: keep the table small)
                    self._plans.pop(next(iter(self._plans)))
            array, n_groups, cfg, dev, _alive = plan
            _run(array, n_groups, cfg, dev)
        return loss

    def _make_plan(self, batch):
        group = batch[0][0]
        cfg, lr_tensor = _config(*(group[k] for k in _OPTIONS))
        sets = {what: {} for what in ("params", "grads", "exp_avg", "exp_avg_sq", "step", "stats")}
        for a, (g, ps) in enumerate(batch):
            for p in ps:
                state = self.state[p]
                if "exp_avg" not in state:
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            sets["params"][a] = [p.data for p in ps]
            sets["grads"][a] = [p.grad for p in ps]
            sets["exp_avg"][a] = [self.state[p]["exp_avg"] for p in ps]
            sets["exp_avg_sq"][a] = [self.state[p]["exp_avg_sq"] for p in ps]
            sets["step"][a], sets["stats"][a] = self._words_of(g)
        if len(batch) == 1:
            sets = {what: d[0] for what, d in sets.items()}
        array, n_groups, dev = _plan(sets["params"], sets["grads"], sets["exp_avg"], sets["exp_avg_sq"], sets["step"], sets["stats"], cfg,
                                     lr_tensor)
        return array, n_groups, cfg, dev, sets
