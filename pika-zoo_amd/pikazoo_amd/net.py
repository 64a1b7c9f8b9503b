"""What a trainer runs on every policy step between ``env.step()``'s observation rows and the ``[N, A + 1]`` head that
``policy.sample`` and ``ppo.loss(head=...)`` read: a three-layer policy net, forward, in ONE launch.

    from pikazoo_amd import net, policy
    model = net.ActorCritic(in_features=35, hidden=64, num_actions=18).to("cuda")
    head = model.act(obs)                                   # the rollout side: one launch per step, both agents, no graph
    out = policy.sample({a: h[:, :18] for a, h in head.items()}, seed=7, step=t)
    head = {a: model(o) for a, o in obs.items()}            # the update side: torch autograd on the same parameters

ctypes binding of libpikazoo_net.so (C ABI and the definition: include/pikazoo_net.h), a library of its own beside the
product library; nothing in the step path, ``learn``, ``policy`` or ``ppo`` imports this module.  There is no torch
fallback: a missing or stale library raises.  Operands and accumulation are float32, the parameters are torch's own
``nn.Linear`` tensors read in place, and a row's bits do not depend on the batch around it.  The argument check of the net
(``_observations``, ``_box``, ``_outputs``) is also ``pool.forward``'s and ``netgrad.backward``'s; the launch plumbing is
``_launch``'s.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _launch, _native

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_net.so"
ABI_VERSION = 1
OBS_FORMATS = {torch.int32: 0, torch.int16: 1, torch.float32: 2, torch.float16: 3, torch.bfloat16: 4}
OUT_FORMATS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACTIVATIONS = {"tanh": 0, "relu": 1}
MAX_IN, HIDDEN, MAX_OUT = 72, (32, 64, 128), 40

_P = C.c_void_p
SIGNATURES = {
    "pz_net_abi_version": (C.c_int, []),
    "pz_net_build_id": (C.c_char_p, []),
    # (obs_p1, obs_p2, obs_format, n, in_features, obs_pitch, hidden, out_features, activation, w1_p1, b1_p1, w2_p1, b2_p1, w3_p1,
    #  b3_p1, w1_p2, b1_p2, w2_p2, b2_p2, w3_p2, b3_p2, out_p1, out_p2, out_format, out_pitch, stream)
    "pz_mlp_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int64, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a size or a pitch beyond the kernel's range", -3: "an unknown format or activation"}
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
_lib = None


def load():
    """Load libpikazoo_net.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_net.hip", SIGNATURES, "pz_net_abi_version", ABI_VERSION)
    return _lib


def _rows(ts, what, n, width, dtypes, dev):
    """the common row stride of [n, width] tensors whose last dimension is contiguous"""
    pitches = set()
    for t in ts:
        if t.dim() != 2 or tuple(t.shape) != (n, width) or t.dtype not in dtypes or t.dtype != ts[0].dtype or t.device != dev:
            raise ValueError(f"{what} must be {' or '.join(str(d) for d in dtypes)} [{n}, {width}] on {dev}, got {t.dtype} "
                             f"{list(t.shape)} on {t.device}")
        if width > 1 and t.stride(1) != 1:
            raise ValueError(f"{what}: the last dimension must be contiguous (stride {t.stride(1)})")
        if n > 1 and t.stride(0) < width:
            raise ValueError(f"{what}: rows overlap (row stride {t.stride(0)} < {width})")
        pitches.add(int(t.stride(0)) if n > 1 else width)
    if len(pitches) != 1:
        raise ValueError(f"{what}: both agents' tensors must have the same row stride, got {sorted(pitches)}")
    return pitches.pop()


def _parameter_sets(params, keys, sides):
    if isinstance(params, dict):
        if keys is None or list(params) != keys:
            raise ValueError(f"params must name the agents of obs in their order: {keys}, got {list(params)}")
        sets = list(params.values())
    else:
        sets = [params] * sides  # one sequence for two agents: shared weights
    out = []
    for ps in sets:
        if isinstance(ps, torch.Tensor) or not hasattr(ps, "__len__") or len(ps) != 6:
            raise ValueError("params must be a sequence of six tensors (W1, b1, W2, b2, W3, b3), or an {agent: ...} dict of them")
        for p in ps:
            if not isinstance(p, torch.Tensor):
                raise ValueError(f"a parameter must be a tensor, got {type(p).__name__}")
        out.append([p.data for p in ps])
    return out


# ---- the argument check of every launch on this net: forward, pool.forward and netgrad.backward ---------------------------------
def _observations(obs, activation):
    """(keys, tensors, n, K, device, row pitch) of the observations of one or two agents, and the activation's name checked"""
    keys, xs = _launch.sides(obs, "obs")
    x0 = xs[0]
    if x0.dim() != 2:
        raise ValueError(f"obs must have shape [N, K], got {tuple(x0.shape)}")
    n, K, dev = int(x0.shape[0]), int(x0.shape[1]), x0.device
    if not 1 <= K <= MAX_IN:
        raise ValueError(f"obs: 1 <= K <= {MAX_IN} features, got {K}")
    if n > 1 << 30:
        raise ValueError(f"obs: at most 2^30 rows, got {n}")
    if x0.dtype not in OBS_FORMATS:
        raise ValueError(f"obs must be {' or '.join(str(d) for d in OBS_FORMATS)}, got {x0.dtype}")
    obs_pitch = _rows(xs, "obs", n, K, tuple(OBS_FORMATS), dev)
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be {' or '.join(repr(a) for a in ACTIVATIONS)}, got {activation!r}")
    return keys, xs, n, K, dev, obs_pitch


def _box(sets, K, dev, label=""):
    """(H, O, the six shapes) of parsed parameter sets that all hold one net of the box for K features on `dev`; set ``m`` is
    named ``label.format(m)`` in front of its tensor's name"""
    w1 = sets[0][0]
    if w1.dim() != 2:
        raise ValueError(f"W1 must have shape [hidden, {K}], got {tuple(w1.shape)}")
    H = int(w1.shape[0])
    if H not in HIDDEN:
        raise ValueError(f"hidden must be one of {HIDDEN}, got {H}")
    w3 = sets[0][4]
    if w3.dim() != 2:
        raise ValueError(f"W3 must have shape [out_features, {H}], got {tuple(w3.shape)}")
    O = int(w3.shape[0])
    if not 1 <= O <= MAX_OUT:
        raise ValueError(f"1 <= out_features <= {MAX_OUT}, got {O}")
    shapes = ((H, K), (H,), (H, H), (H,), (O, H), (O,))
    for m, ps in enumerate(sets):
        for name, shape, p in zip(NAMES, shapes, ps):
            if tuple(p.shape) != shape or p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError(f"{label.format(m)}{name} must be a contiguous float32 {list(shape)} tensor on {dev}, got {p.dtype} "
                                 f"{list(p.shape)} on {p.device}{'' if p.is_contiguous() else ', not contiguous'}")
    return H, O, shapes


def _outputs(out, out_dtype, keys, n, O, dev):
    """(the tensors of ``out=`` or None, their row pitch) of a forward; without ``out=``, ``out_dtype`` is checked instead"""
    if out is None:
        if out_dtype not in OUT_FORMATS:
            raise ValueError(f"out_dtype must be {' or '.join(str(d) for d in OUT_FORMATS)}, got {out_dtype}")
        return None, O
    okeys, ys = _launch.sides(out, "out")
    if okeys != keys:
        raise ValueError(f"out must name the agents of obs in their order: {keys}, got {okeys}")
    if ys[0].dtype not in OUT_FORMATS:
        raise ValueError(f"out must be {' or '.join(str(d) for d in OUT_FORMATS)}, got {ys[0].dtype}")
    return ys, _rows(ys, "out", n, O, tuple(OUT_FORMATS), dev)


def forward(obs, params, activation: str = "tanh", out=None, out_dtype=torch.float32):
    """``W3 · act(W2 · act(W1 · x + b1) + b2) + b3`` for every observation row of one or both agents, in one launch
    (``pz_mlp_forward``).

    ``obs``: ``[N, K]`` int32, int16, float32, float16 or bfloat16 -- a tensor, or an ``{agent: tensor}`` dict of one or
    two agents -- at any row stride >= K with the last dimension contiguous; an element converts to float32 inside the
    kernel.  ``params``: a sequence ``(W1, b1, W2, b2, W3, b3)`` of ``nn.Linear``'s own tensors (``W`` is ``[out, in]``),
    or an ``{agent: ...}`` dict of them; one sequence given with a two-agent ``obs`` means shared weights.  They are
    float32, contiguous and on the obs' device, and are read in place (``.data``: ``requires_grad`` is allowed, the result
    carries no graph).  ``1 <= K <= 72``, hidden in ``{32, 64, 128}``, ``1 <= O <= 40``.  ``activation``: ``"tanh"`` or
    ``"relu"``.

    Returns ``[N, O]`` of ``out_dtype`` (float32, float16 or bfloat16), or a dict of them.  ``out=`` a previous result
    (or ``[N, O]`` tensors at any common row stride) makes the call allocation-free; an output must not overlap an input
    or the other output.  The launch goes to the current stream without a synchronisation.  Shape, dtype, device and
    range errors raise ``ValueError`` before any launch."""
    keys, xs, n, K, dev, obs_pitch = _observations(obs, activation)
    sets = _parameter_sets(params, keys, len(xs))
    H, O, _ = _box(sets, K, dev)
    ys, out_pitch = _outputs(out, out_dtype, keys, n, O, dev)
    if dev.type != "cuda":
        raise ValueError(f"the policy net runs on the GPU: obs are on {dev}")
    if ys is None:
        ys = [torch.empty((n, O), dtype=out_dtype, device=dev) for _ in xs]
        out = _launch.shape(keys, ys)
    _launch.no_alias([(f"out[{s}]", y) for s, y in enumerate(ys)],
                     [(f"obs[{s}]", x) for s, x in enumerate(xs)] + [(f"{name}[{s}]", p) for s, ps in enumerate(sets) for name, p in zip(NAMES, ps)])
    if n == 0:
        return out
    second = [p.data_ptr() for p in sets[1]] if len(xs) == 2 else [None] * 6
    _launch.launch(load().pz_mlp_forward, _ERRORS, dev, *_launch.ptrs(xs), OBS_FORMATS[xs[0].dtype], n, K, obs_pitch, H, O, ACTIVATIONS[activation],
                   *[p.data_ptr() for p in sets[0]], *second, *_launch.ptrs(ys), OUT_FORMATS[ys[0].dtype], out_pitch)
    return out


class ActorCritic(torch.nn.Module):
    """The usual actor-critic trunk: three ``nn.Linear`` (``in_features -> hidden -> hidden -> num_actions + 1``), trunk and
    head shared between the policy and the value; column ``num_actions`` of the output is the value.  Orthogonal weights
    with the gains sqrt 2, sqrt 2 and 0.01, biases 0.

    ``forward(obs)`` is the torch route, differentiable.  ``act(obs)`` is :func:`forward` of this module (one launch, no
    graph): the rollout side; ``act_sample(obs, seed, step)`` is that launch and ``policy.sample`` on its logits in one
    (``act.sample``).  ``evaluate(obs)`` is the same launch made differentiable by ``netgrad.head``: the update side,
    one call forward and one call backward for both agents.  All read the same storage, so there is nothing to synchronise
    after ``optimizer.step()``."""

    def __init__(self, in_features: int = 35, hidden: int = 64, num_actions: int = 18, activation: str = "tanh"):
        super().__init__()
        if not 1 <= int(in_features) <= MAX_IN:
            raise ValueError(f"1 <= in_features <= {MAX_IN}, got {in_features}")
        if hidden not in HIDDEN:
            raise ValueError(f"hidden must be one of {HIDDEN}, got {hidden}")
        if not 1 <= int(num_actions) + 1 <= MAX_OUT:
            raise ValueError(f"0 <= num_actions <= {MAX_OUT - 1}, got {num_actions}")
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be {' or '.join(repr(a) for a in ACTIVATIONS)}, got {activation!r}")
        self.in_features, self.hidden, self.num_actions, self.activation = int(in_features), int(hidden), int(num_actions), activation
        self.fc1 = torch.nn.Linear(self.in_features, self.hidden)
        self.fc2 = torch.nn.Linear(self.hidden, self.hidden)
        self.head = torch.nn.Linear(self.hidden, self.num_actions + 1)
        for layer, gain in ((self.fc1, math.sqrt(2.0)), (self.fc2, math.sqrt(2.0)), (self.head, 0.01)):
            torch.nn.init.orthogonal_(layer.weight, gain)
            torch.nn.init.zeros_(layer.bias)

    def parameter_tensors(self):
        """``(W1, b1, W2, b2, W3, b3)``: what :func:`forward` takes as ``params``"""
        return (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.head.weight, self.head.bias)

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        f = torch.tanh if self.activation == "tanh" else torch.relu
        x = obs.to(torch.float32)
        return self.head(f(self.fc2(f(self.fc1(x)))))

    def act(self, obs, out=None, out_dtype=torch.float32):
        """the ``[N, num_actions + 1]`` head of a tensor or an ``{agent: tensor}`` dict of observations, both agents on
        this module's parameters, in one launch"""
        with torch.no_grad():
            return forward(obs, self.parameter_tensors(), self.activation, out=out, out_dtype=out_dtype)

    def act_sample(self, obs, seed: int, step=0, first_game: int = 0, head: bool = False, out=None):
        """:meth:`act` and ``policy.sample`` on its logits in ONE launch (``act.sample``, imported on first use: nothing loads
        libpikazoo_act.so before): ``{"actions", "log_probs", "entropy", "values"}`` of a tensor or an ``{agent: tensor}`` dict
        of observations, plus ``"head"`` when asked -- the bits of the two calls, from the same Philox stream"""
        from . import act

        with torch.no_grad():
            return act.sample(obs, self.parameter_tensors(), self.num_actions, seed, step=step, first_game=first_game,
                              activation=self.activation, head=head, out=out)

    def rollout(self, env, k: int, seed: int, step=0, first_game: int = 0, action_dtype=torch.int64, entropy: bool = False, out=None):
        """``k`` steps of :meth:`act_sample` and ``env.step`` in ONE launch, both agents on this module's parameters:
        ``env.unwrapped.rollout_policy(self, k, seed, ...)`` (documented there; nothing loads libpikazoo_rollout.so before)"""
        with torch.no_grad():
            return env.unwrapped.rollout_policy(self, k, seed, step=step, first_game=first_game, action_dtype=action_dtype,
                                                entropy=entropy, out=out)

    def evaluate(self, obs):
        """the ``[N, num_actions + 1]`` float32 head of a tensor or an ``{agent: tensor}`` dict of observations, as
        :meth:`act` computes it, differentiable with respect to this module's parameters: ``netgrad.head`` (imported on
        first use: nothing loads libpikazoo_netgrad.so before), whose backward is one ``netgrad.backward`` call"""
        from . import netgrad

        return netgrad.head(obs, self.parameter_tensors(), self.activation)
