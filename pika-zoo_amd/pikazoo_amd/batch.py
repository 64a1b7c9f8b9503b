"""The data movement of a PPO iteration: one policy step's records into the ``[k, n, ...]`` rollout buffers in ONE launch, and
every tensor of a shuffled minibatch out of them in ONE launch, the permutation computed inside the kernel from a counter.

    from pikazoo_amd import batch
    buf = batch.RolloutBuffer(k, n, dict(obs=obs, actions=actions, log_probs=log_probs, head=head, rewards=rewards,
                                         terminations=terminations), minibatches=4, seed=0)
    buf.store(t, obs=obs, actions=actions, log_probs=log_probs, head=head, rewards=rewards, terminations=terminations)
    buf.set_targets(learn.gae(buf.rewards, buf.values, buf.terminations))
    mb = buf.minibatch(counter=epoch * 4 + m)         # {"obs", "actions", "log_probs", "advantages", "returns"} of [B, ...]

    batch.copy([(src, dst), ...])                     # row g of every dst <- row g of its src
    batch.gather(sources, minibatches=4, seed=0, counter=c)      # the same structure of [B, ...] tensors
    batch.permutation(M, seed=0, epoch=e)             # int64[M]: the order gather visits the rows in

ctypes binding of libpikazoo_batch.so (C ABI and the definition: include/pikazoo_batch.h), a library of its own beside the
product library; nothing in the step path or in the other modules imports this one, and it imports none of them.  There is no torch fallback: a missing or
stale library raises.  A launch allocates nothing and does not synchronise: it can be captured in a graph, and a counter
given as a device tensor is read at run time.  Every tensor is a COLUMN described by bytes, so any dtype and any agent is
just another column; at most 16 columns per launch, rows of at most 512 bytes.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _launch, _native

LIB_PATH = _native.PKG_ROOT / "lib" / "libpikazoo_batch.so"
ABI_VERSION = 1
MAX_COLUMNS = 16
MAX_ROW_BYTES = 512
MAX_ROWS = 1 << 31

_P = C.c_void_p


class Column(C.Structure):
    """pz_batch_column"""
    _fields_ = [("src", _P), ("dst", _P), ("src_step_pitch", C.c_int64), ("src_game_pitch", C.c_int64), ("dst_pitch", C.c_int64),
                ("row_bytes", C.c_int32), ("elem_bytes", C.c_int32)]


SIGNATURES = {
    "pz_batch_abi_version": (C.c_int, []),
    "pz_batch_build_id": (C.c_char_p, []),
    # (cols, ncols, n, stream)
    "pz_batch_copy": (C.c_int, [C.POINTER(Column), C.c_int32, C.c_int64, _P]),
    # (cols, ncols, k, n, minibatches, seed, counter, counter_dev, index_in, index_out, errors, stream)
    "pz_batch_gather": (C.c_int, [C.POINTER(Column), C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P]),
}
_ERRORS = {**_launch.ERRORS, -2: "a count, a pitch or an extent beyond the kernel's range", -3: "an element size other than 1, 2, 4 or 8",
           -4: "a pointer, pitch or row not aligned to its element"}
_lib = None


def load():
    """Load libpikazoo_batch.so (once).  Raises if it has not been built or was built from other sources than the ones in
    this tree."""
    global _lib
    if _lib is None:
        _lib = _native.load_library(LIB_PATH, "pz_batch.hip", SIGNATURES, "pz_batch_abi_version", ABI_VERSION)
    return _lib


# ---- descriptors ---------------------------------------------------------------------------------------------------------------
def _row(t, lead, what):
    """(row_bytes, [pitch in bytes of each of the `lead` leading dimensions]) of a tensor whose trailing dimensions form one
    dense row"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dim() < lead:
        raise ValueError(f"{what} must have at least {lead} dimension{'s' if lead > 1 else ''}, got shape {list(t.shape)}")
    if t.dtype.is_complex or t.is_sparse or t.is_quantized:
        raise ValueError(f"{what}: a dense real, integer or bool tensor is needed, got {t.dtype}")
    elem = t.element_size()
    if elem not in (1, 2, 4, 8):
        raise ValueError(f"{what}: elements of 1, 2, 4 or 8 bytes, got {t.dtype}")
    width = 1
    for size, stride in zip(reversed(t.shape[lead:]), reversed(t.stride()[lead:])):
        if size != 1 and stride != width:
            raise ValueError(f"{what}: the dimensions behind the first {lead} must be contiguous (shape {list(t.shape)}, strides {list(t.stride())})")
        width *= size
    row_bytes = width * elem
    if not 1 <= row_bytes <= MAX_ROW_BYTES:
        raise ValueError(f"{what}: a row of 1..{MAX_ROW_BYTES} bytes, got {row_bytes} (shape {list(t.shape)}, {t.dtype})")
    pitches = []
    for d in range(lead):
        if t.shape[d] > 1 and t.stride(d) < width:
            raise ValueError(f"{what}: rows overlap (stride {t.stride(d)} of dimension {d} is below the row's {width} elements)")
        pitches.append(int(t.stride(d)) * elem if t.shape[d] > 1 else row_bytes)
    return row_bytes, pitches


def _leaves(x, what, path=()):
    """[(path, tensor)] of a possibly nested dict of tensors, in its order"""
    if isinstance(x, dict):
        out = []
        for key, value in x.items():
            out += _leaves(value, what, path + (key,))
        return out
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}{''.join(f'[{p!r}]' for p in path)} must be a tensor or a dict of tensors, got {type(x).__name__}")
    return [(path, x)]


def _rebuild(x, values):
    """the structure of `x` with its leaves replaced by the next items of the iterator `values`"""
    if isinstance(x, dict):
        return {key: _rebuild(value, values) for key, value in x.items()}
    return next(values)


def _name(what, path):
    return what + "".join(f"[{p!r}]" for p in path)


def _device(tensors):
    dev = tensors[0].device
    for t in tensors:
        if t.device != dev:
            raise ValueError(f"every tensor must be on one device, got {dev} and {t.device}")
    return dev


def _need_gpu(dev):
    if dev.type != "cuda":
        raise ValueError(f"the batch launches run on the GPU: the tensors are on {dev}")


# ---- copy ----------------------------------------------------------------------------------------------------------------------
def _plan_copy(pairs):
    """Every check that needs no library, then (Column array, ncols, n, device).  The structs hold addresses only."""
    if isinstance(pairs, (torch.Tensor, dict)) or not hasattr(pairs, "__len__"):
        raise ValueError(f"pairs must be a sequence of (src, dst) tensor pairs, got {type(pairs).__name__}")
    pairs = list(pairs)
    if not 1 <= len(pairs) <= MAX_COLUMNS:
        raise ValueError(f"one launch moves 1..{MAX_COLUMNS} columns, got {len(pairs)}")
    array = (Column * MAX_COLUMNS)()
    n = None
    for i, pair in enumerate(pairs):
        if isinstance(pair, torch.Tensor) or not hasattr(pair, "__len__") or len(pair) != 2:
            raise ValueError(f"pairs[{i}] must be a (src, dst) pair")
        src, dst = pair
        row_bytes, (src_pitch,) = _row(src, 1, f"pairs[{i}] src")
        dst_bytes, (dst_pitch,) = _row(dst, 1, f"pairs[{i}] dst")
        if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
            raise ValueError(f"pairs[{i}]: src is {src.dtype} {list(src.shape)}, dst is {dst.dtype} {list(dst.shape)}: a copy converts nothing")
        if n is None:
            n = int(src.shape[0])
        if src.shape[0] != n:
            raise ValueError(f"pairs[{i}] has {src.shape[0]} rows, pairs[0] has {n}")
        array[i] = Column(src.data_ptr(), dst.data_ptr(), 0, src_pitch, dst_pitch, row_bytes, src.element_size())
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^31 rows, got {n}")
    dev = _device([t for pair in pairs for t in pair])
    _launch.no_alias([(f"pairs[{i}] dst", d) for i, (_, d) in enumerate(pairs)], [(f"pairs[{i}] src", s) for i, (s, _) in enumerate(pairs)])
    _need_gpu(dev)
    return array, len(pairs), n, dev


def _launch_copy(array, ncols, n, dev):
    if n:
        _launch.launch(load().pz_batch_copy, _ERRORS, dev, array, ncols, n)


def copy(pairs):
    """Row ``g`` of every ``dst`` becomes row ``g`` of its ``src``, for all pairs in one launch (``pz_batch_copy``).

    ``pairs``: 1..16 ``(src, dst)`` pairs of ``[n, ...]`` tensors of one ``n``; a pair shares shape and dtype (nothing is
    converted).  The dimensions behind the first form one dense row of at most 512 bytes; the first dimension may have any
    stride that keeps rows apart, so ``head[:, A]`` -- the value column of an ``[n, A + 1]`` head -- is a column like any
    other.  A ``dst`` must not overlap a ``src`` or another ``dst``.  Shape, dtype, device, overlap and stride errors raise
    ``ValueError`` before any launch.  Allocates nothing and does not synchronise."""
    _launch_copy(*_plan_copy(pairs))


# ---- gather --------------------------------------------------------------------------------------------------------------------
def _int_word(t, what, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
        raise ValueError(f"{what} must be one int64 element on {dev}, got {_launch.describe(t)}")
    return t


class _GatherPlan:
    """the arguments of one pz_batch_gather, checked; it keeps its tensors alive"""

    def __init__(self, sources, minibatches, seed, counter, counter_dev, index, out, index_out, errors):
        leaves = _leaves(sources, "sources")
        if not leaves:
            raise ValueError("sources holds no tensor (batch.permutation() returns the order alone)")
        if len(leaves) > MAX_COLUMNS:
            raise ValueError(f"one launch moves at most {MAX_COLUMNS} columns, got {len(leaves)}")
        first = leaves[0][1]
        if first.dim() < 2:
            raise ValueError(f"{_name('sources', leaves[0][0])} must be [k, n, ...], got shape {list(first.shape)}")
        k, n = int(first.shape[0]), int(first.shape[1])
        dev = first.device
        self.k, self.n = k, n
        M = k * n
        rows = []
        for path, t in leaves:
            what = _name("sources", path)
            row_bytes, (step_pitch, game_pitch) = _row(t, 2, what)
            if tuple(t.shape[:2]) != (k, n):
                raise ValueError(f"{what} is {list(t.shape)}: every source is [k, n, ...] with k = {k}, n = {n}")
            rows.append((row_bytes, step_pitch, game_pitch))
        if not 1 <= M <= MAX_ROWS:
            raise ValueError(f"k * n must be in 1..2^31, got {k} x {n}")
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
                raise ValueError("index must be a contiguous one-dimensional int64 tensor")
            B = int(index.shape[0])
            self.passed, self.seed, self.counter = B, 0, 0
            counter_dev = None
        else:
            if isinstance(minibatches, bool) or not isinstance(minibatches, int) or not 1 <= minibatches <= M:
                raise ValueError(f"minibatches must be an integer in 1..{M} (k * n), got {minibatches!r}")
            if isinstance(counter, bool) or not isinstance(counter, int) or not 0 <= counter < 1 << 62:
                raise ValueError(f"counter must be an integer in [0, 2^62), got {counter!r}")
            if isinstance(seed, bool) or not isinstance(seed, int):
                raise ValueError(f"seed must be an integer, got {seed!r}")
            B = M // minibatches
            self.passed, self.seed, self.counter = minibatches, seed & 0xFFFFFFFFFFFFFFFF, counter
            if counter_dev is not None:
                _int_word(counter_dev, "counter_dev", dev)
        self.B = B
        if out is None:
            outs = [torch.empty((B, *t.shape[2:]), dtype=t.dtype, device=t.device) for _, t in leaves]
            self.result = _rebuild(sources, iter(outs))
        else:
            got = _leaves(out, "out")
            if [p for p, _ in got] != [p for p, _ in leaves]:
                raise ValueError("out must have the structure of sources (pass a previous result)")
            outs = [t for _, t in got]
            self.result = out
        array = (Column * MAX_COLUMNS)()
        for i, ((path, t), o, (row_bytes, step_pitch, game_pitch)) in enumerate(zip(leaves, outs, rows)):
            what = _name("out", path)
            out_bytes, (dst_pitch,) = _row(o, 1, what)
            if tuple(o.shape) != (B, *t.shape[2:]) or o.dtype != t.dtype:
                raise ValueError(f"{what} must be {t.dtype} {[B, *t.shape[2:]]}, got {o.dtype} {list(o.shape)}")
            array[i] = Column(t.data_ptr(), o.data_ptr(), step_pitch, game_pitch, dst_pitch, row_bytes, t.element_size())
        if index_out is not None:
            if (not isinstance(index_out, torch.Tensor) or index_out.dtype != torch.int64 or tuple(index_out.shape) != (B,)
                    or not index_out.is_contiguous()):
                raise ValueError(f"index_out must be a contiguous int64 tensor of {B} elements")
        if errors is not None:
            if not isinstance(errors, torch.Tensor) or errors.dtype != torch.int32 or errors.numel() != 1:
                raise ValueError("errors must be one int32 element")
        extras = [(name, t) for name, t in (("counter_dev", counter_dev), ("index", index), ("index_out", index_out), ("errors", errors))
                  if t is not None]
        dev = _device([t for _, t in leaves] + outs + [t for _, t in extras])
        outputs = [(_name("out", p), o) for (p, _), o in zip(leaves, outs)] + [(name, t) for name, t in extras if name in ("index_out", "errors")]
        inputs = [(_name("sources", p), t) for p, t in leaves] + [(name, t) for name, t in extras if name in ("counter_dev", "index")]
        _launch.no_alias(outputs, inputs)
        _need_gpu(dev)
        self.array, self.ncols, self.dev = array, len(leaves), dev
        self.pointers = tuple(t.data_ptr() if t is not None else None for t in (counter_dev, index, index_out, errors))
        self._alive = (leaves, outs, extras)

    def launch(self, counter=None):
        _launch.launch(load().pz_batch_gather, _ERRORS, self.dev, self.array, self.ncols, self.k, self.n, self.passed, self.seed,
                       self.counter if counter is None else counter, *self.pointers)
        return self.result


def gather(sources, minibatches, seed, counter=0, counter_dev=None, index=None, out=None, index_out=None, errors=None):
    """Minibatch ``m`` of epoch ``E`` of every source, in one launch (``pz_batch_gather``; the definition is
    include/pikazoo_batch.h's): with ``M = k * n``, ``B = M // minibatches`` and ``C = counter + counter_dev[0]``, ``E = C //
    minibatches`` and ``m = C % minibatches``, output row ``j`` is flat source row ``permutation(M, seed, E)[m * B + j]``.

    ``sources``: a (possibly nested) dict of 1..16 ``[k, n, ...]`` tensors of one ``k`` and ``n``, any dtypes; the dimensions
    behind the first two form one dense row of at most 512 bytes, the first two may have any strides that keep rows apart.
    Returns the same structure of ``[B, ...]`` tensors; with ``out=`` a previous result nothing is allocated.  ``counter_dev``:
    an int64 device tensor of one element that the kernel reads when it runs (increment it between replays of a captured
    graph).  ``index``: an int64 device tensor ``[B]`` of flat rows that replaces the permutation (``minibatches``, ``seed``
    and the counters are then ignored); a row outside ``[0, M)`` is delivered as zeros and sets ``errors`` (an int32 device
    tensor of one element) to 1.  ``index_out``: an int64 ``[B]`` tensor that receives the source row of every output row.
    Shape, dtype, device, overlap, stride and range errors raise ``ValueError`` before any launch."""
    return _GatherPlan(sources, minibatches, seed, counter, counter_dev, index, out, index_out, errors).launch()


def permutation(M, seed, epoch, device=None):
    """``int64[M]``: the order in which epoch ``epoch`` of :func:`gather` visits ``M`` flat rows under ``seed``"""
    if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= MAX_ROWS:
        raise ValueError(f"M must be an integer in 1..2^31, got {M!r}")
    if isinstance(epoch, bool) or not isinstance(epoch, int) or not 0 <= epoch < 1 << 62:
        raise ValueError(f"epoch must be an integer in [0, 2^62), got {epoch!r}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _need_gpu(dev)
    out = torch.empty(M, dtype=torch.int64, device=dev)
    _launch.launch(load().pz_batch_gather, _ERRORS, dev, None, 0, 1, M, 1, seed & 0xFFFFFFFFFFFFFFFF, epoch, None, None, out.data_ptr(), None)
    return out


# ---- the rollout buffer --------------------------------------------------------------------------------------------------------
_FIELDS = ("obs", "actions", "log_probs", "head", "rewards", "terminations")


def _identity(x):
    """what a cached plan depends on in a tensor: where it lies and how it is laid out (a plan's checks ran on exactly this);
    anything that is no tensor is its own identity, so that the plan is made, and refused, again"""
    return (x.data_ptr(), tuple(x.shape), x.stride(), x.dtype, x.device) if isinstance(x, torch.Tensor) else ("not a tensor", id(x))


class RolloutBuffer:
    """The ``[k, n, ...]`` buffers of a two-agent rollout and their two launches.

    ``example_step``: one step's tensors, from which the buffers take shapes, dtypes and the device --
    ``obs`` ``{agent: [n, K]}``, ``actions`` ``{agent: [n]}``, ``log_probs`` ``{agent: [n]}``, ``head`` ``{agent: [n, A + 1]}``
    (logits and, in its last column, the value), ``rewards`` ``{agent: [n]}`` in the env's dtype (``learn.gae`` reads it as it
    is) and ``terminations`` ``[n]`` (or an ``{agent: [n]}`` dict, whose first entry is taken).  ``rewards`` and
    ``terminations`` may be left out: their buffers are then allocated by the first :meth:`store` that brings them (the first
    policy step of a rollout has seen no ``env.step`` yet).

    Buffers: ``obs``, ``actions``, ``log_probs``, ``rewards`` ``{agent: [k, n, ...]}``, ``values`` ``{agent: [k + 1, n]}`` and
    ``terminations`` ``[k, n]``."""

    def __init__(self, k, n, example_step, minibatches=4, seed=0):
        if not isinstance(example_step, dict) or not set(_FIELDS[:4]) <= set(example_step) <= set(_FIELDS):
            raise ValueError(f"example_step must hold {_FIELDS}, got {sorted(example_step) if isinstance(example_step, dict) else type(example_step).__name__}")
        if k < 1 or n < 1 or k * n > MAX_ROWS:
            raise ValueError(f"k >= 1, n >= 1 and k * n <= 2^31 are needed, got k = {k}, n = {n}")
        self.k, self.n, self.minibatches, self.seed = int(k), int(n), minibatches, seed
        self.agents = list(example_step["obs"])
        for name in ("actions", "log_probs", "head", "rewards"):
            if name not in example_step:
                continue
            if not isinstance(example_step[name], dict) or list(example_step[name]) != self.agents:
                raise ValueError(f"example_step[{name!r}] must be a dict over {self.agents}")
        for name in example_step:
            for path, t in _leaves(example_step[name], f"example_step[{name!r}]"):
                if t.dim() < 1 or t.shape[0] != n:
                    raise ValueError(f"{_name(f'example_step[{name!r}]', path)} must be [n = {n}, ...], got {list(t.shape)}")
        ex = example_step
        like = self._like
        self.obs = {a: like(ex["obs"][a], k) for a in self.agents}
        self.actions = {a: like(ex["actions"][a], k) for a in self.agents}
        self.log_probs = {a: like(ex["log_probs"][a], k) for a in self.agents}
        self.values = {a: like(ex["head"][a], k + 1, ()) for a in self.agents}
        self.rewards = {a: like(ex["rewards"][a], k) for a in self.agents} if "rewards" in ex else None
        self.terminations = like(self._flags(ex["terminations"]), k) if "terminations" in ex else None
        self.targets = None
        self._stores, self._gathers = {}, {}

    def _like(self, t, rows, tail=None):
        return torch.empty((rows, self.n, *(t.shape[1:] if tail is None else tail)), dtype=t.dtype, device=t.device)

    def _flags(self, terminations):
        return terminations[self.agents[0]] if isinstance(terminations, dict) else terminations

    def store(self, t, obs=None, actions=None, log_probs=None, head=None, rewards=None, terminations=None):
        """File one policy step in ONE ``pz_batch_copy``.  ``obs``, ``actions``, ``log_probs`` and the value column of ``head``
        are those of policy step ``t`` and go to row ``t`` (``head`` alone also to row ``k``: the bootstrap value).  ``rewards``
        and ``terminations`` are what the env returned TOGETHER WITH these observations -- the outcome of step ``t - 1`` -- and
        go to row ``t - 1``; they are not given at ``t == 0``.  So a rollout of ``k`` steps is ``k + 1`` calls, one per
        ``ActorCritic.act``, each in front of the ``env.step`` that overwrites its inputs.  Every argument is optional."""
        given = (obs, actions, log_probs, head, rewards, terminations)
        key = (t,) + tuple(_identity(x) for field in given if field is not None
                           for x in (field.values() if isinstance(field, dict) else (field,)))
        plan = self._stores.get(key)
        if plan is None:
            if len(self._stores) > 4 * (self.k + 1):
                self._stores.clear()
            plan = self._stores[key] = self._plan_store(t, *given)
        _launch_copy(*plan[:4])

    def _plan_store(self, t, obs, actions, log_probs, head, rewards, terminations):
        k = self.k
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= k:
            raise ValueError(f"t must be an integer in 0..{k}, got {t!r}")
        if rewards is not None and self.rewards is None and isinstance(rewards, dict) and list(rewards) == self.agents:
            for a in self.agents:
                if not isinstance(rewards[a], torch.Tensor) or tuple(rewards[a].shape) != (self.n,):
                    raise ValueError(f"rewards[{a!r}] must be [{self.n}]")
            self.rewards = {a: self._like(rewards[a], k) for a in self.agents}
        if terminations is not None and self.terminations is None:
            flags = self._flags(terminations)
            if not isinstance(flags, torch.Tensor) or tuple(flags.shape) != (self.n,):
                raise ValueError(f"terminations must be [{self.n}]")
            self.terminations = self._like(flags, k)
        pairs = []
        for name, field, buf, row, last in (("obs", obs, self.obs, t, k - 1), ("actions", actions, self.actions, t, k - 1),
                                            ("log_probs", log_probs, self.log_probs, t, k - 1), ("head", head, self.values, t, k),
                                            ("rewards", rewards, self.rewards, t - 1, k - 1)):
            if field is None:
                continue
            if not isinstance(field, dict) or list(field) != self.agents:
                raise ValueError(f"{name} must be a dict over {self.agents}")
            if not 0 <= row <= last:
                raise ValueError(f"{name} at t = {t}: its row {row} is outside 0..{last}")
            for a in self.agents:
                x = field[a]
                if name == "head":
                    if not isinstance(x, torch.Tensor) or x.dim() != 2:
                        raise ValueError(f"head[{a!r}] must be [n, A + 1]")
                    x = x[:, x.shape[1] - 1]
                pairs.append((x, buf[a][row]))
        if terminations is not None:
            if not 1 <= t <= k:
                raise ValueError(f"terminations at t = {t}: its row {t - 1} is outside 0..{k - 1}")
            pairs.append((self._flags(terminations), self.terminations[t - 1]))
        if not pairs:
            raise ValueError("store() needs at least one tensor")
        return (*_plan_copy(pairs), pairs)

    def set_targets(self, targets):
        """Register what ``learn.gae`` returned (``{"advantages": {agent: [k, n]}, "returns": {agent: [k, n]}}``) as the last
        two tensors of a minibatch."""
        for name in ("advantages", "returns"):
            if not isinstance(targets, dict) or name not in targets or list(targets[name]) != self.agents:
                raise ValueError(f"targets must hold 'advantages' and 'returns' as dicts over {self.agents}")
            for a in self.agents:
                if tuple(targets[name][a].shape[:2]) != (self.k, self.n):
                    raise ValueError(f"targets[{name!r}][{a!r}] must be [{self.k}, {self.n}], got {list(targets[name][a].shape)}")
        self.targets = {name: dict(targets[name]) for name in ("advantages", "returns")}

    def sources(self):
        """what a minibatch is drawn from: ``{"obs", "actions", "log_probs", "advantages", "returns"}`` of ``{agent: [k, n, ...]}``"""
        if self.targets is None:
            raise ValueError("set_targets() first: a minibatch holds the advantages and returns of learn.gae")
        return {"obs": self.obs, "actions": self.actions, "log_probs": self.log_probs, "advantages": self.targets["advantages"],
                "returns": self.targets["returns"]}

    def minibatch(self, counter=0, counter_dev=None, out=None):
        """Minibatch ``counter % minibatches`` of epoch ``counter // minibatches`` in ONE ``pz_batch_gather``: everything
        ``ActorCritic.evaluate`` and ``ppo.loss`` take, as ``{"obs", "actions", "log_probs", "advantages", "returns"}`` of
        ``{agent: [B, ...]}``.  ``out=`` a previous result: nothing is allocated.  ``counter_dev`` as in :func:`gather`."""
        sources = self.sources()
        key = tuple(_identity(t) for _, t in _leaves(sources, "sources")) + (
            tuple(_identity(t) for _, t in _leaves(out, "out")) if out is not None else None, _identity(counter_dev) if counter_dev is not None else None)
        plan = self._gathers.get(key) if out is not None else None
        if plan is None:
            plan = _GatherPlan(sources, self.minibatches, self.seed, counter, counter_dev, None, out, None, None)
            if out is not None:
                if len(self._gathers) > 8:
                    self._gathers.clear()
                self._gathers[key] = plan
        elif isinstance(counter, bool) or not isinstance(counter, int) or not 0 <= counter < 1 << 62:
            raise ValueError(f"counter must be an integer in [0, 2^62), got {counter!r}")
        return plan.launch(counter)
