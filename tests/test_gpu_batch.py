"""GPU tests of the batch library (include/pikazoo_batch.h) against tests/batch_judge.py, bit for bit: a copy has no tolerance.
Every case runs through the C ABI and through ``pikazoo_amd.batch`` on the same bytes; every destination and ``index_out`` is
a view between sentinel guards, the gaps between ``row_bytes`` and ``dst_pitch`` included; sources keep their bits; the
sources are random bytes, so NaN payloads of every float width pass through.  The shapes are small: each is the smallest at
which something can go wrong (tests/batch_judge.py: basic_shapes, VARIETY)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import batch_judge as J

REPO = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = 0xA5
DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SEED = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def batch():
    from pikazoo_amd import batch

    batch.load()
    return batch


def on_device(array):
    pad = (-len(array)) % 8
    return torch.from_numpy(np.concatenate([array, np.zeros(pad, np.uint8)])).cuda()


def guarded(nbytes):
    total = GUARD + nbytes + GUARD
    return torch.full((total + (-total) % 8,), SENTINEL, dtype=torch.uint8, device="cuda")


class Case:
    """one column on the device: its source allocation, its guarded destination, and both routes' views of them"""

    def __init__(self, case, k, n, B, seed, copy=False):
        self.c = c = J.sized(case, 1 if copy else k, n)
        self.B, self.n, self.copy = B, n, copy
        self.source = J.make_source(c, seed)
        self.src = on_device(self.source)
        self.dst = guarded(c["dst_offset"] + ((B - 1) * c["dst_pitch"] + c["row_bytes"] if B else 0))

    def column(self, batch):
        c = self.c
        return batch.Column(self.src.data_ptr() + c["src_offset"], self.dst.data_ptr() + GUARD + c["dst_offset"], c["step_pitch"], c["game_pitch"],
                            c["dst_pitch"], c["row_bytes"], c["elem_bytes"])

    def views(self, k):
        """(source, destination) as typed strided tensors over the same bytes"""
        c, e = self.c, self.c["elem_bytes"]
        width = c["row_bytes"] // e
        src = self.src.view(DTYPES[e])
        dst = self.dst.view(DTYPES[e]).as_strided((self.B, width), (c["dst_pitch"] // e, 1), (GUARD + c["dst_offset"]) // e)
        if self.copy:
            return src.as_strided((self.n, width), (c["game_pitch"] // e, 1), c["src_offset"] // e), dst
        return src.as_strided((k, self.n, width), (c["step_pitch"] // e, c["game_pitch"] // e, 1), c["src_offset"] // e), dst

    def check(self, want_rows, what):
        c = self.c
        want = np.full(self.dst.numel(), SENTINEL, dtype=np.uint8)
        at = GUARD + c["dst_offset"] + np.arange(self.B, dtype=np.int64)[:, None] * c["dst_pitch"] + np.arange(c["row_bytes"], dtype=np.int64)[None, :]
        want[at] = want_rows
        got = self.dst.cpu().numpy()
        assert np.array_equal(got, want), (what, c, int(np.flatnonzero(got != want)[0]) - GUARD - c["dst_offset"])
        assert np.array_equal(self.src.cpu().numpy()[:len(self.source)], self.source), (what, "the source changed")
        self.dst.fill_(SENTINEL)


def run_gather(batch, cases, k, n, mb, counter, want_rows, seed=SEED, route="abi", counter_dev=None, index=None, errors=None):
    """one call on `cases` through one route; checks every destination and index_out against `want_rows`"""
    B = len(want_rows)
    index_out = guarded(B * 8)
    iv = index_out.view(torch.int64)[GUARD // 8:GUARD // 8 + B]
    if route == "abi":
        array = (batch.Column * 16)(*[x.column(batch) for x in cases])
        code = batch.load().pz_batch_gather(array, len(cases), k, n, B if index is not None else mb, seed, counter,
                                            counter_dev.data_ptr() if counter_dev is not None else None, index.data_ptr() if index is not None else None,
                                            iv.data_ptr(), errors.data_ptr() if errors is not None else None, None)
        assert code == 0
    else:
        views = [x.views(k) for x in cases]
        out = batch.gather({i: s for i, (s, _) in enumerate(views)}, mb, seed, counter=counter, counter_dev=counter_dev, index=index,
                           out={i: d for i, (_, d) in enumerate(views)}, index_out=iv, errors=errors)
        assert all(out[i] is d for i, (_, d) in enumerate(views))
    torch.cuda.synchronize()
    what = (k, n, mb, counter, route)
    got = index_out.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + 8 * B:] == SENTINEL).all(), what
    assert np.array_equal(got[GUARD:GUARD + 8 * B].view(np.int64), want_rows), what
    for x in cases:
        x.check(J.gather_bytes(x.source, x.c, n, want_rows), what)


def test_basic_shapes(batch):
    """n in {1, 63, 64, 65, 241} x k in {1, 2, 17} x minibatches in {1, 3, 4, M}, at the first and last minibatch of an epoch,
    the next epoch and a far one: four kinds of column and index_out, both routes"""
    for k, n, mb in J.basic_shapes():
        B = k * n // mb
        cases = [Case(c, k, n, B, seed=100 + i) for i, c in enumerate(J.SIMPLE)]
        for i, counter in enumerate(J.counters(mb)):
            run_gather(batch, cases, k, n, mb, counter, J.minibatch_rows(k * n, mb, SEED, counter), route="abi" if i % 2 == 0 else "binding")
        run_gather(batch, cases, k, n, mb, 1, J.minibatch_rows(k * n, mb, SEED, 1), route="binding")
        run_gather(batch, cases, k, n, mb, 1, J.minibatch_rows(k * n, mb, SEED, 1), route="abi")


@pytest.mark.parametrize("k,n,mb", [(2, 65, 3), (17, 241, 4), (1, 64, 1), (3, 300, 2)])
def test_column_variety_in_one_gather(batch, k, n, mb):
    """sixteen columns of every kind in one call -- rows of 1, 2, 4, 8, 70, 76, 140, 288 and 512 bytes, the value column of a
    head, pitches above the row on both sides, mixed-offset bases -- then a single column, then none (index_out alone)"""
    B = k * n // mb
    cases = [Case(c, k, n, B, seed=200 + i) for i, c in enumerate(J.VARIETY)]
    for route in ("abi", "binding"):
        for counter in (0, mb + mb // 2):
            rows = J.minibatch_rows(k * n, mb, SEED, counter)
            run_gather(batch, cases, k, n, mb, counter, rows, route=route)
        run_gather(batch, cases[6:7], k, n, mb, 2, J.minibatch_rows(k * n, mb, SEED, 2), route=route)
    run_gather(batch, [], k, n, mb, 5, J.minibatch_rows(k * n, mb, SEED, 5), route="abi")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 241, 300, 1025])
def test_copy_of_every_kind_of_column(batch, n):
    cases = [Case(c, 1, n, n, seed=300 + i, copy=True) for i, c in enumerate(J.VARIETY)]
    for route in ("abi", "binding"):
        for part in (cases, cases[:11], cases[4:5]):
            if route == "abi":
                array = (batch.Column * 16)(*[x.column(batch) for x in part])
                for col in array:
                    col.src_step_pitch = -12345          # ignored by pz_batch_copy
                assert batch.load().pz_batch_copy(array, len(part), n, None) == 0
            else:
                batch.copy([x.views(1) for x in part])
            torch.cuda.synchronize()
            for x in part:
                x.check(J.copy_bytes(x.source, x.c, n), (n, route, len(part)))


def test_large_permutations_without_columns(batch):
    """index_out alone: one whole epoch at M = 2^21 + 7 against the judge (through batch.permutation and through the C ABI in
    three minibatches), and the first, a middle and the last minibatch of M = 2^31 with 2^20 minibatches"""
    M = (1 << 21) + 7
    want = J.perm(np.arange(M), M, SEED, 3)
    assert np.array_equal(batch.permutation(M, SEED, 3).cpu().numpy(), want)
    for m in range(3):
        run_gather(batch, [], 1, M, 3, 3 * 3 + m, want[m * (M // 3):(m + 1) * (M // 3)])
    M, mb = 1 << 31, 1 << 20
    for m in (0, 777_777, mb - 1):
        rows = J.minibatch_rows(M, mb, SEED, 5 * mb + m)
        assert len(rows) == 2048 and rows.max() < M
        run_gather(batch, [], 1 << 11, 1 << 20, mb, 5 * mb + m, rows)


def test_a_step_pitch_beyond_32_bits(batch):
    """k = 3 steps that lie 2^32 + 64 bytes apart inside one large allocation (only the rows the gather reads are written):
    the column's offsets need 64 bits; beside it a column that does not"""
    k, n, width = 3, 65, 35
    pitch = (1 << 32) + 64
    big = torch.empty(2 * pitch + n * width * 4 + 64, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(9)
    steps = [rng.integers(0, 256, size=n * width * 4, dtype=np.uint8) for _ in range(k)]
    for t in range(k):
        big[16 + t * pitch:16 + t * pitch + n * width * 4] = torch.from_numpy(steps[t]).cuda()
    src = big.view(torch.int32).as_strided((k, n, width), (pitch // 4, width, 1), 4)
    small = Case(J.SIMPLE[0], k, n, k * n, seed=5)
    rows = J.minibatch_rows(k * n, 1, SEED, 2)
    want = np.stack([steps[r // n][(r % n) * width * 4:(r % n + 1) * width * 4] for r in rows])
    # the binding
    dst = guarded(k * n * width * 4)
    view = dst.view(torch.int32)[GUARD // 4:GUARD // 4 + k * n * width].view(k * n, width)
    batch.gather({"wide": src, "small": small.views(k)[0]}, 1, SEED, counter=2, out={"wide": view, "small": small.views(k)[1]})
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + want.size].reshape(want.shape), want)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + want.size:] == SENTINEL).all()
    small.check(J.gather_bytes(small.source, small.c, n, rows), "beside the wide column")
    # the C ABI
    dst.fill_(SENTINEL)
    array = (batch.Column * 16)(batch.Column(big.data_ptr() + 16, dst.data_ptr() + GUARD, pitch, width * 4, width * 4, width * 4, 4), small.column(batch))
    assert batch.load().pz_batch_gather(array, 2, k, n, 1, SEED, 2, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + want.size].reshape(want.shape), want) and (got[GUARD + want.size:] == SENTINEL).all()
    small.check(J.gather_bytes(small.source, small.c, n, rows), "beside the wide column")
    for t in range(k):
        assert np.array_equal(big[16 + t * pitch:16 + t * pitch + n * width * 4].cpu().numpy(), steps[t])


def test_a_callers_index(batch):
    """index_in: duplicates and the last row; then one index of -1 and one of M -- those rows are zeros, errors is 1, every
    other row exact, the guards intact"""
    k, n = 5, 67
    M = k * n
    rng = np.random.default_rng(4)
    good = rng.integers(0, M, size=301).astype(np.int64)
    good[:4] = (M - 1, 0, M - 1, M - 1)
    bad = good.copy()
    bad[17], bad[256] = -1, M
    for rows, flag in ((good, 0), (bad, 1)):
        cases = [Case(c, k, n, len(rows), seed=400 + i) for i, c in enumerate(J.VARIETY[:9])]
        for route in ("abi", "binding"):
            errors = torch.zeros(1, dtype=torch.int32, device="cuda")
            run_gather(batch, cases, k, n, 999, 1 << 63, rows, route=route, index=torch.from_numpy(rows).cuda(), errors=errors)
            assert int(errors.item()) == flag
    # without `errors` a bad index is still never read
    cases = [Case(J.SIMPLE[1], k, n, len(bad), seed=1)]
    run_gather(batch, cases, k, n, 0, 0, bad, index=torch.from_numpy(bad).cuda())


def test_counters_capture_and_reuse(batch):
    k, n, mb = 4, 65, 4
    M, B = k * n, k * n // mb
    cases = [Case(c, k, n, B, seed=500 + i) for i, c in enumerate(J.SIMPLE)]
    # a count by value equals the same count in the device word, and their sum is what counts
    for by_value, on_device_word in ((6, 0), (0, 6), (2, 4)):
        word = torch.tensor([on_device_word], dtype=torch.int64, device="cuda")
        for route in ("abi", "binding"):
            run_gather(batch, cases, k, n, mb, by_value, J.minibatch_rows(M, mb, SEED, 6), route=route, counter_dev=word)
    # a captured graph: the gather and the increment of the device word, replayed three times across an epoch boundary
    sources = {"a": torch.randn(k, n, 35, device="cuda"), "b": {"x": torch.randint(0, 9, (k, n), device="cuda")}}
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = batch.gather(sources, mb, SEED, counter=3, counter_dev=word)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = batch.gather(sources, mb, SEED, counter=3, counter_dev=word, out=out)
    assert torch.cuda.memory_allocated() == before and again is out             # out= reuse allocates nothing
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.gather(sources, mb, SEED, counter=3, counter_dev=word, out=out)
        word.add_(1)
    flat = {"a": sources["a"].reshape(M, 35).cpu().numpy(), "x": sources["b"]["x"].reshape(M).cpu().numpy()}
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        rows = J.minibatch_rows(M, mb, SEED, 3 + replay)                          # C = 3 (epoch 0), 4 and 5 (epoch 1)
        assert np.array_equal(out["a"].cpu().numpy().view(np.int32), flat["a"][rows].view(np.int32)), replay
        assert np.array_equal(out["b"]["x"].cpu().numpy(), flat["x"][rows]), replay
    assert int(word.item()) == 3


def test_return_codes_and_value_errors_on_device_tensors(batch):
    """every return code on real tensors, and nothing is written by a refused call; the binding's ValueErrors that need a
    device"""
    k, n = 2, 64
    x = Case(J.SIMPLE[1], k, n, 32, seed=7)
    lib = batch.load()

    def call(ncols=1, kk=k, mb=4, index_out=None, **fields):
        array = (batch.Column * 16)(*[x.column(batch)] * 16)
        for field, value in fields.items():
            setattr(array[0], field, value)
        return lib.pz_batch_gather(array, ncols, kk, n, mb, SEED, 0, None, None, index_out, None, None)

    assert call(src=None) == -1 and call(ncols=0) == -1
    assert call(ncols=17) == -2 and call(kk=0) == -2 and call(mb=0) == -2 and call(mb=k * n + 1) == -2 and call(row_bytes=516) == -2
    assert call(dst_pitch=136) == -2
    assert call(elem_bytes=3) == -3
    assert call(elem_bytes=8) == -4 and call(src=x.src.data_ptr() + 2) == -4 and call(index_out=x.dst.data_ptr() + 4) == -4
    array = (batch.Column * 16)(x.column(batch))
    assert lib.pz_batch_copy(array, 0, n, None) == -1 and lib.pz_batch_copy(array, 1, -1, None) == -2
    torch.cuda.synchronize()
    assert (x.dst == SENTINEL).all()
    assert call() == 0                                                            # (and the good call is good)
    torch.cuda.synchronize()
    x.check(J.gather_bytes(x.source, x.c, n, J.minibatch_rows(k * n, 4, SEED, 0)), "the good call")
    src, dst = torch.zeros(k, n, 35, device="cuda"), torch.zeros(32, 35, device="cuda")
    for bad in (dict(sources={"x": src, "y": torch.zeros(k, n)}), dict(out={"x": dst.cpu()}), dict(counter_dev=torch.zeros(1, dtype=torch.int64)),
                dict(index=torch.zeros(32, dtype=torch.int64)), dict(out={"x": src[0, :32]}), dict(out={"x": torch.zeros(32, 70, device="cuda")[:, ::2]}),
                dict(out={"x": torch.zeros(32, 35, dtype=torch.float64, device="cuda")}), dict(minibatches=k * n + 1)):
        with pytest.raises(ValueError):
            batch.gather(**{**dict(sources={"x": src}, minibatches=4, seed=0, out={"x": dst}), **bad})
    with pytest.raises(ValueError):
        batch.copy([(src[0], src[0])])
    with pytest.raises(ValueError):
        batch.copy([(src[0], dst.cpu())])
    with pytest.raises(ValueError):
        batch.copy([(torch.zeros(n, 129, device="cuda"), torch.zeros(n, 129, device="cuda"))])


@pytest.fixture(scope="module")
def rollout(batch):
    """k policy steps of a real env filed twice: by the eleven copy_ calls of the example, and by RolloutBuffer.store"""
    from pikazoo_amd import learn, net, pikazoo_v0, policy
    from pikazoo_amd.wrappers import NormalizeObservation

    n, k, seed = 256, 5, 3
    torch.manual_seed(seed)
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device="cuda:0", seed=seed, validate_actions=False))
    agents = env.agents
    A = env.action_space(agents[0]).n
    obs, _ = env.reset()
    K = obs[agents[0]].shape[1]
    model = net.ActorCritic(in_features=K, hidden=64, num_actions=A).to("cuda:0")
    hand = dict(obs={a: torch.empty((k, n, K), dtype=obs[a].dtype, device="cuda") for a in agents},
                actions={a: torch.empty((k, n), dtype=torch.int64, device="cuda") for a in agents},
                log_probs={a: torch.empty((k, n), dtype=torch.float32, device="cuda") for a in agents},
                values={a: torch.empty((k + 1, n), dtype=torch.float32, device="cuda") for a in agents},
                rewards={a: torch.empty((k, n), dtype=torch.float32, device="cuda") for a in agents},
                terminations=torch.empty((k, n), dtype=torch.bool, device="cuda"))
    buf = head = picked = rewards = terminations = None
    for t in range(k):
        head = model.act(obs, out=head)
        picked = policy.sample({a: head[a][:, :A] for a in agents}, seed=seed, step=t, out=picked)
        if buf is None:
            buf = batch.RolloutBuffer(k, n, dict(obs=obs, actions=picked["actions"], log_probs=picked["log_probs"], head=head), minibatches=3, seed=seed)
        buf.store(t, obs=obs, actions=picked["actions"], log_probs=picked["log_probs"], head=head, rewards=rewards if t else None,
                  terminations=terminations if t else None)
        for a in agents:
            hand["obs"][a][t].copy_(obs[a])
            hand["actions"][a][t].copy_(picked["actions"][a])
            hand["log_probs"][a][t].copy_(picked["log_probs"][a])
            hand["values"][a][t].copy_(head[a][:, A])
        obs, rewards, terminations, _, _ = env.step(picked["actions"])
        for a in agents:
            hand["rewards"][a][t].copy_(rewards[a])
        hand["terminations"][t].copy_(terminations[agents[0]])
    head = model.act(obs, out=head)
    buf.store(k, head=head, rewards=rewards, terminations=terminations)
    for a in agents:
        hand["values"][a][k].copy_(head[a][:, A])
    targets = learn.gae(buf.rewards, buf.values, buf.terminations, gamma=0.99, lam=0.95)
    buf.set_targets(targets)
    torch.cuda.synchronize()
    return buf, hand, agents, targets


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy() if t.dtype != torch.bool else t.cpu().numpy()


def test_rollout_buffer_store_equals_the_eleven_copies(rollout):
    buf, hand, agents, _ = rollout
    for a in agents:
        for name in ("obs", "actions", "log_probs", "values"):
            got, want = getattr(buf, name)[a], hand[name][a]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want)), (name, a)
        assert buf.rewards[a].shape == hand["rewards"][a].shape and np.array_equal(bits(buf.rewards[a].to(torch.float32)), bits(hand["rewards"][a])), a
    assert buf.terminations.dtype == torch.bool and np.array_equal(bits(buf.terminations), bits(hand["terminations"]))
    assert float(hand["log_probs"][agents[0]].abs().sum()) > 0 and float(hand["obs"][agents[0]].abs().sum()) > 0


def test_rollout_buffer_minibatch_equals_indexing_by_the_permutation(batch, rollout):
    buf, hand, agents, targets = rollout
    k, n, mb = buf.k, buf.n, buf.minibatches
    M, B = k * n, k * n // mb
    sources = {"obs": hand["obs"], "actions": hand["actions"], "log_probs": hand["log_probs"], "advantages": targets["advantages"],
               "returns": targets["returns"]}
    out = None
    for counter in (0, 2, 4):
        epoch, m = divmod(counter, mb)
        order = batch.permutation(M, buf.seed, epoch)
        assert np.array_equal(order.cpu().numpy(), J.perm(np.arange(M), M, buf.seed, epoch))
        idx = order[m * B:(m + 1) * B]
        out = buf.minibatch(counter=counter, out=out)
        assert sorted(out) == sorted(sources)
        for name, d in sources.items():
            for a in agents:
                want = d[a][:k].reshape(M, *d[a].shape[2:])[idx]
                assert out[name][a].shape == want.shape and out[name][a].dtype == want.dtype and np.array_equal(bits(out[name][a]), bits(want)), (name, a)
    word = torch.tensor([2], dtype=torch.int64, device="cuda")
    other = buf.minibatch(counter=2, counter_dev=word)
    assert all(np.array_equal(bits(other[name][a]), bits(out[name][a])) for name in sources for a in agents)


def test_the_example_runs_on_both_batch_routes():
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    logs = [ppo_selfplay.main(num_envs=256, iters=2, steps=8, native_batch=flag, log=lambda line: None) for flag in (True, False)]
    for log in logs:
        assert len(log) == len(logs[0]) == 2 * 2 * 4 and all(np.isfinite(entry) for entry in log)


def test_a_cached_plan_is_not_reused_for_another_shape(batch):
    """a view of the same storage with the same strides but fewer rows is checked again, not served from the plan cache"""
    n, k, agents = 8, 3, ("p1", "p2")
    step = dict(obs={a: torch.rand(n, 35, device="cuda") for a in agents}, actions={a: torch.zeros(n, dtype=torch.int64, device="cuda") for a in agents},
                log_probs={a: torch.rand(n, device="cuda") for a in agents}, head={a: torch.rand(n, 19, device="cuda") for a in agents},
                rewards={a: torch.rand(n, device="cuda") for a in agents}, terminations={a: torch.zeros(n, dtype=torch.bool, device="cuda") for a in agents})
    buf = batch.RolloutBuffer(k, n, step, minibatches=2, seed=1)
    buf.store(1, **step)
    buf.store(1, **step)                                                          # (the cached plan)
    shorter = {name: {a: t[:4] for a, t in field.items()} for name, field in step.items()}
    assert all(shorter[name][a].data_ptr() == step[name][a].data_ptr() and shorter[name][a].stride() == step[name][a].stride()
               for name in step for a in agents)
    with pytest.raises(ValueError):
        buf.store(1, **shorter)
    buf.set_targets({name: {a: torch.rand(k, n, device="cuda") for a in agents} for name in ("advantages", "returns")})
    out = buf.minibatch(counter=0)
    assert buf.minibatch(counter=1, out=out) is out and buf.minibatch(counter=2, out=out) is out
    cut = {name: {a: t[:4] for a, t in d.items()} for name, d in out.items()}
    with pytest.raises(ValueError):
        buf.minibatch(counter=3, out=cut)
    torch.cuda.synchronize()
    assert torch.equal(buf.obs["p1"][1], step["obs"]["p1"]) and torch.equal(buf.rewards["p2"][0], step["rewards"]["p2"])
