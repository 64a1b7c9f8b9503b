"""GPU tests (``-m gpu``) of the policy-head launches (include/pikazoo_policy.h: ``pz_sample_actions``,
``pz_action_log_probs``, ``pz_action_log_probs_backward``) and of ``pikazoo_amd.policy`` / ``raw_env.sample_actions``.

The judge is tests/policy_judge.py: the header's definition in numpy float64, with DERIVED tolerances and a derived
ambiguity width (held to a second formulation, central differences, a float32 restatement and mutants by
tests/test_policy_host.py).  No GPU result is ever an expected value: an unambiguous row must return exactly the judge's
action, an ambiguous one a live action between its two neighbours; log-prob and entropy are judged AT the action the
kernel returned.  Every C-ABI launch writes into sentinel-filled outputs with elements behind the last one, which must
keep the sentinel; pad columns of the logits hold NaN patterns, which must not reach any output.
"""
import numpy as np
import pytest
import torch

import policy_judge as J

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
SENT = -7    # the integer pattern the outputs hold before a launch (as float32 / 16-bit floats a NaN nothing here produces)
TAIL = 40    # elements behind the last one of every buffer
NP_LOGIT = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
TORCH_LOGIT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
TORCH_ACTION = {"int32": torch.int32, "int64": torch.int64}
NAN_BITS = 0x7FC00000


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import policy

    return policy.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_rows(values, dtype, pitch, offset):
    """[n, A] float32 values (representable in `dtype`) -> (a flat device tensor holding them at `pitch` elements from row to
    row, starting `offset` elements in, a NaN pattern everywhere else; the address of the first row)"""
    n, A = values.shape
    bits = J.logit_bits(values, dtype)
    flat = np.empty(offset + n * pitch + TAIL, bits.dtype)
    flat[:] = J.logit_bits(np.array([np.nan], np.float32), dtype)[0]
    flat[offset:offset + n * pitch].reshape(n, pitch)[:, :A] = bits
    host = flat.view(np.int16) if flat.dtype == np.uint16 else flat
    t = torch.from_numpy(host).to("cuda:0")
    return t, t.data_ptr() + offset * flat.itemsize


def sentinel(count, torch_dtype):
    return torch.full((count + TAIL,), SENT, dtype=torch_dtype, device="cuda:0")


def run_sample(lib, logits, dtype, pitch, offset, action_dtype, draw, both=True, with_logp=True, with_ent=True, step_dev_tensor=None):
    """pz_sample_actions on both (or one) agents' [n, A] float32 values: per side (actions int64, logp, entropy) as numpy,
    checked for the sentinels; plus the device buffers of the launch"""
    n, A = logits[0].shape
    sides = 2 if both else 1
    bufs = [device_rows(l, dtype, pitch, offset) for l in logits[:sides]]
    act = [sentinel(n, TORCH_ACTION[action_dtype]) for _ in range(sides)]
    logp = [sentinel(n, torch.int32) for _ in range(sides)]
    ent = [sentinel(n, torch.int32) for _ in range(sides)]
    seed, first_game, step, step_dev = draw
    if step_dev is not None and step_dev_tensor is None:
        step_dev_tensor = torch.tensor([step_dev], dtype=torch.int64, device="cuda:0")
    p = lambda ts, on=True: [(ts[i].data_ptr() if on and i < sides else None) for i in (0, 1)]  # noqa: E731
    err = lib.pz_sample_actions(bufs[0][1], bufs[1][1] if both else None, J.LOGIT_DTYPES.index(dtype), A, n, pitch, seed, first_game,
                                step, step_dev_tensor.data_ptr() if step_dev_tensor is not None else None,
                                J.ACTION_DTYPES.index(action_dtype), *p(act), *p(logp, with_logp), *p(ent, with_ent), stream())
    assert err == 0
    torch.cuda.synchronize()
    out = []
    for s in range(sides):
        a, lp, en = cpu(act[s]), cpu(logp[s]), cpu(ent[s])
        assert (a[n:] == SENT).all() and (lp[n:] == SENT).all() and (en[n:] == SENT).all(), "a launch wrote behind its output"
        assert with_logp or (lp == SENT).all()
        assert with_ent or (en == SENT).all()
        out.append((a[:n].astype(np.int64), lp[:n].view(np.float32), en[:n].view(np.float32)))
    return out, dict(bufs=bufs, act=act, logp=logp, ent=ent)


def check_against_judge(l, u, got, where):
    """one side's (actions, logp, entropy) of a sampling launch against the judge"""
    act, logp, ent = got
    n, A = l.shape
    a, amb, nb, st = J.sample(l, u)
    assert ((act >= 0) & (act < A)).all(), where
    wrong = np.nonzero(~amb & (act != a))[0]
    assert wrong.size == 0, (where, "row", int(wrong[0]), "got", int(act[wrong[0]]), "judge", int(a[wrong[0]]), "u", u[wrong[0]])
    assert ((act >= nb[:, 0]) & (act <= nb[:, 1]) & (st["live"][np.arange(n), act] | st["bad"])).all(), where
    good = ~st["bad"]
    assert (act[~good] == 0).all() and np.isnan(logp[~good]).all() and np.isnan(ent[~good]).all(), where
    want, tol = J.log_prob(st, act)
    err_logp = np.abs(logp.astype(np.float64) - want)[good]
    err_ent = np.abs(ent.astype(np.float64) - st["H"])[good]
    tol_ent = J.entropy_tolerance(st)[good]
    if good.any():
        print(f"{where}: logp error / tolerance {float((err_logp / tol[good]).max()):.3f}, entropy {float((err_ent / tol_ent).max()):.3f}, "
              f"{int(amb.sum())} ambiguous of {n}")
    assert (err_logp <= tol[good]).all() and (err_ent <= tol_ent).all(), where
    return st, amb


def check_row_kinds(kind, got, A):
    act, logp, ent = got
    k = np.array(kind)
    assert (logp[k == "one_hot"] == 0).all() and (ent[k == "one_hot"] == 0).all()  # exactly: S = 1, log 1 = 0, T = 0
    assert np.allclose(ent[k == "equal"], np.log(A), rtol=0, atol=2e-6) and np.allclose(logp[k == "equal"], -np.log(A), rtol=0, atol=2e-6)


def run_log_probs(lib, bufs, dtype, n, A, pitch, action_dtype, act, both=True):
    sides = 2 if both else 1
    logp = [sentinel(n, torch.int32) for _ in range(sides)]
    ent = [sentinel(n, torch.int32) for _ in range(sides)]
    p = lambda ts: [(ts[i].data_ptr() if i < sides else None) for i in (0, 1)]  # noqa: E731
    err = lib.pz_action_log_probs(bufs[0][1], bufs[1][1] if both else None, J.LOGIT_DTYPES.index(dtype), A, n, pitch,
                                  J.ACTION_DTYPES.index(action_dtype), *p(act), *p(logp), *p(ent), stream())
    assert err == 0
    torch.cuda.synchronize()
    return [cpu(t) for t in logp], [cpu(t) for t in ent]


def run_backward(lib, bufs, dtype, n, A, pitch, action_dtype, act, glogp, gent, grad_pitch, grad_offset, both=True):
    """pz_action_log_probs_backward; glogp / gent: per side float32 [n] or None (the pair is NULL).  Per side the [n, A]
    gradient as float32, checked for untouched pad columns and elements behind the rows."""
    sides = 2 if both else 1
    np_dtype = NP_LOGIT[dtype]
    size = np.dtype(np_dtype).itemsize
    grads = [torch.full((grad_offset + n * grad_pitch + TAIL,), SENT, dtype=torch.int32 if size == 4 else torch.int16, device="cuda:0")
             for _ in range(sides)]
    up = lambda xs: [None, None] if xs is None else [torch.from_numpy(x).to("cuda:0") for x in xs[:sides]] + [None] * (2 - sides)  # noqa: E731
    gl, ge = up(glogp), up(gent)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    p = lambda ts: [(ts[i].data_ptr() if i < sides else None) for i in (0, 1)]  # noqa: E731
    gp = [g.data_ptr() + grad_offset * size for g in grads] + [None] * (2 - sides)
    err = lib.pz_action_log_probs_backward(bufs[0][1], bufs[1][1] if both else None, J.LOGIT_DTYPES.index(dtype), A, n, pitch,
                                           J.ACTION_DTYPES.index(action_dtype), *p(act), ptr(gl[0]), ptr(gl[1]), ptr(ge[0]), ptr(ge[1]),
                                           gp[0], gp[1], grad_pitch, stream())
    assert err == 0
    torch.cuda.synchronize()
    out = []
    for g in grads:
        flat = cpu(g)
        rows = flat[grad_offset:grad_offset + n * grad_pitch].reshape(n, grad_pitch)
        assert (flat[:grad_offset] == SENT).all() and (flat[grad_offset + n * grad_pitch:] == SENT).all(), "the backward wrote outside its rows"
        assert (rows[:, A:] == SENT).all(), "the backward wrote a pad column"
        out.append(J.bits_to_float(np.ascontiguousarray(rows[:, :A]).view(np_dtype if dtype != "bfloat16" else np.uint16), dtype))
    return out


def check_gradient(st, act, glogp, gent, got, dtype, where):
    n = st["n"]
    zero = np.zeros(n, np.float32)
    want, tol = J.gradient(st, act, zero if glogp is None else glogp, zero if gent is None else gent)
    good = ~st["bad"]
    assert np.isnan(got[~good]).all(), where
    rounded, ulp = J.round_to(want[good], dtype)
    err = np.abs(got[good].astype(np.float64) - rounded)
    allowed = tol[good] + (ulp if dtype != "float32" else 0.0)
    assert (err <= allowed).all(), (where, float((err / allowed).max()))


CONFIGS = [(n, extra, offset, adt, both) for n in J.N_EDGES for extra in (0, 1) for offset in (0, 1) for adt in J.ACTION_DTYPES
           for both in (True, False)]


@pytest.mark.parametrize("dtype", J.LOGIT_DTYPES)
@pytest.mark.parametrize("A", J.A_EDGES)
def test_sample_log_probs_and_backward_against_the_judge(lib, A, dtype):
    """Every n of policy_judge.N_EDGES x pitch A and A + 1 x the base pointer at the buffer's start and one element in x
    both action formats x both sides and one, the draws (seed, first game, step, device part) cycling: the sampling
    launch against the judge; pz_action_log_probs on the sampled actions bit for bit equal to it; the backward against
    the judge's gradient, at grad_pitch A and A + 1, with either upstream pair absent in turn."""
    rng = np.random.default_rng(A)
    cases = {}
    for i, (n, extra, offset, adt, both) in enumerate(CONFIGS):
        index = i % len(J.DRAWS)
        draw = J.DRAWS[index]
        if (n, index) not in cases:  # (the judge's inputs of a case, computed once)
            cases[n, index] = (J.case_logits(n, A, dtype, index), J.uniforms(*draw, n))
        logits, us = cases[n, index]
        pitch = A + extra
        where = f"A={A} {dtype} n={n} pitch={pitch} offset={offset} {adt} both={both} draw={index}"
        got, dev = run_sample(lib, [l for l, _ in logits], dtype, pitch, offset, adt, draw, both)
        sides = 2 if both else 1
        logp2, ent2 = run_log_probs(lib, dev["bufs"], dtype, n, A, pitch, adt, dev["act"], both)
        glogp = [rng.normal(size=n).astype(np.float32) for _ in range(sides)] if i % 3 != 1 else None
        gent = [rng.normal(size=n).astype(np.float32) for _ in range(sides)] if i % 3 != 2 else None
        grads = run_backward(lib, dev["bufs"], dtype, n, A, pitch, adt, dev["act"], glogp, gent, A + (i // 2) % 2, (i // 4) % 2, both)
        for s in range(sides):
            st, _ = check_against_judge(logits[s][0], us[s], got[s], f"{where} side {s}")
            check_row_kinds(logits[s][1], got[s], A)
            assert np.array_equal(logp2[s][:n], cpu(dev["logp"][s])[:n]) and np.array_equal(ent2[s][:n], cpu(dev["ent"][s])[:n]), where
            assert (logp2[s][n:] == SENT).all() and (ent2[s][n:] == SENT).all()
            check_gradient(st, got[s][0], None if glogp is None else glogp[s], None if gent is None else gent[s], grads[s], dtype, where)


def test_wide_pitches_are_gathered(lib):
    """a pitch above the staged range (a view into a much wider tensor) and one at its edge"""
    for pitch in (64, 65, 700):
        for dtype in ("float32", "bfloat16"):
            n, A = 191, 18
            logits = J.case_logits(n, A, dtype, 0)
            us = J.uniforms(*J.DRAWS[1], n)
            got, dev = run_sample(lib, [l for l, _ in logits], dtype, pitch, 1, "int64", J.DRAWS[1])
            glogp = [np.ones(n, np.float32)] * 2
            grads = run_backward(lib, dev["bufs"], dtype, n, A, pitch, "int64", dev["act"], glogp, None, pitch, 1)
            for s in (0, 1):
                st, _ = check_against_judge(logits[s][0], us[s], got[s], f"pitch {pitch} {dtype} side {s}")
                check_gradient(st, got[s][0], glogp[s], None, grads[s], dtype, f"pitch {pitch} {dtype}")


def test_optional_outputs_and_given_actions_out_of_range(lib):
    n, A = 191, 18
    logits = J.case_logits(n, A, "float32", 0)
    ls = [l for l, _ in logits]
    full, _ = run_sample(lib, ls, "float32", A, 0, "int32", J.DRAWS[0])
    for with_logp, with_ent in ((False, True), (True, False), (False, False)):
        part, _ = run_sample(lib, ls, "float32", A, 0, "int32", J.DRAWS[0], with_logp=with_logp, with_ent=with_ent)
        for s in (0, 1):
            assert np.array_equal(part[s][0], full[s][0])
            assert not with_logp or np.array_equal(part[s][1].view(np.uint32), full[s][1].view(np.uint32))
            assert not with_ent or np.array_equal(part[s][2].view(np.uint32), full[s][2].view(np.uint32))
    # given actions outside [0, A): a NaN log-prob, the entropy of the row, no [i == a] term in the gradient
    bufs = [device_rows(l, "float32", A, 0) for l in ls]
    for adt, values in (("int32", (-1, A, 2 ** 31 - 1)), ("int64", (-1, A, 2 ** 40, -2 ** 40))):
        given = np.arange(n) % A
        given[:len(values)] = 0
        acts = []
        for s in (0, 1):
            t = sentinel(n, TORCH_ACTION[adt])
            host = given.astype(np.int64)
            host[:len(values)] = values
            t[:n] = torch.from_numpy(host).to(TORCH_ACTION[adt])
            acts.append(t)
        logp, ent = run_log_probs(lib, bufs, "float32", n, A, A, adt, acts)
        grads = run_backward(lib, bufs, "float32", n, A, A, adt, acts, [np.ones(n, np.float32)] * 2, None, A, 0)
        for s in (0, 1):
            st = J.stats(ls[s])
            host = cpu(acts[s])[:n].astype(np.int64)
            want, tol = J.log_prob(st, host)
            got = logp[s][:n].view(np.float32)
            bad_rows = st["bad"][:len(values)]
            assert np.isnan(got[:len(values)]).all() and np.isnan(want[:len(values)]).all()
            fin = np.isfinite(want)
            assert (np.abs(got - want)[fin] <= tol[fin]).all() and np.array_equal(np.isnan(got), np.isnan(want))
            assert np.array_equal(ent[s][:n].view(np.uint32), full[s][2].view(np.uint32))
            check_gradient(st, host, np.ones(n, np.float32), None, grads[s], "float32", f"out of range {adt}")
            rows = ~bad_rows
            assert np.allclose(grads[s][:len(values)][rows], -st["p"][:len(values)][rows], atol=1e-5)


@pytest.mark.parametrize("side", [0, 1])
def test_the_largest_u_on_masked_tails(lib, side):
    """u = 1 - 2^-24 (the committed game ids of policy_judge.LARGEST_U) on rows whose last actions are masked: the last
    LIVE action, never a masked one"""
    for A in J.A_EDGES[1:]:
        for dtype in J.LOGIT_DTYPES:
            l, first = J.largest_u_case(A, dtype, side)
            draw = (J.LARGEST_U["seed"], first, J.LARGEST_U["step"], None)
            us = J.uniforms(*draw, 64)
            assert us[side][5] == 1 - 2.0 ** -24
            got, _ = run_sample(lib, [l, l], dtype, A + 1, 1, "int64", draw)
            st, amb = check_against_judge(l, us[side], got[side], f"largest u, A={A} {dtype} side {side}")
            assert not amb[5] and got[side][0][5] == st["last"][5] and np.isfinite(l[np.arange(64), got[side][0]]).all()


def test_a_shard_draws_what_the_whole_batch_draws(lib):
    n, A, g0 = 4133, 18, 1000
    for dtype, index in (("float32", 1), ("bfloat16", 2)):
        logits = [l for l, _ in J.case_logits(n, A, dtype, index)]
        seed, first, step, step_dev = J.DRAWS[index]
        whole, _ = run_sample(lib, logits, dtype, A + 1, 0, "int64", J.DRAWS[index])
        shard, _ = run_sample(lib, [l[g0:] for l in logits], dtype, A + 1, 0, "int64", (seed, first + g0, step, step_dev))
        for s in (0, 1):
            for w, h in zip(whole[s], shard[s]):
                assert np.array_equal(w[g0:].view(np.uint32 if w.dtype == np.float32 else w.dtype), h.view(np.uint32 if h.dtype == np.float32 else h.dtype))


def as_torch(values, dtype):
    bits = J.logit_bits(values, dtype)
    if dtype == "bfloat16":
        return torch.from_numpy(bits.view(np.int16)).to("cuda:0").view(torch.bfloat16)
    return torch.from_numpy(bits).to("cuda:0")


def test_policy_sample_and_its_out_argument():
    from pikazoo_amd import policy

    n, A = 191, 18
    logits = J.case_logits(n, A, "bfloat16", 0)
    us = J.uniforms(11, 5, 9, None, n)
    wide = {a: torch.zeros((n, A + 1), dtype=torch.bfloat16, device="cuda:0") for a in (A1, A2)}
    views = {a: wide[a][:, :A] for a in (A1, A2)}  # the actor-critic head: 18 logits and a value per row
    for a, (l, _) in zip((A1, A2), logits):
        views[a].copy_(as_torch(l, "bfloat16"))
        wide[a][:, A] = float("nan")
    out = policy.sample(views, seed=11, step=9, first_game=5)
    again = policy.sample(views, seed=11, step=9, first_game=5, out=out)
    counter = torch.tensor([4], dtype=torch.int64, device="cuda:0")
    by_counter = policy.sample(views, seed=11, step=counter + 5, first_game=5, action_dtype=torch.int32)
    one = policy.sample(views[A1], seed=11, step=9, first_game=5)
    torch.cuda.synchronize()
    assert again is out and list(out) == ["actions", "log_probs", "entropy"] and list(out["actions"]) == [A1, A2]
    assert out["actions"][A1].dtype == torch.int64 and by_counter["actions"][A1].dtype == torch.int32
    assert isinstance(one["actions"], torch.Tensor) and torch.equal(one["actions"], out["actions"][A1])
    for s, a in enumerate((A1, A2)):
        got = (cpu(out["actions"][a]), cpu(out["log_probs"][a]), cpu(out["entropy"][a]))
        check_against_judge(logits[s][0], us[s], got, f"policy.sample {a}")
        assert np.array_equal(cpu(by_counter["actions"][a]).astype(np.int64), got[0])
        assert np.array_equal(cpu(by_counter["log_probs"][a]).view(np.uint32), got[1].view(np.uint32))
    for bad in (lambda: policy.sample(views, seed=-1), lambda: policy.sample(views, seed=1, step=-1),
                lambda: policy.sample(views, seed=1, step=1 << 62), lambda: policy.sample(views, seed=1, first_game=-1),
                lambda: policy.sample(views, seed=1, action_dtype=torch.int16),
                lambda: policy.sample(views, seed=1, step=torch.zeros(1, dtype=torch.int32, device="cuda:0")),
                lambda: policy.sample(views, seed=1, step=torch.zeros(1, dtype=torch.int64)),
                lambda: policy.sample(views, seed=1, out={"actions": out["actions"], "log_probs": out["log_probs"]}),
                lambda: policy.sample(views, seed=1, out=by_counter),  # int32 actions where int64 are asked for
                lambda: policy.sample({A1: views[A1], A2: views[A2].contiguous()}, seed=1),  # two row strides
                lambda: policy.sample(views[A1].cpu(), seed=1),
                lambda: policy.log_probs(views, out["actions"][A1]),
                lambda: policy.log_probs(views[A1], out["actions"][A1].to(torch.int16))):
        with pytest.raises(ValueError):
            bad()


def test_graph_capture_replays_to_the_eager_bits():
    """one sampling launch and ``counter.add_(1)`` captured on a side stream: three replays equal three eager calls at
    steps 0, 1 and 2, bit for bit"""
    from pikazoo_amd import policy

    n, A = 191, 18
    logits = {a: as_torch(l, "float32") for a, (l, _) in zip((A1, A2), J.case_logits(n, A, "float32", 0))}
    eager = []
    for step in range(3):
        out = policy.sample(logits, seed=3, step=step, first_game=77)
        torch.cuda.synchronize()
        eager.append({key: {a: cpu(t).copy() for a, t in out[key].items()} for key in out})
    assert not np.array_equal(eager[0]["actions"][A1], eager[1]["actions"][A1])
    counter = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    held = policy.sample(logits, seed=3, step=counter, first_game=77)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = policy.sample(logits, seed=3, step=counter, first_game=77, out=held)
            counter.add_(1)
    assert captured is held
    torch.cuda.synchronize()
    counter.zero_()
    torch.cuda.synchronize()
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for key in held:
            for a in (A1, A2):
                got, want = cpu(held[key][a]), eager[step][key][a]
                assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want), (step, key, a)
    assert int(counter.item()) == 3


def test_sampled_actions_step_the_env_uncast():
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd.wrappers import SimplifyAction

    env = pikazoo_v0.env(num_envs=64, device="cuda:0", seed=5, env_id_base=1 << 33)
    env.reset()
    raw = env.unwrapped
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    logits = {a: torch.randn((64, 18), device="cuda:0", generator=gen) for a in (A1, A2)}
    out = None
    for t in range(3):
        assert raw.steps_done == t
        out = raw.sample_actions(logits, out=out)
        torch.cuda.synchronize()
        us = J.uniforms(5, 1 << 33, t, None, 64)
        for s, a in enumerate((A1, A2)):
            assert out["actions"][a].dtype == torch.int64
            check_against_judge(cpu(logits[a]), us[s], (cpu(out["actions"][a]), cpu(out["log_probs"][a]), cpu(out["entropy"][a])), f"env step {t}")
        before = {a: out["actions"][a].data_ptr() for a in (A1, A2)}
        obs, rew, term, trunc, infos = env.step(out["actions"])  # int64, as they are
        assert {a: out["actions"][a].data_ptr() for a in (A1, A2)} == before
    raw.check_actions()
    assert obs[A1].shape == (64, 35)
    given = raw.sample_actions(logits, step=0)
    torch.cuda.synchronize()
    assert np.array_equal(cpu(given["actions"][A1]), J.sample(cpu(logits[A1]), J.uniforms(5, 1 << 33, 0, None, 64)[0])[0])
    # 13 actions under a fused SimplifyAction: 18 logits are refused before any launch, 13 go
    simple = SimplifyAction(pikazoo_v0.env(num_envs=64, device="cuda:0", seed=5))
    simple.reset()
    assert simple.unwrapped.n_actions == 13
    with pytest.raises(ValueError, match="13"):
        simple.unwrapped.sample_actions(logits)
    small = simple.unwrapped.sample_actions({a: l[:, :13].contiguous() for a, l in logits.items()})
    simple.step(small["actions"])
    simple.unwrapped.check_actions()
    assert int(small["actions"][A1].max()) < 13


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_log_probs_under_autograd(dtype):
    """policy.log_probs through torch.autograd: the forward equals the launch without autograd bit for bit, the backward
    the judge's gradient (gradcheck itself needs float64 inputs: the judge's central-difference-checked gradient stands
    in for it)"""
    from pikazoo_amd import policy

    n, A = 191, 18
    rng = np.random.default_rng(4)
    cases = J.case_logits(n, A, dtype, 1)
    acts_h = [rng.integers(0, A, n) for _ in (0, 1)]
    wide = {a: torch.zeros((n, A + 1), dtype=TORCH_LOGIT[dtype], device="cuda:0") for a in (A1, A2)}
    for a, (l, _) in zip((A1, A2), cases):
        wide[a][:, :A] = as_torch(l, dtype)
    leaves = {a: w.requires_grad_(True) for a, w in wide.items()}
    logits = {a: w[:, :A] for a, w in leaves.items()}
    actions = {a: torch.from_numpy(h).to("cuda:0") for a, h in zip((A1, A2), acts_h)}
    plain = policy.log_probs({a: l.detach() for a, l in logits.items()}, actions)
    logp, ent = policy.log_probs(logits, actions)
    assert logp[A1].requires_grad and ent[A2].requires_grad and not plain[0][A1].requires_grad
    glogp = [rng.normal(size=n).astype(np.float32) for _ in (0, 1)]
    gent = [rng.normal(size=n).astype(np.float32) for _ in (0, 1)]
    good = [~J.stats(l)["bad"] for l, _ in cases]
    loss = sum((logp[a][torch.from_numpy(good[s]).to("cuda:0")] * torch.from_numpy(glogp[s][good[s]]).to("cuda:0")).sum()
               + (ent[a][torch.from_numpy(good[s]).to("cuda:0")] * torch.from_numpy(gent[s][good[s]]).to("cuda:0")).sum()
               for s, a in enumerate((A1, A2)))
    loss.backward()
    torch.cuda.synchronize()
    for s, a in enumerate((A1, A2)):
        assert torch.equal(logp[a].detach().view(torch.int32), plain[0][a].view(torch.int32))
        assert torch.equal(ent[a].detach().view(torch.int32), plain[1][a].view(torch.int32))
        grad = leaves[a].grad
        assert grad.dtype == TORCH_LOGIT[dtype] and (grad[:, A] == 0).all()
        st = J.stats(cases[s][0])
        got = cpu(grad[:, :A].float())
        # (rows the loss leaves out get a zero upstream gradient: their own gradient is the kernel's NaN times nothing)
        gl, ge = np.where(good[s], glogp[s], 0).astype(np.float32), np.where(good[s], gent[s], 0).astype(np.float32)
        check_gradient(st, acts_h[s], gl, ge, got, dtype, f"autograd {dtype} {a}")
    # one tensor, only the entropy used: the log-prob's upstream gradient is absent
    single = as_torch(cases[0][0][good[0]], dtype).requires_grad_(True)
    _, e = policy.log_probs(single, actions[A1][torch.from_numpy(good[0]).to("cuda:0")])
    e.sum().backward()
    torch.cuda.synchronize()
    st = J.stats(cases[0][0][good[0]])
    m = int(good[0].sum())
    check_gradient(st, acts_h[0][good[0]], None, np.ones(m, np.float32), cpu(single.grad.float()), dtype, "entropy only")
