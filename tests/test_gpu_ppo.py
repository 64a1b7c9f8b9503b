"""GPU tests (``-m gpu``) of the PPO-loss launches (include/pikazoo_ppo.h: ``pz_ppo_moments``, ``pz_ppo_loss``) and of
``pikazoo_amd.ppo``.

The judge is tests/ppo_judge.py: the header's definition in numpy float64 with DERIVED tolerances and derived ambiguity
widths (held to central differences, a torch float64 formulation, a float32 restatement and mutants by
tests/test_ppo_host.py).  No GPU result is ever an expected value.  Every C-ABI launch writes into sentinel-filled outputs
with elements behind the last one, which must keep the sentinel; pad columns of the logits, the values and the gradients
hold NaN patterns or sentinels, which must stay and must not reach any output.
"""
import numpy as np
import pytest
import torch

import policy_judge as J
import ppo_judge as P
from test_gpu_policy import NP_LOGIT, SENT, TAIL, TORCH_ACTION, TORCH_LOGIT, as_torch, cpu, device_rows, run_backward, run_log_probs, sentinel, stream

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
WS_TAIL, WS_FILL = 64, 0xA5


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import ppo

    return ppo.load()


def f32_vector(x):
    """a float32 [n] input with NaN-pattern elements behind it"""
    host = np.full(len(x) + TAIL, np.nan, np.float32)
    host[:len(x)] = x
    return torch.from_numpy(host).to("cuda:0")


def int_buffer(count, itemsize):
    return torch.full((count,), SENT, dtype=torch.int32 if itemsize == 4 else torch.int16, device="cuda:0")


def workspace_for(lib, n):
    size = int(lib.pz_ppo_workspace_bytes(n))
    return torch.full((max(size, 16) + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda:0"), size


def run_moments(lib, xs, eps=1e-8, ws=None):
    """pz_ppo_moments on one or two float32 vectors: ([side][mean, rscale] as float32, the device buffer)"""
    n = len(xs[0])
    bufs = [f32_vector(x) for x in xs]
    out = sentinel(4, torch.int32)
    own = ws is None
    if own:
        ws, size = workspace_for(lib, n)
    err = lib.pz_ppo_moments(bufs[0].data_ptr(), bufs[1].data_ptr() if len(xs) == 2 else None, n, eps, out.data_ptr(), ws.data_ptr(), stream())
    assert err == 0
    torch.cuda.synchronize()
    host = cpu(out)
    assert (host[2 * len(xs):] == SENT).all(), "the moments wrote behind their output"
    if own:
        assert (cpu(ws)[max(size, 16):] == WS_FILL).all(), "the moments wrote behind their workspace"
    return host[:2 * len(xs)].view(np.float32).reshape(len(xs), 2), out


def run_loss(lib, cases, dtype, vdt, pitch=None, offset=0, adt="int64", grad_pitch=None, grad_offset=0, value_pitch=1, old_vdt=None,
             with_grad_logits=True, with_grad_values=True, grad_value_pitch=1, fused=False):
    """pz_ppo_loss (behind pz_ppo_moments where the case normalises) on one or two agents' cases: per side
    {"stats" [8], "grad_logits" [n, A] or None, "grad_values" [n] or None} as float32 values, every buffer checked for
    what must not have been written.  `fused`: logits and value are one [n, A + 1] tensor at `pitch`, and so are the
    gradients at `grad_pitch`."""
    c0 = cases[0]
    n, A = c0["logits"].shape
    sides = len(cases)
    pitch = pitch or (A + 1 if fused else A)
    grad_pitch = grad_pitch or (A + 1 if fused else A)
    lsize, vsize = np.dtype(NP_LOGIT[dtype]).itemsize, np.dtype(NP_LOGIT[vdt]).itemsize
    if fused:
        assert vdt == dtype and pitch > A and grad_pitch > A
        heads = [device_rows(np.concatenate([c["logits"], c["values"][:, None]], 1), dtype, pitch, offset) for c in cases]
        lptr = [h[1] for h in heads]
        vptr = [p + A * lsize for p in lptr]
        value_pitch = pitch
    else:
        lbufs = [device_rows(c["logits"], dtype, pitch, offset) for c in cases]
        vbufs = [device_rows(c["values"][:, None], vdt, value_pitch, 1) for c in cases]
        lptr, vptr = [b[1] for b in lbufs], [b[1] for b in vbufs]
    act = [sentinel(n, TORCH_ACTION[adt]) for _ in cases]
    for t, c in zip(act, cases):
        t[:n] = torch.from_numpy(c["actions"]).to(TORCH_ACTION[adt])
    old_logp, adv, ret = ([f32_vector(c[k]) for c in cases] for k in ("old_logp", "adv", "ret"))
    clipped = c0["value_clip"] > 0
    old_vdt = old_vdt or vdt
    oldv = [device_rows(c["old_values"][:, None], old_vdt, 1, 1) for c in cases] if clipped else None
    glog = [int_buffer(grad_offset + n * grad_pitch + TAIL, lsize) for _ in cases]
    gptr = [g.data_ptr() + grad_offset * lsize for g in glog]
    if fused:
        gval, gvptr, grad_value_pitch = None, [p + A * lsize for p in gptr], grad_pitch
    else:
        gval = [int_buffer(1 + n * grad_value_pitch + TAIL, vsize) for _ in cases]
        gvptr = [g.data_ptr() + vsize for g in gval]
    stats = sentinel(16, torch.int32)
    ws, size = workspace_for(lib, n)
    norm = None
    if c0["normalize"]:
        _, norm = run_moments(lib, [c["adv"] for c in cases], ws=ws)
    two = lambda ps, on=True: [(ps[i] if on and i < sides else None) for i in (0, 1)]  # noqa: E731
    ptrs = lambda ts, on=True: two([t.data_ptr() for t in ts], on)  # noqa: E731
    err = lib.pz_ppo_loss(*two(lptr), J.LOGIT_DTYPES.index(dtype), A, n, pitch, J.ACTION_DTYPES.index(adt), *ptrs(act), *ptrs(old_logp),
                          *ptrs(adv), *ptrs(ret), *two(vptr), J.LOGIT_DTYPES.index(vdt), value_pitch,
                          *(two([b[1] for b in oldv]) if clipped else (None, None)), J.LOGIT_DTYPES.index(old_vdt) if clipped else 0,
                          norm.data_ptr() if norm is not None else None, c0["clip"], c0["value_clip"], c0["vf_coef"], c0["ent_coef"],
                          *two(gptr, with_grad_logits), grad_pitch, *two(gvptr, with_grad_values), grad_value_pitch, stats.data_ptr(),
                          ws.data_ptr(), stream())
    assert err == 0
    torch.cuda.synchronize()
    host_stats = cpu(stats)
    assert (host_stats[8 * sides:] == SENT).all(), "the loss wrote behind its statistics"
    assert (cpu(ws)[max(size, 16):] == WS_FILL).all(), "the loss wrote behind its workspace"
    out = []
    for s in range(sides):
        st = host_stats[8 * s:8 * s + 8].view(np.float32)
        assert st[6:].view(np.uint32).tolist() == [0, 0], "statistics 6 and 7 are +0"
        flat = cpu(glog[s])
        rows = flat[grad_offset:grad_offset + n * grad_pitch].reshape(n, grad_pitch)
        assert (flat[:grad_offset] == SENT).all() and (flat[grad_offset + n * grad_pitch:] == SENT).all(), "a gradient outside its rows"
        live = A + 1 if fused and with_grad_values else A
        assert (rows[:, live:] == SENT).all(), "a pad column of the gradient was written"
        as_values = lambda bits, d: J.bits_to_float(np.ascontiguousarray(bits).view(NP_LOGIT[d] if d != "bfloat16" else np.uint16), d)  # noqa: E731
        gl = gv = None
        if with_grad_logits:
            gl = as_values(rows[:, :A], dtype)
        else:
            assert (rows[:, :A] == SENT).all()
        if fused:
            if with_grad_values:
                gv = as_values(rows[:, A], dtype)
        else:
            vflat = cpu(gval[s])
            vrows = vflat[1:1 + n * grad_value_pitch].reshape(n, grad_value_pitch)
            assert vflat[0] == SENT and (vflat[1 + n * grad_value_pitch:] == SENT).all() and (vrows[:, 1:] == SENT).all(), "a value gradient outside its column"
            if with_grad_values:
                gv = as_values(vrows[:, 0], vdt)
            else:
                assert (vrows == SENT).all()
        out.append(dict(stats=st, grad_logits=gl, grad_values=gv))
    return out


def check(jd, got, dtype, vdt, where):
    res = P.compare(jd, got, dtype, vdt)
    print(f"{where}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, (_, v) in res.items()) + f"; {int(jd['ambiguous'].sum())} ambiguous")
    assert not P.failures(res), (where, res)


# the layouts every case runs under: (logit pitch: A + extra or 67, base offset, action format, both agents, gradient of the
# logits, gradient of the values, value pitch, gradient pitch extra, gradient offset, gradient value pitch, old values as float32)
LAYOUTS = ((0, 0, "int64", True, True, True, 1, 0, 0, 1, False),
           (1, 1, "int32", True, True, True, 3, 1, 1, 2, True),
           (67, 0, "int64", False, False, True, 1, 0, 0, 1, False),
           (0, 1, "int32", False, True, False, 2, 0, 1, 1, True),
           (67, 1, "int64", True, True, True, 1, 67, 0, 1, False))


@pytest.mark.parametrize("dtype", J.LOGIT_DTYPES)
@pytest.mark.parametrize("A", J.A_EDGES)
def test_loss_statistics_and_gradients_against_the_judge(lib, A, dtype):
    """Every n of ppo_judge.N_EDGES (policy_judge's, and 19 141 rows = 300 partials for the finisher's 256 threads), value
    clip and normalisation on and off with n, the value format cycling, under five layouts: logit pitch A, A + 1 and 67,
    the base pointer one element in, both action formats, one side and two, each gradient pair NULL in turn, value and
    gradient pitches above 1, old values in their own format; the fused head ([n, A + 1], value and its gradient in column
    A) at pitch A + 1 and wider; and the planted boundary rows."""
    for name, cases, vdt, planted, fused in P.gpu_cases(A, dtype):
        judged = [P.judge(c) for c in cases]
        if fused:
            for pitch, gpitch, offset in ((A + 1, A + 1, 0), (A + 3, A + 2, 1)):
                got = run_loss(lib, cases, dtype, vdt, pitch=pitch, offset=offset, grad_pitch=gpitch, grad_offset=offset, fused=True)
                for s in (0, 1):
                    check(judged[s], got[s], dtype, vdt, f"A={A} {dtype} {name} pitch {pitch} side {s}")
            continue
        for k, (extra, offset, adt, both, gl, gv, vpitch, gextra, goffset, gvpitch, old32) in enumerate(LAYOUTS):
            pitch = 67 if extra == 67 else A + extra
            got = run_loss(lib, cases if both else cases[:1], dtype, vdt, pitch=pitch, offset=offset, adt=adt,
                           grad_pitch=67 if gextra == 67 else A + gextra, grad_offset=goffset, value_pitch=vpitch,
                           old_vdt="float32" if old32 else vdt, with_grad_logits=gl, with_grad_values=gv, grad_value_pitch=gvpitch)
            for s in range(len(got)):
                check(judged[s], got[s], dtype, vdt, f"A={A} {dtype} {name} layout {k} side {s}")


@pytest.mark.parametrize("dtype", J.LOGIT_DTYPES)
def test_first_epoch_pins_and_agreement_with_the_policy_backward(lib, dtype):
    """old_logp from pz_action_log_probs on the same logits and actions: d == +0 and r == 1 in every row, so approx_kl and
    clip_fraction are +0 BIT FOR BIT; and the gradient agrees with pz_action_log_probs_backward's for glogp = -Ahat / M,
    gent = -ent_coef / M within the two launches' judged bounds."""
    n, A = 4133, 18
    cases = [P.make_case(n, A, dtype, "float32", seed=400 + s, value_clip=0.0, normalize=False) for s in (0, 1)]
    bufs = [device_rows(c["logits"], dtype, A + 1, 1) for c in cases]
    act = [sentinel(n, torch.int64) for _ in cases]
    for t, c in zip(act, cases):
        t[:n] = torch.from_numpy(c["actions"])
    logp, _ = run_log_probs(lib_policy(), bufs, dtype, n, A, A + 1, "int64", act)
    for s, c in enumerate(cases):
        c["old_logp"] = logp[s][:n].view(np.float32).copy()
        assert np.isfinite(c["old_logp"]).all()
    got = run_loss(lib, cases, dtype, "float32", pitch=A + 1, offset=1)
    M = np.float32(n)
    glogp = [(-c["adv"] / M).astype(np.float32) for c in cases]
    gent = [np.full(n, -np.float32(c["ent_coef"]) / M, np.float32) for c in cases]
    back = run_backward(lib_policy(), bufs, dtype, n, A, A + 1, "int64", act, glogp, gent, A, 0)
    for s, c in enumerate(cases):
        jd = P.judge(c)
        assert got[s]["stats"][4:6].view(np.uint32).tolist() == [0, 0], got[s]["stats"]
        check(jd, got[s], dtype, "float32", f"first epoch {dtype} side {s}")
        assert (jd["glp_k"] == 0).all()
        want, tol = J.gradient(jd["st"], c["actions"], glogp[s], gent[s])
        _, ulp = J.round_to(want, dtype)
        allowed = tol + jd["t_grad_logits"][0] + (2 * ulp if dtype != "float32" else 0.0)
        diff = np.abs(got[s]["grad_logits"].astype(np.float64) - back[s].astype(np.float64))
        assert (diff <= allowed).all(), float((diff / allowed).max())


def lib_policy():
    from pikazoo_amd import policy

    return policy.load()


def test_two_runs_return_the_same_bits(lib):
    """pin (b): 300 partials per agent and term, two agents, two launches of everything -- the same bits in the statistics
    and in both gradients, whatever order the workgroups ran in"""
    n, A = P.N_EDGES[-1], 18
    cases = [P.make_case(n, A, "bfloat16", "float16", seed=500 + s) for s in (0, 1)]
    first = run_loss(lib, cases, "bfloat16", "float16")
    second = run_loss(lib, cases, "bfloat16", "float16")
    for a, b in zip(first, second):
        assert np.array_equal(a["stats"].view(np.uint32), b["stats"].view(np.uint32))
        assert np.array_equal(a["grad_logits"].view(np.uint32), b["grad_logits"].view(np.uint32))
        assert np.array_equal(a["grad_values"].view(np.uint32), b["grad_values"].view(np.uint32))
    assert np.isfinite(first[0]["stats"]).all()


def test_special_rows(lib):
    """rows of the policy header's step 6 (a NaN, a +inf, no finite logit), masked rows, and actions outside [0, A): NaN
    gradient rows; loss, policy_loss, approx_kl and clip_fraction NaN; entropy NaN only with a step-6 row; value_loss never"""
    n, A = 191, 18
    for kinds, with_bad in ((P.GOOD_KINDS, False), (J.ROW_KINDS, True)):
        for dtype in ("float32", "bfloat16"):
            cases = [P.make_case(n, A, dtype, "float32", seed=600 + s, kinds=kinds) for s in (0, 1)]
            for c, values in zip(cases, ((-1, A, 2 ** 40), (-2 ** 40, A + 5, -7))):
                rows = [g for g in range(n) if c["kinds"][g] == "random2"][:3]
                c["actions"][rows] = values
            got = run_loss(lib, cases, dtype, "float32", pitch=A + 1, offset=1, adt="int64")
            for s, c in enumerate(cases):
                jd = P.judge(c)
                assert jd["nan_row"].sum() >= 3 and (jd["bad"].any() == with_bad)
                check(jd, got[s], dtype, "float32", f"special rows {dtype} bad={with_bad} side {s}")
                st = got[s]["stats"]
                assert np.isnan(st[[0, 1, 4, 5]]).all() and np.isfinite(st[2]) and np.isnan(st[3]) == with_bad, st
                assert np.isnan(got[s]["grad_logits"][jd["nan_row"]]).all() and np.isfinite(got[s]["grad_logits"][~jd["nan_row"]]).all()
                assert np.isfinite(got[s]["grad_values"]).all()


def test_moments(lib):
    """mean and 1 / (std + eps) against the float64 judge: normal data, the offset case (1000 + noise of spread 1e-3), n = 2,
    a constant vector, an outlier as the shift, 300 partials; one side and two; twice the same bits; n = 1 refused"""
    cases = P.moments_cases()
    for name, x in cases.items():
        mean, rscale, t_mean, t_rs = P.moments(x)
        got, _ = run_moments(lib, [x])
        again, _ = run_moments(lib, [x, x])
        print(f"moments {name}: mean error / bound {abs(got[0, 0] - mean) / t_mean if t_mean else 0:.3f}, rscale {abs(got[0, 1] - rscale) / t_rs:.3f}")
        assert abs(got[0, 0] - mean) <= t_mean and abs(got[0, 1] - rscale) <= t_rs, (name, got, mean, rscale)
        assert np.array_equal(again[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(again[1].view(np.uint32), got[0].view(np.uint32))
    pair, _ = run_moments(lib, [cases["normal"], cases["offset"]], eps=0.0)
    for s, name in enumerate(("normal", "offset")):
        mean, rscale, t_mean, t_rs = P.moments(cases[name], eps=0.0)
        assert abs(pair[s, 0] - mean) <= t_mean and abs(pair[s, 1] - rscale) <= t_rs
    x = f32_vector(cases["two"])
    out = sentinel(4, torch.int32)
    ws, _ = workspace_for(lib, 2)
    assert lib.pz_ppo_moments(x.data_ptr(), None, 1, 1e-8, out.data_ptr(), ws.data_ptr(), stream()) == -2
    torch.cuda.synchronize()
    assert (cpu(out) == SENT).all()
    nan, _ = run_moments(lib, [np.array([1.0, np.nan, 2.0], np.float32)])
    assert np.isnan(nan).all()


def torch_on_device(case, logits, values):
    """the trainer's own formulation (CleanRL's) in torch float64 on the device, under autograd"""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float64)).to("cuda:0")  # noqa: E731
    dist = torch.distributions.Categorical(logits=logits)
    logratio = dist.log_prob(torch.from_numpy(case["actions"]).to("cuda:0")) - t(case["old_logp"])
    ratio = logratio.exp()
    adv = t(case["adv"])
    if case["normalize"]:
        adv = (adv - adv.mean()) / (adv.std() + P.f32(1e-8))
    clip, vclip = P.f32(case["clip"]), P.f32(case["value_clip"])
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    ret, old_v = t(case["ret"]), t(case["old_values"])
    v_clipped = old_v + torch.clamp(values - old_v, -vclip, vclip)
    v_loss = 0.5 * torch.max((values - ret) ** 2, (v_clipped - ret) ** 2).mean()
    ent = dist.entropy().mean()
    loss = pg + P.f32(case["vf_coef"]) * v_loss - P.f32(case["ent_coef"]) * ent
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
        cf = ((ratio - 1.0).abs() > clip).double().mean()
    return loss, [float(x.detach()) for x in (loss, pg, v_loss, ent, kl, cf)]


UNMASKED = ("random0.5", "random2", "random6", "equal", "plus80", "minus100")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_loss_under_autograd_out_reuse_and_graph_capture(dtype):
    """ppo.loss through torch.autograd against the judge and against the torch formulation on the device (float64, so it
    lies within the judge's bounds itself), separate tensors and the fused head; loss_and_grad with out= allocates and
    moves nothing; the pair of launches captured into a graph replays to the eager bits twice."""
    from pikazoo_amd import ppo

    n, A = 4133, 18
    cases = [P.make_case(n, A, dtype, dtype, seed=700 + s, kinds=UNMASKED) for s in (0, 1)]
    judged = [P.judge(c) for c in cases]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    common = dict(actions={a: dev(c["actions"]) for a, c in zip((A1, A2), cases)},
                  old_log_probs={a: dev(c["old_logp"]) for a, c in zip((A1, A2), cases)},
                  advantages={a: dev(c["adv"]) for a, c in zip((A1, A2), cases)},
                  returns={a: dev(c["ret"]) for a, c in zip((A1, A2), cases)},
                  old_values={a: as_torch(c["old_values"], dtype) for a, c in zip((A1, A2), cases)},
                  clip=P.CLIP, value_clip=P.VALUE_CLIP, vf_coef=P.VF_COEF, ent_coef=P.ENT_COEF)
    # the torch formulation on the device lies within the judge's bounds
    for s, c in enumerate(cases):
        l64 = dev(c["logits"].astype(np.float64)).requires_grad_(True)
        v64 = dev(c["values"].astype(np.float64)).requires_grad_(True)
        loss, stats = torch_on_device(c, l64, v64)
        loss.backward()
        torch.cuda.synchronize()
        check(judged[s], dict(stats=np.array(stats), grad_logits=cpu(l64.grad), grad_values=cpu(v64.grad)), "float32", "float32", f"torch float64 side {s}")
    # separate logits (a view of a wider tensor) and values [n, 1]
    wide = {a: torch.zeros((n, A + 1), dtype=TORCH_LOGIT[dtype], device="cuda:0") for a in (A1, A2)}
    for a, c in zip((A1, A2), cases):
        wide[a][:, :A] = as_torch(c["logits"], dtype)
        wide[a][:, A] = as_torch(c["values"], dtype)
    leaves = {a: w.clone().requires_grad_(True) for a, w in wide.items()}
    vleaves = {a: as_torch(c["values"], dtype).reshape(n, 1).requires_grad_(True) for a, c in zip((A1, A2), cases)}
    loss, stats = ppo.loss({a: w[:, :A] for a, w in leaves.items()}, vleaves, **common)
    assert loss[A1].requires_grad and not stats["approx_kl"][A1].requires_grad and list(stats) == list(P.STAT_NAMES)
    (loss[A1] + 2.0 * loss[A2]).backward()
    torch.cuda.synchronize()
    for s, a in enumerate((A1, A2)):
        scale = 1.0 + s
        assert leaves[a].grad.dtype == TORCH_LOGIT[dtype] and (leaves[a].grad[:, A] == 0).all() and vleaves[a].grad.shape == (n, 1)
        got = dict(stats=np.array([float(stats[k][a]) for k in P.STAT_NAMES]), grad_logits=cpu(leaves[a].grad[:, :A].float()) / scale,
                   grad_values=cpu(vleaves[a].grad[:, 0].float()) / scale)
        check(judged[s], got, dtype, dtype, f"ppo.loss {dtype} {a}")
    # the fused head: one tensor in, one gradient of the same shape out, every column written
    heads = {a: w.clone().requires_grad_(True) for a, w in wide.items()}
    loss, stats = ppo.loss(head=heads, num_actions=A, **common)
    (loss[A1] + loss[A2]).backward()
    single, _ = ppo.loss(head=heads[A1].detach().clone().requires_grad_(True), num_actions=A, **{k: (v[A1] if isinstance(v, dict) else v) for k, v in common.items()})
    torch.cuda.synchronize()
    assert isinstance(single, torch.Tensor) and single.dim() == 0
    assert torch.equal(single.detach().view(torch.int32), loss[A1].detach().view(torch.int32))
    for s, a in enumerate((A1, A2)):
        g = heads[a].grad
        assert g.shape == (n, A + 1) and g.dtype == TORCH_LOGIT[dtype]
        got = dict(stats=np.array([float(stats[k][a]) for k in P.STAT_NAMES]), grad_logits=cpu(g[:, :A].float()), grad_values=cpu(g[:, A].float()))
        check(judged[s], got, dtype, dtype, f"ppo.loss fused {dtype} {a}")
    # loss_and_grad: out= reuse, then the capture of the pair of launches (moments + loss: a chain, no parallel branches)
    plain = {a: w.detach() for a, w in heads.items()}
    out = ppo.loss_and_grad(head=plain, num_actions=A, **common)
    torch.cuda.synchronize()
    eager = {a: (cpu(out["_stats"]).copy(), cpu(out["grad_head"][a].float()).copy()) for a in (A1, A2)}
    for s, a in enumerate((A1, A2)):
        assert np.array_equal(eager[a][1].view(np.uint32), cpu(heads[a].grad.float()).view(np.uint32))
        assert out["loss"][a].dim() == 0 and float(out["loss"][a]) == float(eager[a][0][s, 0])
    where = {a: out["grad_head"][a].data_ptr() for a in (A1, A2)}
    for a in (A1, A2):
        out["grad_head"][a].fill_(7.0)
    out["_stats"].fill_(7.0)
    again = ppo.loss_and_grad(head=plain, num_actions=A, out=out, **common)
    torch.cuda.synchronize()
    assert again is out and {a: out["grad_head"][a].data_ptr() for a in (A1, A2)} == where
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ppo.loss_and_grad(head=plain, num_actions=A, out=out, **common)
    assert captured is out
    torch.cuda.synchronize()
    for replay in range(2):
        for a in (A1, A2):
            out["grad_head"][a].fill_(7.0)
        out["_stats"].fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a in (A1, A2):
            assert np.array_equal(cpu(out["_stats"]).view(np.uint32), eager[a][0].view(np.uint32)), replay
            assert np.array_equal(cpu(out["grad_head"][a].float()).view(np.uint32), eager[a][1].view(np.uint32)), (replay, a)
    # errors before any launch: aliasing, a missing old_values, a wrong out
    for bad in (lambda: ppo.loss_and_grad(head=plain, num_actions=A, out={**out, "grad_head": plain}, **common),
                lambda: ppo.loss_and_grad(head=plain, num_actions=A, **{**common, "old_values": None}),
                lambda: ppo.loss_and_grad(head=plain, num_actions=A, **{**common, "clip": 1.0}),
                lambda: ppo.loss_and_grad(head=plain, num_actions=A + 1, **common),
                lambda: ppo.loss_and_grad(head=plain, num_actions=A, out={"grad_head": out["grad_head"]}, **common),
                lambda: ppo.loss_and_grad(head=plain[A1], num_actions=A, **common)):
        with pytest.raises(ValueError):
            bad()
