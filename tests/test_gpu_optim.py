"""GPU tests of the optimizer step (include/pikazoo_optim.h) against tests/optim_judge.py: the header's definition in float64
with a derived per-element tolerance (held to torch float64, a float32 restatement and seven mutants by
tests/test_optim_host.py).  Every step is judged from the state the previous one left on the device, so no tolerance ever
spans more than one step.  Every tensor is a view into a sentinel-filled buffer with guard elements in front and behind, the
step and statistics words included; gradients must keep their bits.  Every case runs through the C ABI and through
``pikazoo_amd.optim`` on copies of the same state, and the two must agree bit for bit.  Every test prints its worst
error / tolerance."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import optim_judge as J

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
DEV = "cuda"
GUARD, SENTINEL, WORD_SENTINEL = 8, -12345.0, -987654321
# elements in front of (param, grad, exp_avg, exp_avg_sq) of tensor i.  "aligned": 16-byte aligned views; "odd": odd element
# offsets, the four of a tensor alike (a scalar head, then 16-byte accesses); "mixed": offsets that differ (4-byte accesses)
FRONTS = {"aligned": lambda i: (8, 8, 8, 8), "odd": lambda i: (9 + 2 * (i % 4),) * 4, "mixed": lambda i: (9, 10 + i % 2, 11, 8)}


@pytest.fixture(scope="module")
def om():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    from pikazoo_amd import optim

    optim.load()
    return optim


class DeviceGroup:
    """a judge group (optim_judge.make_group) on the device, every tensor a view between guards"""

    def __init__(self, grp, mode="aligned"):
        self.buffers, self.fronts = [], []
        self.p, self.g, self.m, self.v = [], [], [], []
        for i in range(len(grp["p"])):
            for name, front in zip("pgmv", FRONTS[mode](i)):
                arr = grp[name][i]
                buf = torch.full((front + arr.size + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
                view = buf[front:front + arr.size].view(arr.shape)
                view.copy_(torch.from_numpy(arr))
                assert view.data_ptr() % 16 == (4 * front) % 16
                self.buffers.append(buf)
                self.fronts.append(front)
                getattr(self, name).append(view)
        self.step_buffer = torch.tensor([WORD_SENTINEL, grp["t"], grp["skipped"], WORD_SENTINEL], dtype=torch.int64, device=DEV)
        self.step = self.step_buffer[1:3]
        self.stats_buffer = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
        self.stats = self.stats_buffer[1:3]
        self.gradient_bits = None

    def set_gradients(self, grads):
        for view, arr in zip(self.g, grads):
            view.copy_(torch.from_numpy(arr))

    def numpy(self):
        words = self.step.cpu().numpy()
        return dict(p=[x.cpu().numpy() for x in self.p], g=[x.cpu().numpy() for x in self.g], m=[x.cpu().numpy() for x in self.m],
                    v=[x.cpu().numpy() for x in self.v], t=int(words[0]), skipped=int(words[1]), norm=float(self.stats[0]), coef=float(self.stats[1]))

    def assert_guards(self):
        for buf, front, view in zip(self.buffers, self.fronts, [x for quad in zip(self.p, self.g, self.m, self.v) for x in quad]):
            n = view.numel()
            assert bool((buf[:front] == SENTINEL).all()) and bool((buf[front + n:] == SENTINEL).all()), "a guard element was written"
        assert int(self.step_buffer[0]) == WORD_SENTINEL == int(self.step_buffer[3])
        assert float(self.stats_buffer[0]) == SENTINEL == float(self.stats_buffer[3])


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def same_bits(a, b):
    """two DeviceGroup.numpy() states are bit-equal (parameters, moments, step words, statistics; NaN payloads included)"""
    return (all(np.array_equal(bits(x), bits(y)) for name in "pmv" for x, y in zip(a[name], b[name])) and a["t"] == b["t"]
            and a["skipped"] == b["skipped"] and np.array_equal(bits(np.float32([a["norm"], a["coef"]])), bits(np.float32([b["norm"], b["coef"]]))))


def keyed(groups, what):
    """the argument of optim.adam_step: a sequence for one group, an {agent: sequence} dict for two"""
    return getattr(groups[0], what) if len(groups) == 1 else {f"agent_{a}": getattr(g, what) for a, g in enumerate(groups)}


def step_python(om, groups, kw, lr=None):
    kw = dict(kw)
    if lr is not None:
        kw["lr"] = lr
    om.adam_step(keyed(groups, "p"), keyed(groups, "g"), keyed(groups, "m"), keyed(groups, "v"), keyed(groups, "step"), stats=keyed(groups, "stats"), **kw)


def step_cabi(om, groups, kw, lr_tensor=None):
    o = J.options(**kw)
    array = (om.Group * om.MAX_GROUPS)()
    for a, grp in enumerate(groups):
        array[a].count = len(grp.p)
        for i, (p, g, m, v) in enumerate(zip(grp.p, grp.g, grp.m, grp.v)):
            array[a].tensors[i] = om.Tensor(p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
        array[a].step, array[a].stats = grp.step.data_ptr(), grp.stats.data_ptr()
        array[a].lr_device = lr_tensor.data_ptr() if lr_tensor is not None else None
    cfg = om.Config(o["lr"], o["beta1"], o["beta2"], o["eps"], o["wd"], o["max_norm"], int(o["decoupled"]), int(o["skip"]))
    code = om.load().pz_adam_step(array, len(groups), C.byref(cfg), torch.cuda.current_stream().cuda_stream)
    assert code == 0, code


def judged_step(om, groups, twins, kw, lr_value=None, lr_tensor=None):
    """One launch on `groups` through optim.adam_step and one on `twins` (equal state) through the C ABI; every group judged from
    the state it had.  Returns (worst share, elements beyond, [whether the clip engaged])."""
    o = J.options(**kw)
    before = [g.numpy() for g in groups]
    step_python(om, groups, kw, lr=lr_tensor)
    step_cabi(om, twins, kw, lr_tensor=lr_tensor)
    torch.cuda.synchronize()
    worst, beyond, engaged = 0.0, 0, []
    for grp, twin, was in zip(groups, twins, before):
        got, other = grp.numpy(), twin.numpy()
        grp.assert_guards()
        twin.assert_guards()
        assert same_bits(got, other), "the C ABI and optim.adam_step disagree"
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["g"], was["g"])), "a gradient was written"
        verdict = J.judge(was, o, lr_value)
        w, b = J.check_group(got, verdict)
        assert got["t"] == verdict["t"] and got["skipped"] == verdict["skipped"]
        if np.isfinite(verdict["norm"]):
            assert abs(got["norm"] - verdict["norm"]) <= verdict["e_norm"] and abs(got["coef"] - verdict["coef"]) <= verdict["e_coef"]
        else:
            assert not np.isfinite(got["norm"]) and (np.isnan(got["norm"]) == np.isnan(verdict["norm"]))
        worst, beyond = max(worst, w), beyond + b
        engaged.append(verdict["coef"] < 1)
    return worst, beyond, engaged


CASES = J.gpu_cases()


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_three_steps_of_every_shape_and_option(om, index):
    name, shapes, oname = CASES[index]
    kw = dict(J.OPTION_SETS)[oname]
    mode = "odd" if name == "odd_views" else ("mixed" if name == "sixteen_tensors" else "aligned")
    host = J.case_groups(index, shapes)
    groups, twins = [DeviceGroup(g, mode) for g in host], [DeviceGroup(g, mode) for g in host]
    worst, engaged = 0.0, []
    for step in range(J.STEPS):
        if step:
            for a, (grp, twin) in enumerate(zip(groups, twins)):
                fresh = J.case_gradients(index, a, step, host[a])
                grp.set_gradients(fresh)
                twin.set_gradients(fresh)
        w, beyond, e = judged_step(om, groups, twins, kw)
        assert not beyond, (name, step, w)
        assert all(int(g.step[0]) == step + 1 for g in groups)
        worst, engaged = max(worst, w), engaged + e
    print(f"{name}: worst error / tolerance {worst:.4f}; clip engaged in {sum(engaged)} of {len(engaged)} steps")
    if name == "default_net_clip_engaged":
        assert all(engaged)
    if name in ("default_net_clip_idle", "single_65"):
        assert not any(engaged)


def test_lr_from_a_device_tensor_that_changes_between_steps(om):
    kw = dict(lr=123.0, eps=1e-5, max_grad_norm=0.5)  # (the host lr is NOT used when a device lr is given)
    host = J.case_groups(50, [J.DEFAULT_NET])
    groups, twins = [DeviceGroup(g) for g in host], [DeviceGroup(g) for g in host]
    lr = torch.zeros((), dtype=torch.float32, device=DEV)
    worst = 0.0
    for value in (3e-4, 1e-2, 0.0):
        lr.fill_(value)
        before = groups[0].numpy()
        w, beyond, _ = judged_step(om, groups, twins, kw, lr_value=np.float32(value), lr_tensor=lr)
        assert not beyond
        worst = max(worst, w)
        moved = any(not np.array_equal(a, b) for a, b in zip(before["p"], groups[0].numpy()["p"]))
        assert moved == (value != 0.0)
    print(f"device lr: worst error / tolerance {worst:.4f}")


@pytest.mark.parametrize("t", J.PLANTED_T)
def test_planted_step_counts(om, t):
    """the bias corrections come from the int64 t in float64; betas whose powers are still alive at t = 10^6"""
    kw = dict(lr=3e-4, betas=J.PLANTED_BETAS, eps=1e-8, max_grad_norm=0.5)
    host = J.case_groups(70, [J.DEFAULT_NET], t)
    groups, twins = [DeviceGroup(g) for g in host], [DeviceGroup(g) for g in host]
    w, beyond, _ = judged_step(om, groups, twins, kw)
    assert not beyond and int(groups[0].step[0]) == t + 1
    bc1, bc2 = J.bias_corrections(J.options(**kw), t + 1)
    print(f"t = {t}: bias corrections {bc1:.6g}, {bc2:.6g}; worst error / tolerance {w:.4f}")


def test_exact_pin(om):
    host, o, want = J.exact_pin_case()
    kw = dict(lr=float(o["lr"]), betas=(0.5, 0.75), eps=0.0)
    for mode in FRONTS:
        groups, twins = [DeviceGroup(host, mode)], [DeviceGroup(host, mode)]
        step_python(om, groups, kw)
        step_cabi(om, twins, kw)
        torch.cuda.synchronize()
        got, other = groups[0].numpy(), twins[0].numpy()
        groups[0].assert_guards()
        assert same_bits(got, other) and got["t"] == 1 and got["skipped"] == 0 and got["coef"] == 1.0
        for name in "pmv":
            for g, w in zip(got[name], want[name]):
                assert np.array_equal(bits(g), bits(w)), (mode, name)
        for g, was in zip(got["p"], host["p"]):
            assert np.array_equal(np.abs(g.astype(np.float64) - was), np.full(g.shape, float(o["lr"])))


def test_zero_gradient_with_eps(om):
    """parameters keep their bits, exp_avg_sq decays by beta2 exactly, exp_avg (at zero) stays; grad_norm is +0 and clip_coef 1"""
    def planted(live_first_moment):
        grp = J.make_group(8, J.DEFAULT_NET, 1.0, t=3)  # (moments as after three steps: exp_avg_sq > 0 everywhere)
        for g, m in zip(grp["g"], grp["m"]):
            g[...] = 0
            if not live_first_moment:
                m[...] = 0
        assert all((v > 0).all() for v in grp["v"])
        return grp

    host = planted(False)
    kw = dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    groups, twins = [DeviceGroup(host)], [DeviceGroup(host)]
    w, beyond, _ = judged_step(om, groups, twins, kw)
    got = groups[0].numpy()
    assert not beyond
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["p"], host["p"]))
    assert all(np.array_equal(a, np.float32(0.999) * b) and (a < b).all() for a, b in zip(got["v"], host["v"]))
    assert all(not a.any() for a in got["m"])
    assert got["norm"] == 0.0 and not np.signbit(np.float32(got["norm"])) and got["coef"] == 1.0 and got["t"] == 4
    # with live first moments the judge decides: they decay, and the parameters follow them
    host = planted(True)
    groups, twins = [DeviceGroup(host)], [DeviceGroup(host)]
    w2, beyond, _ = judged_step(om, groups, twins, kw)
    assert not beyond
    assert all((np.abs(a) < np.abs(b)).all() for a, b in zip(groups[0].numpy()["m"], host["m"]))
    print(f"zero gradient: worst error / tolerance {max(w, w2):.4f}")


@pytest.mark.parametrize("skip", (False, True), ids=("default", "skip_nonfinite"))
@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_nan_and_infinity_stay_in_their_group(om, bad, skip):
    """One bad gradient element in group 1 of 2.  By default the definition runs: under the clip a NaN makes coef NaN and the
    whole group NaN; an infinity makes coef 0, that element NaN (0 * inf) and the others see a zero gradient -- the judge
    decides, class for class.  With skip_nonfinite group 1 keeps its bits.  Group 2 is judged as ever and is bit-equal to its
    run alone."""
    kw = dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5, skip_nonfinite=skip)
    host = J.case_groups(60, [J.DEFAULT_NET, J.LARGEST_BOX], t=2)
    host[0]["g"][2][17, 5] = bad
    groups, twins = [DeviceGroup(g) for g in host], [DeviceGroup(g) for g in host]
    alone, alone_twin = [DeviceGroup(host[1])], [DeviceGroup(host[1])]
    w, beyond, _ = judged_step(om, groups, twins, kw)
    w1, beyond1, _ = judged_step(om, alone, alone_twin, kw)
    assert not beyond and not beyond1
    got = groups[0].numpy()
    assert not np.isfinite(got["norm"])
    if skip:
        assert got["t"] == 2 and got["skipped"] == 1
        assert all(np.array_equal(bits(a), bits(b)) for name in "pmv" for a, b in zip(got[name], host[0][name]))
    else:
        assert got["t"] == 3 and got["skipped"] == 0
        flat = np.concatenate([x.reshape(-1) for name in "pmv" for x in got[name]])
        if np.isnan(bad):
            assert np.isnan(flat).all() and np.isnan(got["coef"])
        else:
            assert got["coef"] == 0.0 and np.isnan(flat).sum() == 3 and all(np.isnan(got[name][2][17, 5]) for name in "pmv")
    second = groups[1].numpy()
    assert np.isfinite(second["norm"]) and second["t"] == 3 and second["skipped"] == 0
    assert same_bits(second, alone[0].numpy())
    print(f"bad = {bad}, skip = {skip}: worst error / tolerance {max(w, w1):.4f}")


def test_bit_equality(om):
    kw = dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5, weight_decay=0.01)
    host = J.case_groups(61, [tuple((n,) for n in J.ODD_VIEWS) + J.DEFAULT_NET, J.LARGEST_BOX], t=5)
    results = {}
    for name, mode, both in (("first", "aligned", True), ("again", "aligned", True), ("odd", "odd", True), ("mixed", "mixed", True),
                             ("alone", "aligned", False)):
        groups = [DeviceGroup(g, mode) for g in (host if both else host[:1])]
        for step in range(2):
            (step_python if name != "again" else step_cabi)(om, groups, kw)
        torch.cuda.synchronize()
        for g in groups:
            g.assert_guards()
        results[name] = [g.numpy() for g in groups]
    for name in ("again", "odd", "mixed"):
        assert all(same_bits(a, b) for a, b in zip(results["first"], results[name])), name     # equal state; views at any offset
    assert same_bits(results["first"][0], results["alone"][0])                                # group 1 without group 2
    # own allocations (what torch hands out) against the views above, and optim.Adam against the functional form
    params = [torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in host[1]["p"]]
    opt = om.Adam(params, **kw)
    for p, m, v in zip(params, host[1]["m"], host[1]["v"]):
        opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = torch.from_numpy(m).to(DEV), torch.from_numpy(v).to(DEV)
    opt.state[params[0]]["step"] = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    for p, g in zip(params, host[1]["g"]):
        p.grad = torch.from_numpy(g).to(DEV)
    for step in range(2):
        opt.step()
    torch.cuda.synchronize()
    want = results["first"][1]
    assert int(opt.steps) == 7 == want["t"] and int(opt.skipped) == 0
    assert np.array_equal(bits(np.float32([float(opt.stats["grad_norm"]), float(opt.stats["clip_coef"])])), bits(np.float32([want["norm"], want["coef"]])))
    for p, wp, wm, wv in zip(params, want["p"], want["m"], want["v"]):
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(wp))
        assert np.array_equal(bits(opt.state[p]["exp_avg"].cpu().numpy()), bits(wm)) and np.array_equal(bits(opt.state[p]["exp_avg_sq"].cpu().numpy()), bits(wv))


def drive(opt, params, seeds):
    for seed in seeds:
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for p in params:
            p.grad = (0.02 * torch.randn(p.shape, generator=gen)).to(DEV)
        opt.step()


def test_state_dict_round_trip(om):
    """3 steps, state_dict() into a fresh instance, 2 more: bit-equal to 5 steps straight; two param groups, one launch; a
    parameter without a gradient is left out"""
    def make():
        gen = torch.Generator(device="cpu").manual_seed(3)
        first = [torch.nn.Parameter((0.1 * torch.randn(s, generator=gen)).to(DEV)) for s in J.DEFAULT_NET]
        second = [torch.nn.Parameter((0.1 * torch.randn(s, generator=gen)).to(DEV)) for s in ((33, 7), (5,))]
        idle = torch.nn.Parameter(torch.ones(4, device=DEV))
        opt = om.Adam([{"params": first + [idle]}, {"params": second}], lr=1e-3, eps=1e-5, max_grad_norm=0.5, weight_decay=0.01, decoupled=True)
        return opt, first + second, idle

    straight, ps, idle = make()
    drive(straight, ps, range(5))
    a, pa, idle_a = make()
    drive(a, pa, range(3))
    b, pb, idle_b = make()
    with torch.no_grad():
        for p, q in zip(pb, pa):
            p.copy_(q)
    b.load_state_dict(a.state_dict())
    drive(b, pb, range(3, 5))
    torch.cuda.synchronize()
    assert [int(x) for x in straight.steps] == [5, 5] == [int(x) for x in b.steps] and [int(x) for x in b.skipped] == [0, 0]
    for p, q in zip(ps, pb):
        assert torch.equal(p, q) and not torch.equal(p, torch.zeros_like(p))
        for key in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(bits(straight.state[p][key].cpu().numpy()), bits(b.state[q][key].cpu().numpy()))
    assert torch.equal(idle, torch.ones_like(idle)) and "exp_avg" not in straight.state[idle] and torch.equal(idle_b, torch.ones_like(idle))
    assert float(straight.stats["grad_norm"][0]) > 0 and 0 < float(straight.stats["clip_coef"][1]) <= 1


def test_a_captured_graph_holds_a_whole_minibatch_update(om):
    """net.forward -> ppo.loss_and_grad(head=) -> netgrad.backward -> optim.adam_step at 256 rows in one graph: 4 replays are
    bit-equal to 4 eager repetitions, the parameters move between replays, and t == 4 afterwards"""
    from pikazoo_amd import net, netgrad, ppo

    torch.manual_seed(2)
    n, A = 256, 18
    obs = {k: torch.rand(n, 35, device=DEV) for k in "ab"}
    act = {k: torch.randint(0, A, (n,), device=DEV, dtype=torch.int32) for k in "ab"}
    old = {k: torch.full((n,), -2.9, device=DEV) for k in "ab"}
    adv = {k: torch.randn(n, device=DEV) for k in "ab"}
    ret = {k: torch.randn(n, device=DEV) for k in "ab"}
    start = [p.detach().clone() for p in net.ActorCritic().to(DEV).parameter_tensors()]

    class Learner:
        def __init__(self):
            self.P = [p.clone() for p in start]
            self.m, self.v = [torch.zeros_like(p) for p in start], [torch.zeros_like(p) for p in start]
            self.step, self.stats = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, device=DEV)
            self.ws = netgrad.workspace(n, 35, 64, 19, DEV)
            self.head = self.loss = self.grads = None

        def update(self):
            self.head = net.forward(obs, self.P, out=self.head)
            self.loss = ppo.loss_and_grad(actions=act, old_log_probs=old, advantages=adv, returns=ret, head=self.head, num_actions=A, out=self.loss)
            self.grads = netgrad.backward(obs, self.P, self.loss["grad_head"], out=self.grads, workspace=self.ws)
            om.adam_step(self.P, list(self.grads), self.m, self.v, self.step, lr=1e-2, eps=1e-5, max_grad_norm=0.5, stats=self.stats)

        def reset(self):
            for dst, src in zip(self.P, start):
                dst.copy_(src)
            for t in self.m + self.v + [self.step, self.stats]:
                t.zero_()

    eager = Learner()
    trail = []
    for _ in range(4):
        eager.update()
        trail.append([p.clone() for p in eager.P])
    captured = Learner()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        captured.update()  # (allocates the outputs; it moves the parameters, which reset() puts back)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured.update()
    torch.cuda.current_stream().wait_stream(stream)
    captured.reset()
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured.P, trail[k])), k
    assert not any(torch.equal(a, b) for a, b in zip(trail[0], trail[1]))
    assert captured.step.tolist() == [4, 0] == eager.step.tolist()
    assert all(torch.equal(a, b) for a, b in zip(captured.m + captured.v + [captured.stats], eager.m + eager.v + [eager.stats]))


def test_agreement_with_torch_on_the_device(om):
    """torch.optim.Adam behind clip_grad_norm_ in float32, 3 steps on the default net, beside ours on the same gradients: each
    is judged from its OWN previous state, and both stay within the judge's tolerance"""
    kw = dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    o = J.options(**kw)
    host = J.case_groups(62, [J.DEFAULT_NET])[0]
    ours = om.Adam([torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in host["p"]], **kw)
    theirs_p = [torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in host["p"]]
    theirs = torch.optim.Adam(theirs_p, lr=3e-4, eps=1e-5)
    ours_p = ours.param_groups[0]["params"]
    shares = {}
    for step in range(3):
        grads = host["g"] if step == 0 else J.case_gradients(62, 0, step, host)
        for name, opt, ps in (("ours", ours, ours_p), ("torch", theirs, theirs_p)):
            zeros = [np.zeros(p.shape, np.float32) for p in ps]
            state = [opt.state[p] for p in ps]
            was = dict(p=[p.detach().cpu().numpy() for p in ps], g=grads, t=step, skipped=0,
                       m=[s["exp_avg"].cpu().numpy() if "exp_avg" in s else z for s, z in zip(state, zeros)],
                       v=[s["exp_avg_sq"].cpu().numpy() if "exp_avg_sq" in s else z for s, z in zip(state, zeros)])
            for p, g in zip(ps, grads):
                p.grad = torch.from_numpy(g).to(DEV)
            if name == "torch":
                torch.nn.utils.clip_grad_norm_(ps, 0.5)
            opt.step()
            torch.cuda.synchronize()
            got = dict(p=[p.detach().cpu().numpy() for p in ps], m=[opt.state[p]["exp_avg"].cpu().numpy() for p in ps],
                       v=[opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ps])
            verdict = J.judge(was, o)
            assert verdict["coef"] < 1
            w, beyond = J.check_group(got, verdict)
            shares[name] = max(shares.get(name, 0.0), w)
            assert not beyond, (name, step, w)
    print(f"worst error / tolerance: ours {shares['ours']:.4f}, torch {shares['torch']:.4f}")


def test_the_example_runs_on_both_optimizer_routes():
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    logs = [ppo_selfplay.main(num_envs=256, iters=2, steps=8, native_optimizer=flag, log=lambda line: None) for flag in (True, False)]
    for log in logs:
        assert len(log) == len(logs[0]) > 0 and all(np.isfinite(entry) for entry in log)
