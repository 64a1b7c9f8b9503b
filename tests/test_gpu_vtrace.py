"""GPU tests (``-m gpu``) of ``pz_vtrace`` (include/pikazoo_vtrace.h, the ``pz_vt::vtrace_kernel`` family) and of
``pikazoo_amd.vtrace.targets``.

The judge is tests/vtrace_judge.py (held to exact rational arithmetic, to the float64 formula and to GAE's judge by
tests/test_vtrace_host.py); no GPU result is ever the expected value, with ONE exception that is the point of its test: on-policy
the launch is compared with ``pz_gae`` on the same device buffers, and ``pz_gae`` itself with its own judge in the same test.
  * EXACT cases (every weight 1, 0 or its clip, whatever the device's expf): compared BIT FOR BIT through uint32 views.
  * TOLERANCE cases (random log-ratios): compared with the float64 formula within the tolerance derived per element in the judge.
Every C-ABI launch goes into sentinel-filled outputs with columns beyond n and a tail behind every buffer, which must keep the
sentinel; the inputs must be unchanged; a second launch must give the same bits.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import gae_judge as GJ
import vtrace_judge as J

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
A1, A2 = "player_1", "player_2"
SENT = -7   # the int32 pattern the outputs hold before a launch (as float32 a NaN no arithmetic here produces)
TAIL = 64   # elements behind the last row of every buffer
TORCH_VALUE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def cpu(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import vtrace

    return vtrace.load()


def device_rows(host, pitch, fill):
    """host [rows, n] -> a flat device tensor of rows * pitch + TAIL elements holding it at `pitch`, `fill` elsewhere"""
    rows, n = host.shape
    flat = np.full(rows * pitch + TAIL, fill, host.dtype)
    flat[:rows * pitch].reshape(rows, pitch)[:, :n] = host
    if flat.dtype == np.uint16:  # (bfloat16 patterns: the launch takes a pointer, torch an integer type it knows)
        flat = flat.view(np.int16)
    return torch.from_numpy(flat).to("cuda:0")


class Launch:
    """one case's inputs on the device at the spec's pitches, and pz_vtrace over them into fresh sentinel-filled outputs"""

    def __init__(self, c, s):
        self.c, self.s = c, s
        self.k, self.n = c["k"], c["n"]
        self.rp, self.tp, self.vp, self.lp, self.op = s["pitches"]
        self.sides = 2 if s["both"] else 1
        self.rew = [device_rows(np.ascontiguousarray(r), self.rp, r.dtype.type(9)) for r in c["rew"][:self.sides]]
        self.val = [device_rows(GJ.value_bits(v, s["vf"]), self.vp, GJ.value_bits(v, s["vf"]).dtype.type(3)) for v in c["val"][:self.sides]]
        self.lpb = [device_rows(x, self.lp, np.float32(np.nan)) for x in c["lpb"][:self.sides]]
        self.lpt = [device_rows(x, self.lp, np.float32(np.nan)) for x in c["lpt"][:self.sides]]
        self.term = device_rows(c["d"], self.tp, np.uint8(1))
        self.inputs = self.rew + self.val + self.lpb + self.lpt + [self.term]
        self.before = [cpu(t).copy() for t in self.inputs]
        self.formats = (J.REWARD_DTYPES.index(s["rf"]), J.VALUE_DTYPES.index(s["vf"]))

    def fresh(self, count):
        return [torch.full((self.k * self.op + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(count)]

    @staticmethod
    def pair(ts):
        return ts[0].data_ptr(), (ts[1].data_ptr() if len(ts) == 2 else None)

    def vtrace(self, lib, gamma=None, lam=None, clips=None):
        """[pg_adv per side ..., vs per side ...] as int32 host arrays of the whole buffers"""
        s = self.s
        outs = self.fresh(2 * self.sides)
        pg, vs = outs[:self.sides], outs[self.sides:]
        err = lib.pz_vtrace(*self.pair(self.rew), self.formats[0], self.term.data_ptr(), *self.pair(self.val), self.formats[1], *self.pair(self.lpb),
                            *self.pair(self.lpt), self.k, self.n, self.rp, self.tp, self.vp, self.lp, self.op, s["gamma"] if gamma is None else gamma,
                            s["lam"] if lam is None else lam, *(s["clips"] if clips is None else clips), *self.pair(vs), *self.pair(pg),
                            torch.cuda.current_stream().cuda_stream)
        assert err == 0
        torch.cuda.synchronize()
        return [cpu(o) for o in outs]

    def gae(self, gamma, lam):
        """pz_gae over the SAME device buffers: [adv per side ..., ret per side ...]"""
        from pikazoo_amd import learn

        outs = self.fresh(2 * self.sides)
        adv, ret = outs[:self.sides], outs[self.sides:]
        err = learn.load().pz_gae(*self.pair(self.rew), self.formats[0], self.term.data_ptr(), *self.pair(self.val), self.formats[1], self.k, self.n,
                                  self.rp, self.tp, self.vp, self.op, gamma, lam, *self.pair(adv), *self.pair(ret), torch.cuda.current_stream().cuda_stream)
        assert err == 0
        torch.cuda.synchronize()
        return [cpu(o) for o in outs]

    def rows(self, flat):
        """the [k, n] payload of an output buffer; the columns beyond n and the tail must still hold the sentinel"""
        body = flat[:self.k * self.op].reshape(self.k, self.op)
        assert (body[:, self.n:] == SENT).all() and (flat[self.k * self.op:] == SENT).all(), "a launch wrote outside its rows"
        return body[:, :self.n]

    def inputs_unchanged(self):
        for t, b in zip(self.inputs, self.before):
            assert cpu(t).tobytes() == b.tobytes(), "an input changed"  # (as bytes: a planted NaN equals itself)


def check_exact(lib, s, c=None, nan_rows=()):
    """one spec of the judge's table through the C ABI, twice, against judge32 bit for bit; `nan_rows`: rows that the case makes
    NaN somewhere -- a NaN that arithmetic produces has no pinned sign or payload, so their elements must be NaN where the
    judge's are and its bits elsewhere"""
    c = J.case_of(s) if c is None else c
    run = Launch(c, s)
    first, second = run.vtrace(lib), run.vtrace(lib)
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "two launches differ"
    keep = [t for t in range(run.k) if t not in nan_rows]
    for side in range(run.sides):
        want = J.judge32(c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side], s["gamma"], s["lam"], s["clips"])
        for got, ref, what in ((first[side], want[0], "advantages"), (first[run.sides + side], want[1], "returns")):
            rows = run.rows(got)
            assert np.array_equal(rows[keep].view(np.uint32), bits(ref[keep])), (s, side, what)
            for t in nan_rows:
                have, nan = rows[t].view(np.float32), np.isnan(ref[t])
                assert nan.any() and np.array_equal(np.isnan(have), nan) and np.array_equal(have[~nan].view(np.uint32), bits(ref[t][~nan])), (s, side, what, t)
    run.inputs_unchanged()


@pytest.mark.parametrize("test", [t for t in J.EXACT])
def test_exact_cases(lib, test):
    """the judge's table (tests/vtrace_judge.py: EXACT) -- every k of K_EDGES at n = 200, every n of N_EDGES at k = 33, the six
    flag patterns, the six formats, one side only, five different pitches, pitch == n, gamma and lam at 0 and 1, each clip at 0
    and at 4, and 1 563 workgroups per agent -- with clip_rho != clip_c != clip_pg_rho throughout"""
    for s in J.EXACT[test]:
        check_exact(lib, s)


def test_a_nan_log_prob_stays_in_its_episode(lib):
    """NaN weights pass the three selects as NaN (a minimum would make them the clip) and stop at the episode end"""
    c, nan_rows = J.nan_case()
    check_exact(lib, J.spec(9, 65), c, nan_rows)


def test_nothing_crosses_an_episode_end(lib):
    """non-finite values AND log-probs behind a flagged row: the rows in front of the flag keep the judge's finite bits"""
    s = J.spec(9, 65, "none", seed=8)
    c = J.case_of(s)
    c["d"][4] = 1
    for v, lpb, lpt in zip(c["val"], c["lpb"], c["lpt"]):
        v[5, ::2], v[5, 1::2] = np.inf, np.nan
        lpt[5, ::3], lpb[5, 1::3] = np.nan, np.nan
    check_exact(lib, s, c, nan_rows=(5,))
    pg, vs = J.judge32(c["rew"][0], c["d"], c["val"][0], c["lpb"][0], c["lpt"][0])
    assert np.isfinite(pg[:5]).all() and np.isfinite(vs[:5]).all() and np.isnan(vs[5]).all() and np.isfinite(vs[6:]).all()


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_on_policy_equals_pz_gae_on_the_same_device_buffers_bit_for_bit(lib, lam):
    """target = behaviour (the same bits), clips >= 1: vs is pz_gae's ret and pg_adv its adv.  What it shows: the
    ``(d == 0) ? 1 : expf(d)`` select and the no-FMA order survived the compiler.  pz_gae's own result is held to its judge here
    too, so the yardstick is not taken on trust."""
    for k, n, pattern, rf, vf, clips in ((33, 200, "random10", "float32", "float32", (1.0, 1.0, 1.0)), (130, 65, "random50", "int32", "bfloat16", (1.0, 2.5, 4.0)),
                                         (7, 63, "none", "float32", "float16", (4.0, 1.0, 1.5)), (16, 64, "last_row", "int32", "float32", (1.0, 1.0, 1.0))):
        s = J.spec(k, n, pattern, rf, vf, seed=12, pitches=(256, 320, 208, 232, 264), lam=lam, clips=clips)
        c = J.case_of(s, "on_policy")
        run = Launch(c, s)
        ours, gae = run.vtrace(lib), run.gae(s["gamma"], lam)
        for side in range(2):
            adv, ret = GJ.judge(c["rew"][side], c["d"], c["val"][side], s["gamma"], lam)
            for i, want in ((side, adv), (2 + side, ret)):
                assert np.array_equal(run.rows(gae[i]).view(np.uint32), bits(want)), (s, side, i)
                assert np.array_equal(run.rows(ours[i]), run.rows(gae[i])), (s, side, i)
        run.inputs_unchanged()


@pytest.mark.parametrize("s", J.TOLERANCE, ids=lambda s: f"k{s['k']}-{s['rf']}-{s['vf']}")
def test_random_log_ratios_against_the_float64_formula(lib, s):
    c = J.case_of(s, "random")
    run = Launch(c, s)
    got = run.vtrace(lib)
    for side in range(2):
        pg64, vs64, tol_pg, tol_vs = J.judge64(c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side], s["gamma"], s["lam"], s["clips"])
        used = (J.worst_share(run.rows(got[side]).view(np.float32), pg64, tol_pg), J.worst_share(run.rows(got[2 + side]).view(np.float32), vs64, tol_vs))
        print(f"k={s['k']} {s['rf']}/{s['vf']} side {side}: the kernel uses {used[0]:.3f} (advantages) and {used[1]:.3f} (returns) of the tolerance")
        assert max(used) <= 1, (s, side, used)
    run.inputs_unchanged()


# ---- the binding -----------------------------------------------------------------------------------------------------------------
def on_device(c, vf="float32"):
    t = {}
    for key in ("rew", "val", "lpb", "lpt"):
        t[key] = {a: torch.from_numpy(x).to("cuda:0") for a, x in zip((A1, A2), c[key])}
    t["val"] = {a: v.to(TORCH_VALUE[vf]) for a, v in t["val"].items()}
    t["d"] = torch.from_numpy(c["d"]).to("cuda:0")
    return t


def judged(c, side, **kw):
    return J.judge32(c["rew"][side], c["d"], c["val"][side], c["lpb"][side], c["lpt"][side], **kw)


def test_dicts_single_tensors_flag_types_and_out_reuse():
    from pikazoo_amd import vtrace

    c = J.make_case(33, 200, "random10", "int32", "bfloat16", seed=13)
    t = on_device(c, "bfloat16")
    kw = dict(gamma=0.97, lam=0.9, clip_rho=1.5, clip_c=0.75, clip_pg_rho=3.0)
    out = vtrace.targets(t["rew"], t["val"], t["d"].view(torch.bool), t["lpb"], t["lpt"], **kw)
    torch.cuda.synchronize()
    assert list(out) == ["advantages", "returns"] and list(out["advantages"]) == [A1, A2] == list(out["returns"])
    for side, a in enumerate((A1, A2)):
        pg, vs = judged(c, side, gamma=0.97, lam=0.9, clips=(1.5, 0.75, 3.0))
        assert np.array_equal(bits(cpu(out["advantages"][a])), bits(pg)) and np.array_equal(bits(cpu(out["returns"][a])), bits(vs)), a
    # one side as bare tensors, uint8 flags, a dict of the one flag tensor; the defaults are lam = 1 and clips of 1
    one = vtrace.targets(t["rew"][A2], t["val"][A2], t["d"], t["lpb"][A2], t["lpt"][A2])
    torch.cuda.synchronize()
    pg, vs = judged(c, 1, gamma=0.99, lam=1.0, clips=(1.0, 1.0, 1.0))
    assert isinstance(one["advantages"], torch.Tensor) and np.array_equal(bits(cpu(one["advantages"])), bits(pg)) and np.array_equal(bits(cpu(one["returns"])), bits(vs))
    keep = {key: {a: x.data_ptr() for a, x in out[key].items()} for key in out}
    for key in out:
        for x in out[key].values():
            x.fill_(float("nan"))
    again = vtrace.targets(t["rew"], t["val"], {A1: t["d"], A2: t["d"]}, t["lpb"], t["lpt"], out=out, **kw)
    torch.cuda.synchronize()
    assert again is out and keep == {key: {a: x.data_ptr() for a, x in out[key].items()} for key in out}
    for side, a in enumerate((A1, A2)):
        pg, vs = judged(c, side, gamma=0.97, lam=0.9, clips=(1.5, 0.75, 3.0))
        assert np.array_equal(bits(cpu(out["advantages"][a])), bits(pg)) and np.array_equal(bits(cpu(out["returns"][a])), bits(vs)), a
    # the result drops into learn.gae's place: on-policy it is learn.gae's
    from pikazoo_amd import learn

    gae = learn.gae(t["rew"], t["val"], t["d"], 0.99, 0.95)
    same = vtrace.targets(t["rew"], t["val"], t["d"], t["lpb"], t["lpb"], 0.99, 0.95)
    torch.cuda.synchronize()
    for key in gae:
        for a in (A1, A2):
            assert torch.equal(gae[key][a].view(torch.int32), same[key][a].view(torch.int32)), (key, a)


def test_row_strides():
    """views with row strides of their own: every second row of a taller tensor, column windows, an out= of wider rows"""
    from pikazoo_amd import vtrace

    c = J.make_case(17, 200, "random10", "int32", "float16", seed=14)
    k, n = c["k"], c["n"]
    big_r = torch.zeros((2 * k, n + 8), dtype=torch.int32, device="cuda:0")
    big_v = torch.zeros((k + 1, n + 24), dtype=torch.float16, device="cuda:0")
    big_lp = torch.zeros((2, k, n + 40), dtype=torch.float32, device="cuda:0")
    big_out = torch.full((2, k, n + 16), float("nan"), dtype=torch.float32, device="cuda:0")
    r, v, lpb, lpt = big_r[::2, 8:], big_v[:, 3:n + 3], big_lp[0, :, 5:n + 5], big_lp[1, :, 5:n + 5]
    for dst, src in ((r, c["rew"][0]), (v, c["val"][0]), (lpb, c["lpb"][0]), (lpt, c["lpt"][0])):
        dst.copy_(torch.from_numpy(src))
    d = torch.from_numpy(c["d"]).to("cuda:0")
    pg, vs = judged(c, 0)
    out = vtrace.targets(r, v, d, lpb, lpt, J.GAMMA, J.LAM, *J.CLIPS, out={"advantages": big_out[0, :, :n], "returns": big_out[1, :, :n]})
    torch.cuda.synchronize()
    assert np.array_equal(bits(cpu(out["advantages"])), bits(pg)) and np.array_equal(bits(cpu(out["returns"])), bits(vs))
    assert torch.isnan(big_out[:, :, n:]).all()


def test_graph_capture_replays_to_the_eager_bits():
    from pikazoo_amd import vtrace

    c = J.make_case(33, 200, "random10", seed=15)
    t = on_device(c)
    d = t["d"].view(torch.bool)
    args = (t["rew"], t["val"], d, t["lpb"], t["lpt"], J.GAMMA, J.LAM, *J.CLIPS)
    eager = vtrace.targets(*args)
    torch.cuda.synchronize()
    want = {key: {a: cpu(x).copy() for a, x in eager[key].items()} for key in eager}
    prev = vtrace.targets(*args)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = vtrace.targets(*args, out=prev)
    assert captured is prev
    torch.cuda.synchronize()
    for key in prev:
        for x in prev[key].values():
            x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for side, a in enumerate((A1, A2)):
        pg, vs = judged(c, side)
        for key, ref in (("advantages", pg), ("returns", vs)):
            assert np.array_equal(bits(cpu(prev[key][a])), bits(want[key][a])) and np.array_equal(bits(want[key][a]), bits(ref)), (key, a)


def test_mismatched_shapes_devices_dtypes_strides_ranges_and_agents_raise_value_error():
    from pikazoo_amd import vtrace

    dev = "cuda:0"
    r, v, d = torch.zeros(4, 8, device=dev), torch.zeros(5, 8, device=dev), torch.zeros(4, 8, dtype=torch.bool, device=dev)
    lp, lq = torch.zeros(4, 8, device=dev), torch.zeros(4, 8, device=dev)
    good = vtrace.targets(r, v, d, lp, lq)
    wide = torch.zeros(4, 16, device=dev)
    T = vtrace.targets
    bad = [lambda: T(r, torch.zeros(4, 8, device=dev), d, lp, lq),                 # values need k + 1 rows
           lambda: T(r, v, torch.zeros(4, 9, dtype=torch.bool, device=dev), lp, lq),
           lambda: T(r, v, d, torch.zeros(5, 8, device=dev), lq),
           lambda: T(r, v, d, lp, torch.zeros(4, 7, device=dev)),
           lambda: T(torch.zeros(0, 8, device=dev), v, d, lp, lq),
           lambda: T(r, v.cpu(), d, lp, lq),                                          # another device
           lambda: T(r, v, d.cpu(), lp, lq),
           lambda: T(r, v, d, lp.cpu(), lq),
           lambda: T(r, v, d, lp, lq.cpu()),
           lambda: T(r.to(torch.float64), v, d, lp, lq),                              # dtypes
           lambda: T(r, v.to(torch.float64), d, lp, lq),
           lambda: T(r, v, d.to(torch.int32), lp, lq),
           lambda: T(r, v, d, lp.to(torch.float16), lq),
           lambda: T(r, v, d, lp, lq.to(torch.float64)),
           lambda: T({A1: r, A2: r.to(torch.int32)}, {A1: v, A2: v}, d, {A1: lp, A2: lp}, {A1: lq, A2: lq}),
           lambda: T(r, v, d, lp, lq, gamma=1.5),                                     # ranges
           lambda: T(r, v, d, lp, lq, lam=float("nan")),
           lambda: T(r, v, d, lp, lq, lam=-0.1),
           lambda: T(r, v, d, lp, lq, clip_rho=-1.0),
           lambda: T(r, v, d, lp, lq, clip_c=float("inf")),
           lambda: T(r, v, d, lp, lq, clip_pg_rho=float("nan")),
           lambda: T(r, v, d, lp, lq, clip_rho=1e39),
           lambda: T(r.t().contiguous().t(), v, d, lp, lq),                           # the last dimension must be contiguous
           lambda: T(r, v, d, lp.t().contiguous().t(), lq),
           lambda: T(r, v, d, lp, wide[:, :8]),                                       # the log-probs share one row stride
           lambda: T(r, v, d, lp[:1].expand(4, 8), lq),                  # rows overlap
           lambda: T({A1: r}, {A2: v}, d, {A1: lp}, {A1: lq}),                        # the agents
           lambda: T({A1: r}, {A1: v}, d, lp, {A1: lq}),
           lambda: T({A1: r, A2: r}, {A1: v, A2: v}, {A1: d, A2: d.clone()}, {A1: lp, A2: lp}, {A1: lq, A2: lq}),
           lambda: T(r, v, d, lp, lq, out={"advantages": torch.zeros(4, 9, device=dev), "returns": torch.zeros(4, 8, device=dev)}),   # out=
           lambda: T(r, v, d, lp, lq, out={"advantages": torch.zeros(4, 8, device=dev)}),
           lambda: T(r, v, d, lp, lq, out={"advantages": {A1: good["advantages"]}, "returns": good["returns"]}),
           lambda: T(r, v, d, lp, lq, out={"advantages": good["advantages"], "returns": good["advantages"]}),     # outputs alias each other
           lambda: T(r, v, d, lp, lq, out={"advantages": lp, "returns": good["returns"]}),                        # ... or an input
           lambda: T(r, v, d, lp, lq, out=good["advantages"])]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")


def test_the_example_with_and_without_vtrace():
    """without the flag the example is what it was (the default IS the flag off, and tests/test_gpu_net.py and its neighbours hold
    that run); with it the later epochs use other targets: finite losses that differ from the second minibatch epoch on"""
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    kw = dict(num_envs=256, iters=2, steps=8, log=lambda line: None)
    plain = ppo_selfplay.main(**kw)
    off = ppo_selfplay.main(vtrace=False, **kw)
    on = ppo_selfplay.main(vtrace=True, **kw)
    assert plain == off and len(on) == len(off) == 2 * 2 * 4
    assert all(np.isfinite(on)) and all(np.isfinite(off))
    assert on[:4] == off[:4] and on[4:8] != off[4:8]          # the first epoch keeps learn.gae; the second has the new targets
    with pytest.raises(ValueError, match="native"):
        ppo_selfplay.main(vtrace=True, native_batch=True, **kw)


# ---- at a wide pitch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(5), ids=("reward_pitch", "flag_pitch", "value_pitch", "log_prob_pitch", "out_pitch"))
def test_wide_pitches(lib, which):
    """k = 2 steps (three value rows) of one agent with one of the five pitches wide (tests/wide_rows.py: rows 2^31 elements and
    2^32 bytes apart inside one allocation): the outputs equal the judge's bits and no row's guard is touched.  With a wide
    log-prob pitch the behaviour and target rows, with a wide output pitch the two outputs, are two row sets of one allocation.
    (The kernel has no grid-stride loop -- one lane per game, the grid covers n -- so "many_workgroups" above is its large grid.)"""
    from wide_rows import LIMIT_BYTES, WideRows

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    k, n, vf = 2, 65, "bfloat16"
    c = J.make_case(k, n, "random50", "float32", vf, seed=63, agents=1)
    want = J.judge32(c["rew"][0], c["d"], c["val"][0], c["lpb"][0], c["lpt"][0])
    hosts = [np.ascontiguousarray(c["rew"][0]), np.ascontiguousarray(c["d"]), GJ.value_bits(c["val"][0], vf)]
    pitches, ptrs, keep = [n] * 5, [None] * 3, []
    w = None
    for i, host in enumerate(hosts):
        if i == which:
            w = WideRows(host.shape[0], n, host.dtype.itemsize).put(host)
            pitches[i], ptrs[i] = w.pitch, w.ptr()
        else:
            keep.append(device_rows(host, n, host.dtype.type(3)))
            ptrs[i] = keep[-1].data_ptr()
    if which == 3:
        w = WideRows(k, n, 4, views=2).put(c["lpb"][0], 0).put(c["lpt"][0], 1)
        pitches[3], lps = w.pitch, [w.ptr(0), w.ptr(1)]
    else:
        keep += [device_rows(c["lpb"][0], n, np.float32(9)), device_rows(c["lpt"][0], n, np.float32(9))]
        lps = [keep[-2].data_ptr(), keep[-1].data_ptr()]
    if which == 4:
        w = WideRows(k, n, 4, views=2)
        pitches[4], outs = w.pitch, [w.ptr(0), w.ptr(1)]
    else:
        small = [torch.full((k * n + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        outs = [t.data_ptr() for t in small]
    try:
        err = lib.pz_vtrace(ptrs[0], None, J.REWARD_DTYPES.index("float32"), ptrs[1], ptrs[2], None, J.VALUE_DTYPES.index(vf), lps[0], None, lps[1], None,
                            k, n, *pitches, J.GAMMA, J.LAM, *J.CLIPS, outs[1], None, outs[0], None, torch.cuda.current_stream().cuda_stream)
        assert err == 0
        torch.cuda.synchronize()
        if which == 4:
            got = [w.get(0), w.get(1)]
        else:
            got = []
            for t in small:
                flat = cpu(t)
                assert (flat[k * n:] == SENT).all(), "a launch wrote behind its output"
                got.append(flat[:k * n].reshape(k, n))
        for have, ref, what in zip(got, want, ("advantages", "returns")):
            assert np.array_equal(have.view(np.uint32), bits(ref)), (what, pitches)
        if which < 3:
            assert np.array_equal(w.get().view(hosts[which].dtype), hosts[which]), "an input changed"
        elif which == 3:
            assert np.array_equal(w.get(0).view(np.float32).view(np.uint32), bits(c["lpb"][0])) and np.array_equal(w.get(1).view(np.uint32), bits(c["lpt"][0]))
    finally:
        torch.cuda.synchronize()
        w.close()
        torch.cuda.empty_cache()
    assert torch.cuda.max_memory_allocated() <= LIMIT_BYTES + (256 << 20)
