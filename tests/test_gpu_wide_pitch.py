"""GPU tests (``-m gpu``) of the learner's int64 pitches: every entry point that takes a pitch runs once per pitch on rows that
lie 2^31 elements and 2^32 bytes apart inside one large allocation (tests/wide_rows.py), one wide tensor per call, and is
judged by its library's own judge on the rows written.  A kernel that formed ``row * pitch`` in 32 bits would read or write
somewhere else: the rows behind the limit would be wrong, or a row's guard overwritten.  No GPU result is ever an expected
value.  Every test frees its large buffer and holds at most 10 GiB of device memory at any time.

The three libraries that came after that work are here too: ``pz_mlp_act`` and ``pz_mlp_act_pool`` (``obs_pitch`` and
``head_pitch``: their kernels drive the tile through ``tile_layers`` and ``store_tile_float32``, which repeat the forward's text
beside it, so the forward's test above says nothing about them) and ``pz_ego_rows`` (``in_pitch`` and ``out_pitch`` of the
element-by-element kernel, in place too).  Their 40-row cases are picked to have no ambiguous row (tests/test_act_host.py and
tests/test_pool_act_host.py assert it).
"""
import numpy as np
import pytest
import torch

import act_judge as AJ
import ego_judge as EJ
import gae_judge as GJ
import league_judge as LJ
import net_judge as N
import netgrad_judge as G
import policy_judge as J
import pool_act_judge as PA
import pool_judge as PJ
import ppo_judge as P
from test_gpu_policy import SENT, TAIL, check_against_judge, check_gradient, cpu, device_rows, sentinel, stream
from wide_rows import LIMIT_BYTES, POISON, WideRows

pytestmark = pytest.mark.gpu

ROWS = 40            # one 32-row tile and a part; the last three rows start beyond element 2^31
LIVELY = ("random0.5", "random2", "random6", "masked_tail")    # policy_judge's row kinds whose every output depends on the logits
F16, BF16 = "float16", "bfloat16"


@pytest.fixture
def wide():
    """WideRows, every one of them released when the test ends and the test's peak of live device memory checked"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    made = []

    def make(*args, **kw):
        for w in made:                       # (one wide tensor at a time)
            w.close()
        made.append(WideRows(*args, **kw))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for w in made:
        w.close()
    torch.cuda.empty_cache()
    assert torch.cuda.max_memory_allocated() <= LIMIT_BYTES + (256 << 20)


def bits16(values, dtype):
    """float32 values representable in a 16-bit `dtype` -> its int16 element patterns"""
    return np.ascontiguousarray(J.logit_bits(np.asarray(values, np.float32), dtype)).view(np.int16)


def values16(bits, dtype):
    return J.bits_to_float(np.ascontiguousarray(bits).view(np.float16 if dtype == F16 else np.uint16), dtype)


def narrow(count, dtype=torch.int32):
    return torch.full((count + TAIL,), SENT, dtype=dtype, device="cuda:0")


def read_narrow(t, count):
    flat = cpu(t)
    assert (flat[count:] == SENT).all(), "a launch wrote behind its output"
    return flat[:count]


def within(have, ref, tol, what):
    worst, rows = N.worst_share(have, ref, tol)
    print(f"{what}: worst error / tolerance {worst:.4f}")
    assert worst <= 1, (what, worst, rows)


# ---- pz_mlp_forward, pz_mlp_forward_pool ---------------------------------------------------------------------------------------
def test_mlp_forward(wide):
    from pikazoo_amd import net
    from test_gpu_net import device_obs, device_params

    lib = net.load()
    n, K, H, O = ROWS, 35, 64, 19
    params = N.make_params(K, H, O, 51)
    keep, ptrs = device_params(params)
    obs = N.make_obs(n, K, F16, 52)

    def forward(x, obs_pitch, out, out_format, out_pitch):
        assert lib.pz_mlp_forward(x, None, N.OBS_DTYPES.index(F16), n, K, obs_pitch, H, O, 0, *ptrs, *[None] * 6, out, None, out_format, out_pitch,
                                  stream()) == 0
        torch.cuda.synchronize()

    w = wide(n, K, 2).put(bits16(obs, F16))
    out = narrow(n * O)
    forward(w.ptr(), w.pitch, out.data_ptr(), 0, O)
    have = read_narrow(out, n * O).view(np.float32).reshape(n, O)
    within(have, *N.judge(obs, params, "tanh"), f"obs_pitch {w.pitch}")
    x = device_obs(obs, F16, K, 0)
    w = wide(n, O, 2)
    forward(x[1], K, w.ptr(), N.OUT_DTYPES.index(F16), w.pitch)
    within(values16(w.get(), F16), *N.judge(obs, params, "tanh", F16), f"out_pitch {w.pitch}")
    del keep


def test_mlp_forward_pool(wide):
    from pikazoo_amd import pool
    from test_gpu_net import device_obs, device_params
    from test_gpu_pool import member_array, run_plan

    lib = pool.load()
    n, K, H, O, Pm = ROWS, 35, 64, 19, 3
    params = [N.make_params(K, H, O, 53 + p) for p in range(Pm)]
    sets = [device_params(p) for p in params]
    obs = N.make_obs(n, K, F16, 57)
    members = PJ.typed(PJ.member_vector("round_robin", n, Pm), "int32")
    members[5] = -1                                                                # (a row that must stay unwritten)
    plan = run_plan(lib, members, Pm)[3]
    eff = PJ.effective_members(members, Pm)
    written = eff >= 0

    def forward(x, obs_pitch, out, out_format, out_pitch):
        assert lib.pz_mlp_forward_pool(x, None, N.OBS_DTYPES.index(F16), n, K, obs_pitch, H, O, 1, member_array(sets), Pm, plan[0][1], plan[1][1],
                                       None, None, out, None, out_format, out_pitch, stream()) == 0
        torch.cuda.synchronize()

    w = wide(n, K, 2).put(bits16(obs, F16))
    out = narrow(n * O)
    forward(w.ptr(), w.pitch, out.data_ptr(), 0, O)
    rows = read_narrow(out, n * O).reshape(n, O)
    assert (rows[~written] == SENT).all()
    ref, tol = PJ.judge(obs, params, eff, "relu")
    within(rows.view(np.float32)[written], ref[written], tol[written], f"pool obs_pitch {w.pitch}")
    x = device_obs(obs, F16, K, 0)
    w = wide(n, O, 2)
    forward(x[1], K, w.ptr(), N.OUT_DTYPES.index(BF16), w.pitch)
    got = w.get()
    assert (got[~written] == SENT).all()
    ref, tol = PJ.judge(obs, params, eff, "relu", BF16)
    within(values16(got, BF16)[written], ref[written], tol[written], f"pool out_pitch {w.pitch}")


# ---- pz_mlp_backward -----------------------------------------------------------------------------------------------------------
def test_mlp_backward(wide):
    from pikazoo_amd import netgrad
    from test_gpu_netgrad import guarded, param_tensor, rows_tensor

    lib = netgrad.load()
    n, K, H, O = ROWS, 35, 64, 19
    sides, params = G.make_case(n, K, H, O, "tanh", 58, obs_dtype=F16, grad_dtype=BF16)
    x, g = sides[0]
    refs, tols, _ = G.judge(sides, params, "tanh")
    dev_params = [param_tensor(p) for p in params]
    ws = torch.zeros(lib.pz_mlp_backward_workspace_bytes(n, K, H, O) // 4, device="cuda:0")

    def backward(xp, obs_pitch, gp, grad_pitch, what):
        outs = [guarded(p.shape) for p in params]
        assert lib.pz_mlp_backward(xp, None, N.OBS_DTYPES.index(F16), n, K, obs_pitch, H, O, 0, *[p.data_ptr() for p in dev_params], *[None] * 6,
                                   gp, None, G.GRAD_DTYPES.index(BF16), grad_pitch, *[v.data_ptr() for _, v in outs], *[None] * 6, ws.data_ptr(),
                                   None) == 0
        torch.cuda.synchronize()
        share, beyond = G.worst_share([cpu(v) for _, v in outs], refs, tols)
        print(f"{what}: worst error / tolerance {share:.4f}")
        assert not beyond, (what, share, beyond)

    small_x = rows_tensor(x, F16, K, 0)
    small_g = rows_tensor(g, BF16, O, 0)
    w = wide(n, K, 2).put(bits16(x, F16))
    backward(w.ptr(), w.pitch, small_g.data_ptr(), O, f"backward obs_pitch {w.pitch}")
    w = wide(n, O, 2).put(bits16(g, BF16))
    backward(small_x.data_ptr(), K, w.ptr(), w.pitch, f"backward grad_pitch {w.pitch}")


# ---- the policy launches -------------------------------------------------------------------------------------------------------
def test_policy_launches_on_gathered_rows(wide):
    """a pitch far above the staged range: the A live columns of a row are gathered"""
    from pikazoo_amd import policy

    lib = policy.load()
    n, A, draw = ROWS, 18, J.DRAWS[1]
    logits, kinds = J.make_rows(n, A, F16, seed=59, kinds=LIVELY)
    u = J.uniforms(*draw, n)[0]
    fmt = J.LOGIT_DTYPES.index(F16)

    w = wide(n, A, 2).put(bits16(logits, F16))
    act, logp, ent = narrow(n), narrow(n), narrow(n)
    assert lib.pz_sample_actions(w.ptr(), None, fmt, A, n, w.pitch, draw[0], draw[1], draw[2], None, 0, act.data_ptr(), None, logp.data_ptr(), None,
                                 ent.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    got = (read_narrow(act, n).astype(np.int64), read_narrow(logp, n).view(np.float32), read_narrow(ent, n).view(np.float32))
    st, _ = check_against_judge(logits, u, got, f"sample at logit_pitch {w.pitch}")
    logp2, ent2 = narrow(n), narrow(n)
    assert lib.pz_action_log_probs(w.ptr(), None, fmt, A, n, w.pitch, 0, act.data_ptr(), None, logp2.data_ptr(), None, ent2.data_ptr(), None,
                                   stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(read_narrow(logp2, n), read_narrow(logp, n)) and np.array_equal(read_narrow(ent2, n), read_narrow(ent, n))

    rng = np.random.default_rng(3)
    glogp, gent = (rng.normal(size=n).astype(np.float32) for _ in range(2))
    up = [torch.from_numpy(v).to("cuda:0") for v in (glogp, gent)]

    def backward(lp, logit_pitch, gp, grad_pitch):
        assert lib.pz_action_log_probs_backward(lp, None, fmt, A, n, logit_pitch, 0, act.data_ptr(), None, up[0].data_ptr(), None, up[1].data_ptr(),
                                                None, gp, None, grad_pitch, stream()) == 0
        torch.cuda.synchronize()

    grads = narrow(n * A, torch.int16)
    backward(w.ptr(), w.pitch, grads.data_ptr(), A)
    check_gradient(st, got[0], glogp, gent, values16(read_narrow(grads, n * A).reshape(n, A), F16), F16, f"backward at logit_pitch {w.pitch}")
    small = device_rows(logits, F16, A, 0)
    w = wide(n, A, 2)
    backward(small[1], A, w.ptr(), w.pitch)
    check_gradient(st, got[0], glogp, gent, values16(w.get(), F16), F16, f"backward at grad_pitch {w.pitch}")


def test_sampling_staged_rows_beyond_4_gib(wide):
    """the trainer's layout -- float16 logits at pitch 19, staged -- with so many rows that the last ones lie beyond byte 2^32:
    the first and the last 4133 rows are written and judged; the rows between hold whatever the allocation held (the header
    defines a NaN row's result; nothing is out of bounds)"""
    from pikazoo_amd import policy

    lib = policy.load()
    A, pitch, shard = 18, 19, 4133
    n = -(-(1 << 32) // (pitch * 2)) + shard + 12
    assert (n - shard) * pitch * 2 >= 1 << 32 and n <= 1 << 30
    seed, first_game, step, _ = J.DRAWS[1]
    big = torch.empty(n * pitch, dtype=torch.int16, device="cuda:0")
    rows = big.view(n, pitch)
    cases = {}
    for start in (0, n - shard):
        logits, kinds = J.make_rows(shard, A, F16, seed=61 + (start > 0))
        full = np.full((shard, pitch), np.nan, np.float32)
        full[:, :A] = logits
        rows[start:start + shard].copy_(torch.from_numpy(bits16(full, F16)).to("cuda:0"))
        cases[start] = logits
    act = torch.full((n + TAIL,), SENT, dtype=torch.int32, device="cuda:0")
    logp, ent = torch.full_like(act, SENT), torch.full_like(act, SENT)
    assert lib.pz_sample_actions(big.data_ptr(), None, J.LOGIT_DTYPES.index(F16), A, n, pitch, seed, first_game, step, None, 0, act.data_ptr(), None,
                                 logp.data_ptr(), None, ent.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert all((cpu(t[n:]) == SENT).all() for t in (act, logp, ent)), "a launch wrote behind its output"
    for start, logits in cases.items():
        u = J.uniforms(seed, first_game + start, step, None, shard)[0]
        got = tuple(cpu(t[start:start + shard]) for t in (act, logp, ent))
        check_against_judge(logits, u, (got[0].astype(np.int64), got[1].view(np.float32), got[2].view(np.float32)), f"n = {n}, rows from {start}")
    del big, rows, act, logp, ent


# ---- pz_ppo_loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("logit_pitch", "value_pitch", "grad_pitch", "grad_value_pitch"))
def test_ppo_loss(wide, which):
    from pikazoo_amd import ppo
    from test_gpu_ppo import check, f32_vector, workspace_for

    lib = ppo.load()
    n, A, dtype, vdt = ROWS, 18, BF16, F16
    case = P.make_case(n, A, dtype, vdt, 62, value_clip=0.0, normalize=False, kinds=LIVELY)
    jd = P.judge(case)
    w = wide(n, A if which in ("logit_pitch", "grad_pitch") else 1, 2)
    pitch = dict(logit_pitch=A, value_pitch=1, grad_pitch=A, grad_value_pitch=1)
    pitch[which] = w.pitch
    logits = device_rows(case["logits"], dtype, A, 0)
    values = device_rows(case["values"][:, None], vdt, 1, 0)
    glog, gval = narrow(n * A, torch.int16), narrow(n, torch.int16)
    ptr = dict(logit_pitch=logits[1], value_pitch=values[1], grad_pitch=glog.data_ptr(), grad_value_pitch=gval.data_ptr())
    ptr[which] = w.ptr()
    if which == "logit_pitch":
        w.put(bits16(case["logits"], dtype))
    elif which == "value_pitch":
        w.put(bits16(case["values"][:, None], vdt))
    act = torch.from_numpy(case["actions"].astype(np.int64)).to("cuda:0")
    old_logp, adv, ret = (f32_vector(case[k]) for k in ("old_logp", "adv", "ret"))
    stats = sentinel(16, torch.int32)
    ws, size = workspace_for(lib, n)
    err = lib.pz_ppo_loss(ptr["logit_pitch"], None, J.LOGIT_DTYPES.index(dtype), A, n, pitch["logit_pitch"], J.ACTION_DTYPES.index("int64"),
                          act.data_ptr(), None, old_logp.data_ptr(), None, adv.data_ptr(), None, ret.data_ptr(), None, ptr["value_pitch"], None,
                          J.LOGIT_DTYPES.index(vdt), pitch["value_pitch"], None, None, 0, None, case["clip"], case["value_clip"], case["vf_coef"],
                          case["ent_coef"], ptr["grad_pitch"], None, pitch["grad_pitch"], ptr["grad_value_pitch"], None, pitch["grad_value_pitch"],
                          stats.data_ptr(), ws.data_ptr(), stream())
    assert err == 0
    torch.cuda.synchronize()
    host_stats = cpu(stats)
    assert (host_stats[8:] == SENT).all() and (cpu(ws)[max(size, 16):] == 0xA5).all()
    gl = w.get() if which == "grad_pitch" else read_narrow(glog, n * A).reshape(n, A)
    gv = w.get()[:, 0] if which == "grad_value_pitch" else read_narrow(gval, n)
    got = dict(stats=host_stats[:8].view(np.float32), grad_logits=values16(gl, dtype), grad_values=values16(gv, vdt))
    check(jd, got, dtype, vdt, f"{which} {w.pitch}")


# ---- pz_gae --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=("reward_pitch", "flag_pitch", "value_pitch", "out_pitch"))
def test_gae(wide, which):
    """k = 2 steps (three value rows) of one agent, one of the four pitches wide: the outputs equal the judge's bits; with a
    wide output pitch the advantages and the returns are two row sets of one allocation"""
    from pikazoo_amd import learn
    from test_gpu_gae import GAMMA, LAM, bits, device_rows as flat_rows

    lib = learn.load()
    k, n, value_dtype = 2, 65, BF16
    c = GJ.make_case(k, n, "random50", "float32", value_dtype, seed=63, agents=1)
    want = GJ.judge(c["rew"][0], c["d"], c["val"][0], GAMMA, LAM)
    hosts = [np.ascontiguousarray(c["rew"][0]), np.ascontiguousarray(c["d"]), GJ.value_bits(c["val"][0], value_dtype)]
    pitches, ptrs, keep = [n] * 4, [None] * 3, []
    w = None
    for i, host in enumerate(hosts):
        if i == which:
            w = wide(host.shape[0], n, host.dtype.itemsize).put(host)
            pitches[i], ptrs[i] = w.pitch, w.ptr()
        else:
            keep.append(flat_rows(host, n, host.dtype.type(3)))
            ptrs[i] = keep[-1].data_ptr()
    if which == 3:
        w = wide(k, n, 4, views=2)
        pitches[3], outs = w.pitch, [w.ptr(0), w.ptr(1)]
    else:
        small = [narrow(k * n), narrow(k * n)]
        outs = [t.data_ptr() for t in small]
    err = lib.pz_gae(ptrs[0], None, GJ.REWARD_DTYPES.index("float32"), ptrs[1], ptrs[2], None, GJ.VALUE_DTYPES.index(value_dtype), k, n, *pitches,
                     GAMMA, LAM, outs[0], None, outs[1], None, stream())
    assert err == 0
    torch.cuda.synchronize()
    got = [w.get(0), w.get(1)] if which == 3 else [read_narrow(t, k * n).reshape(k, n) for t in small]
    for have, ref, what in zip(got, want, ("advantages", "returns")):
        assert np.array_equal(have.view(np.uint32), bits(ref)), (what, pitches)
    if which != 3:
        assert np.array_equal(w.get().view(hosts[which].dtype), hosts[which]), "an input changed"


# ---- pz_league_tally -----------------------------------------------------------------------------------------------------------
def test_league_tally(wide):
    """int16 scores of 40 games at a stride beyond 2^31 elements, both agents' scores as two row sets of one allocation"""
    from pikazoo_amd import league
    from test_gpu_league import guarded, on_device, ptr, read_guarded

    lib = league.load()
    n, Pm = ROWS, 3
    case = dict(n=n, P=Pm, terminated="all", stride=1, score_dtype="int16", with_p1=True, member_dtype="int32", invalid=False, seed=64)
    x = LJ.tally_inputs(case)
    want, want_errors = LJ.tally(x["terminated"], x["buf1"], x["buf2"], 1, x["members_p1"], x["members_p2"], Pm, x["table"], x["errors"])
    w = wide(n, 1, 2, views=2).put(x["buf1"][:, None], 0).put(x["buf2"][:, None], 1)
    table, errors = guarded(x["table"], "int64"), guarded([x["errors"]], "int64")
    d = {key: on_device(x[key]) for key in ("terminated", "members_p1", "members_p2")}
    assert lib.pz_league_tally(ptr(d["terminated"]), w.ptr(0), w.ptr(1), LJ.SCORE_DTYPES.index("int16"), w.pitch, ptr(d["members_p1"]),
                               ptr(d["members_p2"]), LJ.MEMBER_DTYPES.index("int32"), n, Pm, table[1], errors[1], stream()) == 0
    torch.cuda.synchronize()
    got = read_guarded(table[0], Pm * Pm * LJ.CELL).reshape(Pm, Pm, LJ.CELL)
    assert int(read_guarded(errors[0], 1)[0]) == want_errors and np.array_equal(got, want), np.argwhere(got != want)[:8]
    behind = np.arange(n) >= w.first_beyond
    counted = behind & (x["members_p1"] >= 0) & (x["members_p1"] < Pm) & (x["members_p2"] >= 0) & (x["members_p2"] < Pm)
    assert counted.sum() == n - w.first_beyond and (x["buf1"][counted] != 0).all(), "the case tallies a game whose scores lie behind the limit"


# ---- pz_mlp_act, pz_mlp_act_pool -----------------------------------------------------------------------------------------------
def wide_head_rows(w, sides, written=None):
    """the float32 head rows of both agents out of a wide tensor (the guard behind every row checked by ``get``); the rows that
    must not be written still hold the poison"""
    out = []
    for s in range(sides):
        got = w.get(s)
        if written is not None:
            assert (got[~written[s]] == POISON).all(), f"the head of side {s}: a row of an invalid member was written"
        out.append(np.ascontiguousarray(got).view(np.float32))
    return out


def test_mlp_act(wide):
    """(35, 64, 19, 18), two agents on nets of their own: float16 observations at a wide obs_pitch (both agents' rows side by
    side in one allocation) with a narrow head, then narrow observations with a float32 head at a wide head_pitch"""
    from pikazoo_amd import act
    from test_gpu_act import Inputs, pointers, read_head, read_vectors, step_tensor, vectors

    lib = act.load()
    c = AJ.WIDE_CASE
    n, (K, H, O, A), activation, draw = c["n"], c["size"], c["activation"], AJ.DRAWS[c["draw"]]
    assert n == ROWS
    obs, params = AJ.wide_case_inputs()
    inp = Inputs(obs, F16, params)
    us = AJ.uniforms(draw, n)
    dev = step_tensor(draw)

    def launch(obs_ptrs, obs_pitch, head_ptrs, head_pitch, what):
        args = list(inp.net_args(activation))
        args[0], args[1], args[5] = obs_ptrs[0], obs_ptrs[1], obs_pitch
        a, logp, ent, val = (vectors(2, n, d) for d in (torch.int64, torch.int32, torch.int32, torch.int32))
        assert lib.pz_mlp_act(*args, A, draw[0], draw[1], draw[2], dev.data_ptr() if dev is not None else None, J.ACTION_DTYPES.index("int64"),
                              *pointers(a, 2, itemsize=8), *pointers(logp, 2), *pointers(ent, 2), *pointers(val, 2), *head_ptrs, head_pitch,
                              stream()) == 0
        torch.cuda.synchronize()
        a, logp, ent, val = (read_vectors(ts, n, True, f"{what}: {key}") for ts, key in ((a, "actions"), (logp, "log_probs"), (ent, "entropy"),
                                                                                      (val, "values")))
        return [dict(actions=a[s].astype(np.int64), log_probs=logp[s].view(np.float32), entropy=ent[s].view(np.float32),
                     values=val[s].view(np.float32)) for s in (0, 1)]

    def judged(got, heads, what):
        for s in (0, 1):
            amb, fails = AJ.verdict(dict(got[s], head=heads[s]), obs[s], params[s], activation, A, us[s], what=f"{what} side {s}")
            assert not fails, fails

    patterns = [bits16(x, F16) for x in obs]
    w = wide(n, K, 2, views=2).put(patterns[0], 0).put(patterns[1], 1)
    heads = [torch.full((n * O + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in (0, 1)]
    got = launch([w.ptr(0), w.ptr(1)], w.pitch, [h.data_ptr() for h in heads], O, "wide obs_pitch")
    judged(got, read_head(heads, n, O, O, 0), f"act obs_pitch {w.pitch}")
    assert all(np.array_equal(w.get(s), patterns[s]) for s in (0, 1)), "an input changed"
    w = wide(n, O, 4, views=2)
    got = launch([inp.xs[0][1], inp.xs[1][1]], K, [w.ptr(0), w.ptr(1)], w.pitch, "wide head_pitch")
    judged(got, wide_head_rows(w, 2), f"act head_pitch {w.pitch}")


def test_mlp_act_pool(wide):
    """the same two pitches with three members round-robin for both agents and, per agent, one row of an invalid member (agent
    2's behind the limit): its outputs keep the sentinel and its head row the poison"""
    from pikazoo_amd import act, policy, pool, pool_act
    from test_gpu_pool_act import Device, draw_args, pointers, read_heads, read_vectors, vectors

    libs = (pool_act.load(), pool.load(), policy.load(), act.load())
    case, obs, params, members = PA.wide_case()
    n, K, O, A = case["n"], case["K"], case["O"], case["A"]
    assert n == ROWS
    d = Device(libs, case, obs, params, members)
    assert [np.flatnonzero(~x).tolist() for x in d.written] == [[5], [38]] and w_first_beyond(n) <= 38
    dev, dargs = draw_args(PA.DRAWS[case["draw"]])
    on = (True, True)

    def launch(obs_ptrs, obs_pitch, head_ptrs, head_pitch, what):
        args = list(d.args())
        args[0], args[1], args[5] = obs_ptrs[0], obs_ptrs[1], obs_pitch
        a, logp, ent, val = (vectors(2, n, t) for t in (torch.int64, torch.int32, torch.int32, torch.int32))
        assert libs[0].pz_mlp_act_pool(*args, A, *dargs, J.ACTION_DTYPES.index("int64"), *pointers(a, on, 8), *pointers(logp, on), *pointers(ent, on),
                                       *pointers(val, on), *head_ptrs, head_pitch, stream()) == 0
        torch.cuda.synchronize()
        a, logp, ent, val = (read_vectors(ts, n, on, d.written, f"{what}: {key}") for ts, key in ((a, "actions"), (logp, "log_probs"),
                                                                                                   (ent, "entropy"), (val, "values")))
        return [dict(written=d.written[s], actions=a[s].astype(np.int64), log_probs=logp[s].view(np.float32), entropy=ent[s].view(np.float32),
                     values=val[s].view(np.float32)) for s in (0, 1)]

    def judged(got, heads, what):
        amb, fails = PA.verdict(case, [dict(got[s], head=heads[s]) for s in (0, 1)], obs, params, members, what=what)
        assert not fails, fails

    patterns = [bits16(x, F16) for x in obs]
    w = wide(n, K, 2, views=2).put(patterns[0], 0).put(patterns[1], 1)
    heads = [torch.full((n * O + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in (0, 1)]
    got = launch([w.ptr(0), w.ptr(1)], w.pitch, [h.data_ptr() for h in heads], O, "wide obs_pitch")
    judged(got, read_heads(heads, n, O, O, 0, on, d.written), f"pool act obs_pitch {w.pitch}")
    assert all(np.array_equal(w.get(s), patterns[s]) for s in (0, 1)), "an input changed"
    w = wide(n, O, 4, views=2)
    got = launch([d.xs[0][1], d.xs[1][1]], K, [w.ptr(0), w.ptr(1)], w.pitch, "wide head_pitch")
    judged(got, wide_head_rows(w, 2, d.written), f"pool act head_pitch {w.pitch}")


def w_first_beyond(rows):
    """the first row of a WideRows of `rows` rows that starts at or beyond the limit"""
    return rows - min(3, max(1, rows // 8))


# ---- pz_ego_rows, element by element -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (6, 1), ids=("bfloat16 normalised", "float32 normalised"))
def test_ego_rows(wide, fmt):
    """wide in_pitch into rows back to back, rows back to back out at a wide out_pitch, and in place on one wide tensor: equal to
    the judge bit for bit, the guard behind every wide row intact, the input unchanged where the call is out of place"""
    from pikazoo_amd import ego

    lib = ego.load()
    n, size = ROWS, EJ.STORAGE[fmt]().itemsize
    stored = EJ.encode(EJ.large_content(n, 5), fmt)
    words, want = EJ.bits(stored), EJ.bits(EJ.mirror(stored, fmt))
    assert (words != want).any(axis=1)[w_first_beyond(n):].all()                   # (the rows behind the limit change)
    word = torch.int16 if size == 2 else torch.int32

    def narrow_rows(fill=None):
        t = torch.full((n * EJ.DIM + TAIL,), SENT, dtype=word, device="cuda:0")
        if fill is not None:
            t[:n * EJ.DIM] = torch.from_numpy(fill.view(np.int16 if size == 2 else np.int32).reshape(-1).copy()).to("cuda:0")
        return t

    def read(t):
        flat = cpu(t)
        assert (flat[n * EJ.DIM:] == SENT).all(), "a launch wrote behind its output"
        return flat[:n * EJ.DIM].view(words.dtype).reshape(n, EJ.DIM)

    def rows(p_in, p_out, in_pitch, out_pitch):
        assert lib.pz_ego_rows(p_in, p_out, fmt, n, in_pitch, out_pitch, stream()) == 0
        torch.cuda.synchronize()

    w = wide(n, EJ.DIM, size).put(words)
    out = narrow_rows()
    rows(w.ptr(), out.data_ptr(), w.pitch, EJ.DIM)
    assert np.array_equal(read(out), want) and np.array_equal(w.get().view(words.dtype), words), f"in_pitch {w.pitch}"
    rows(w.ptr(), w.ptr(), w.pitch, w.pitch)
    assert np.array_equal(w.get().view(words.dtype), want), f"in place at pitch {w.pitch}"
    src = narrow_rows(words)
    w = wide(n, EJ.DIM, size)
    rows(src.data_ptr(), w.ptr(), EJ.DIM, w.pitch)
    assert np.array_equal(w.get().view(words.dtype), want) and np.array_equal(read(src), words), f"out_pitch {w.pitch}"
