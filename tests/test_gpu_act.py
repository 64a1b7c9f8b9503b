"""GPU tests (``-m gpu``) of the act launch (include/pikazoo_act.h: ``pz_mlp_act``) and of ``pikazoo_amd.act``.

Two references, kept apart.  (1) The header's promise: the bits of pz_mlp_forward (float32) followed by pz_sample_actions on
the same inputs -- actions, log-prob, entropy, value and head compared bit for bit, one axis swept per test.  (2) The float64
judge of tests/act_judge.py, which knows nothing of the older kernels (its ``verdict``).  Every C-ABI launch writes into
sentinel-filled outputs with elements in front of the first one and behind the last one (and in the head's pad columns), all
of which must keep the sentinel; the pad columns of the observations and the memory around the parameters hold NaN patterns.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import act_judge as AJ
import net_judge as N
import policy_judge as J
from test_gpu_net import device_obs, device_params
from test_gpu_policy import SENT, TAIL, TORCH_ACTION, cpu, stream

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
REPO = Path(__file__).resolve().parent.parent
FRONT = 8  # elements in front of every output vector (8: an int64 vector stays aligned)


@pytest.fixture(scope="module")
def libs():
    from pikazoo_amd import act, net, policy

    return act.load(), net.load(), policy.load()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


class Inputs:
    """the device buffers of one case, shared by the launches that are compared"""

    def __init__(self, obs, obs_dtype, params, obs_pitch=None, offset=0, shared=False):
        self.n, self.K = obs[0].shape
        self.H, self.O = params[0][0].shape[0], params[0][4].shape[0]
        self.sides, self.obs_dtype, self.obs_pitch = len(obs), obs_dtype, obs_pitch or self.K
        self.xs = [device_obs(x, obs_dtype, self.obs_pitch, offset) for x in obs]
        sets = [device_params(p, offset) for p in params[:1 if shared else len(obs)]]
        self.sets = [sets[0]] * len(obs) if shared else sets

    def net_args(self, activation):
        second = self.sides == 2
        return (self.xs[0][1], self.xs[1][1] if second else None, N.OBS_DTYPES.index(self.obs_dtype), self.n, self.K, self.obs_pitch, self.H,
                self.O, N.ACTIVATIONS.index(activation), *self.sets[0][1], *(self.sets[1][1] if second else [None] * 6))


def vectors(sides, n, dtype):
    return [torch.full((FRONT + n + TAIL,), SENT, dtype=dtype, device="cuda:0") for _ in range(sides)]


def pointers(ts, sides, on=True, itemsize=4, front=FRONT):
    return [(ts[i].data_ptr() + front * itemsize if on and i < sides else None) for i in (0, 1)]


def read_vectors(ts, n, on, what):
    out = []
    for t in ts:
        flat = cpu(t)
        assert (flat[:FRONT] == SENT).all() and (flat[FRONT + n:] == SENT).all(), f"{what}: written outside its rows"
        assert on or (flat == SENT).all(), f"{what}: written though it was not asked for"
        out.append(flat[FRONT:FRONT + n])
    return out


def step_tensor(draw):
    return torch.tensor([draw[3]], dtype=torch.int64, device="cuda:0") if draw[3] is not None else None


def read_head(heads, n, O, pitch, offset):
    out = []
    for h in heads:
        flat = cpu(h)
        rows = flat[offset:offset + n * pitch].reshape(n, pitch)
        assert (flat[:offset] == SENT).all() and (flat[offset + n * pitch:] == SENT).all(), "the head outside its rows"
        assert (rows[:, O:] == SENT).all(), "a pad column of the head was written"
        out.append(np.ascontiguousarray(rows[:, :O]).view(np.float32))
    return out


def run_act(libs, inp, activation, A, draw, action_dtype="int64", head=True, head_pitch=None, offset=0, with_logp=True, with_ent=True,
            with_val=None, expect=0):
    """pz_mlp_act: per side a dict (head or None, actions int64, log_probs, entropy, values or None) as numpy"""
    n, O, sides = inp.n, inp.O, inp.sides
    with_val = O > A if with_val is None else with_val
    head_pitch = head_pitch or O
    asize = 8 if action_dtype == "int64" else 4
    act, logp, ent, val = (vectors(sides, n, d) for d in (TORCH_ACTION[action_dtype], torch.int32, torch.int32, torch.int32))
    heads = [torch.full((offset + n * head_pitch + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(sides)]
    seed, first_game, step, _ = draw
    dev = step_tensor(draw)
    err = libs[0].pz_mlp_act(*inp.net_args(activation), A, seed, first_game, step, dev.data_ptr() if dev is not None else None,
                             J.ACTION_DTYPES.index(action_dtype), *pointers(act, sides, itemsize=asize), *pointers(logp, sides, with_logp),
                             *pointers(ent, sides, with_ent), *pointers(val, sides, with_val), *pointers(heads, sides, head, front=offset),
                             head_pitch, stream())
    assert err == expect
    torch.cuda.synchronize()
    a, lp, en, va = (read_vectors(ts, n, on, what) for ts, on, what in ((act, True, "actions"), (logp, with_logp, "log_probs"),
                                                                        (ent, with_ent, "entropy"), (val, with_val, "values")))
    hs = read_head(heads, n, O, head_pitch, offset) if head else [None] * sides
    assert head or all((cpu(h) == SENT).all() for h in heads), "a head that was not asked for was written"
    return [dict(head=hs[s], actions=a[s].astype(np.int64), log_probs=lp[s].view(np.float32), entropy=en[s].view(np.float32),
                 values=va[s].view(np.float32) if with_val else None) for s in range(sides)]


def run_two_launches(libs, inp, activation, A, draw, action_dtype="int64", head_pitch=None, offset=0):
    """pz_mlp_forward (float32, at `head_pitch`) and pz_sample_actions on its logits: the same dicts"""
    n, O, sides = inp.n, inp.O, inp.sides
    head_pitch = head_pitch or O
    second = sides == 2
    asize = 8 if action_dtype == "int64" else 4
    heads = [torch.full((offset + n * head_pitch + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(sides)]
    hp = pointers(heads, sides, front=offset)
    assert libs[1].pz_mlp_forward(*inp.net_args(activation), *hp, 0, head_pitch, stream()) == 0
    act, logp, ent = (vectors(sides, n, d) for d in (TORCH_ACTION[action_dtype], torch.int32, torch.int32))
    seed, first_game, step, _ = draw
    dev = step_tensor(draw)
    assert libs[2].pz_sample_actions(*hp, 0, A, n, head_pitch, seed, first_game, step, dev.data_ptr() if dev is not None else None,
                                     J.ACTION_DTYPES.index(action_dtype), *pointers(act, sides, itemsize=asize), *pointers(logp, sides),
                                     *pointers(ent, sides), stream()) == 0
    torch.cuda.synchronize()
    hs = read_head(heads, n, O, head_pitch, offset)
    a, lp, en = (read_vectors(ts, n, True, what) for ts, what in ((act, "actions"), (logp, "log_probs"), (ent, "entropy")))
    return [dict(head=hs[s], actions=a[s].astype(np.int64), log_probs=lp[s].view(np.float32), entropy=en[s].view(np.float32),
                 values=np.ascontiguousarray(hs[s][:, A]) if O > A else None) for s in range(second + 1)]


def same_bits(got, want, what, keys=("head", "actions", "log_probs", "entropy", "values")):
    for s, (g, w) in enumerate(zip(got, want)):
        for key in keys:
            if key == "values" and g[key] is None and w[key] is None:  # (a net without a value column)
                continue
            assert g[key] is not None and w[key] is not None, (what, key)
            assert np.array_equal(bits(g[key]), bits(w[key])), (what, "side", s, key, int((bits(g[key]) != bits(w[key])).sum()), "elements differ")


# ---- 1. the bits of the two launches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AJ.N_EDGES)
def test_batch_sizes_return_the_bits_of_the_two_launches(libs, n):
    """every tile edge, one and several workgroups: two agents with nets of their own, head asked and not asked"""
    K, H, O, A = AJ.SIZES[0]
    obs, params = AJ.case_inputs(n, K, H, O)
    inp = Inputs(obs, "float32", params)
    want = run_two_launches(libs, inp, "tanh", A, AJ.DRAWS[0])
    with_head = run_act(libs, inp, "tanh", A, AJ.DRAWS[0])
    without = run_act(libs, inp, "tanh", A, AJ.DRAWS[0], head=False)
    same_bits(with_head, want, f"n = {n}")
    same_bits(without, want, f"n = {n} without the head", keys=("actions", "log_probs", "entropy", "values"))


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("K,H,O,A", AJ.SIZES)
def test_layer_sizes_and_activations(libs, K, H, O, A, activation):
    """... at pitches above the widths and a base offset of one element; one agent, and two agents on shared weights"""
    n = 129
    obs, params = AJ.case_inputs(n, K, H, O, seed=1)
    pitches = dict(head_pitch=O + 2, offset=1)
    for sides, shared in ((1, False), (2, True)):
        inp = Inputs(obs[:sides], "float32", params, obs_pitch=K + 3, offset=1, shared=shared)
        got = run_act(libs, inp, activation, A, AJ.DRAWS[1], **pitches)
        same_bits(got, run_two_launches(libs, inp, activation, A, AJ.DRAWS[1], **pitches), f"{K}-{H}-{O}-{A} {activation} {sides} side(s)")
        assert (got[0]["values"] is None) == (O == A)
        if sides == 1:
            one = got
    same_bits(one, got[:1], "a row's bits changed with the other agent present")


@pytest.mark.parametrize("action_dtype", J.ACTION_DTYPES)
@pytest.mark.parametrize("obs_dtype", N.OBS_DTYPES)
def test_formats(libs, obs_dtype, action_dtype):
    """the five observation formats (a 16-bit base offset by one element) into both action formats"""
    K, H, O, A = AJ.SIZES[0]
    obs, params = AJ.case_inputs(65, K, H, O, obs_dtype, seed=2)
    inp = Inputs(obs, obs_dtype, params, obs_pitch=K + 1, offset=1)
    got = run_act(libs, inp, "relu" if obs_dtype.startswith("int") else "tanh", A, AJ.DRAWS[0], action_dtype=action_dtype)
    same_bits(got, run_two_launches(libs, inp, "relu" if obs_dtype.startswith("int") else "tanh", A, AJ.DRAWS[0], action_dtype=action_dtype),
              f"{obs_dtype} {action_dtype}")


@pytest.mark.parametrize("draw_index", range(len(AJ.DRAWS)))
def test_draws_by_value_and_on_the_device(libs, draw_index):
    """game ids and steps beyond 2^32, and a device part that carries the step; log-prob and entropy NULL one at a time"""
    K, H, O, A = AJ.SIZES[0]
    obs, params = AJ.case_inputs(129, K, H, O, seed=3)
    inp = Inputs(obs, "float32", params)
    draw = AJ.DRAWS[draw_index]
    want = run_two_launches(libs, inp, "tanh", A, draw)
    same_bits(run_act(libs, inp, "tanh", A, draw), want, f"draw {draw_index}")
    for off in ("log_probs", "entropy", "values"):
        got = run_act(libs, inp, "tanh", A, draw, head=False, with_logp=off != "log_probs", with_ent=off != "entropy", with_val=off != "values")
        same_bits(got, want, f"draw {draw_index} without {off}", keys=[k for k in ("actions", "log_probs", "entropy", "values") if k != off])
    if draw[3] is not None:  # the whole step by value draws the same
        same_bits(run_act(libs, inp, "tanh", A, (draw[0], draw[1], draw[2] + draw[3], None), head=False), want, "the step by value",
                  keys=("actions", "log_probs", "entropy", "values"))


# ---- 2. the float64 judge, independent of the older kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(AJ.JUDGE_CASES)))
def test_against_the_float64_judge(libs, index):
    n, (K, H, O, A), activation, obs_dtype, draw_index = AJ.JUDGE_CASES[index]
    obs, params = AJ.case_inputs(n, K, H, O, obs_dtype, seed=index)
    got = run_act(libs, Inputs(obs, obs_dtype, params), activation, A, AJ.DRAWS[draw_index])
    us = AJ.uniforms(AJ.DRAWS[draw_index], n)
    for s in (0, 1):
        amb, fails = AJ.verdict(got[s], obs[s], params[s], activation, A, us[s], what=f"case {index} side {s}")
        assert not fails, fails


# ---- 3. planted rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b3_kind", AJ.PLANTED_B3)
def test_planted_rows(libs, b3_kind):
    """the exact construction: the head's logits are the planted ones bit for bit, and on them masked actions are never drawn,
    the +-80 and +-100 rows are finite, equal and one-hot rows give their closed forms, NaN and +inf rows give action 0 with NaN"""
    K, H, O, A = AJ.SIZES[0]
    n = 4 * 35 * 9 + 7
    x, params, logits, kind, masked = AJ.planted(n, K, H, O, A, b3_kind)
    draw = AJ.DRAWS[1]
    got = run_act(libs, Inputs([x], "float32", [params]), "relu", A, draw)[0]
    assert np.array_equal(got["head"][:, :A], logits, equal_nan=True)
    u = AJ.uniforms(draw, n)[0]
    a, amb, nb, st = J.sample(logits.astype(np.float64), u)
    act, logp, ent = got["actions"], got["log_probs"], got["entropy"]
    assert (act[~amb] == a[~amb]).all() and ((act >= nb[:, 0]) & (act <= nb[:, 1])).all() and amb.sum() <= AJ.CAP(n)
    k = np.array(kind)
    bad = st["bad"]
    assert (bad == ((k == "nan") | (b3_kind == "plus_inf"))).all()
    assert (act[bad] == 0).all() and np.isnan(logp[bad]).all() and np.isnan(ent[bad]).all()
    assert np.isfinite(logp[~bad]).all() and np.isfinite(ent[~bad]).all() and not masked[act[~bad]].any()
    want, tol = J.log_prob(st, act)
    assert (np.abs(logp.astype(np.float64) - want)[~bad] <= tol[~bad]).all()
    assert (np.abs(ent.astype(np.float64) - st["H"])[~bad] <= J.entropy_tolerance(st)[~bad]).all()
    assert np.array_equal(bits(got["values"]), bits(got["head"][:, A]))
    live = int((~masked).sum())
    if b3_kind == "one_hot":
        assert (act[~bad] == int(np.nonzero(~masked)[0][0])).all() and (logp[~bad] == 0).all() and (ent[~bad] == 0).all()
    elif b3_kind != "plus_inf":
        eq = k == "equal"
        assert eq.any() and np.allclose(ent[eq], np.log(live), rtol=0, atol=2e-6) and np.allclose(logp[eq], -np.log(live), rtol=0, atol=2e-6)
        assert len(set(act[eq])) > 1 and set(k[~bad]) == set(AJ.FINITE_KINDS)


# ---- 4. every wave past its first tile ----------------------------------------------------------------------------------------------
def rows_past_the_first_tile():
    """(compute units, n): pz_mlp_tile.hpp's grid cap admits at most two resident workgroups per compute unit, 2 CUs * 128 rows a
    trip of the tile loop.  Twice that, one more workgroup's worth and 37 rows: every wave takes at least two tiles at every
    hidden width and either agent count, the workgroups' tile counts differ, and the last tile has 5 live rows."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, 2 * (2 * cus) * 128 + 128 + 37


LARGE_SIZES = {32: (35, 32, 19, 18), 64: (35, 64, 19, 18), 128: (72, 128, 40, 32)}


@pytest.mark.parametrize("H", sorted(LARGE_SIZES))
def test_every_wave_past_its_first_tile(libs, H):
    K, _, O, A = LARGE_SIZES[H]
    cus, n = rows_past_the_first_tile()
    assert n % 32 == 5
    print(f"{cus} compute units: n = {n}")
    obs, params = AJ.case_inputs(n, K, H, O, seed=4)
    sides, activation = ((2, "tanh") if H == 64 else (1, "relu") if H == 32 else (2, "relu"))
    inp = Inputs(obs[:sides], "float32", params, obs_pitch=K + 3, offset=1)
    got = run_act(libs, inp, activation, A, AJ.DRAWS[2], head_pitch=O + 2, offset=1)
    same_bits(got, run_two_launches(libs, inp, activation, A, AJ.DRAWS[2], head_pitch=O + 2, offset=1), f"H = {H} n = {n}")


# ---- 5. shard, 6. n = 0 -----------------------------------------------------------------------------------------------------------
def test_a_shard_returns_the_bits_of_the_whole_batch_s_tail(libs):
    K, H, O, A = AJ.SIZES[0]
    n, g0 = 1000, 333
    obs, params = AJ.case_inputs(n, K, H, O, seed=5)
    seed, first, step, dev = AJ.DRAWS[1]
    whole = run_act(libs, Inputs(obs, "float32", params), "tanh", A, AJ.DRAWS[1])
    shard = run_act(libs, Inputs([x[g0:] for x in obs], "float32", params), "tanh", A, (seed, first + g0, step, dev))
    same_bits(shard, [{k: (v[g0:] if v is not None else None) for k, v in side.items()} for side in whole], "shard")
    assert not np.array_equal(shard[0]["actions"], whole[0]["actions"][:n - g0])


def test_zero_rows_launch_nothing(libs):
    K, H, O, A = AJ.SIZES[0]
    obs, params = AJ.case_inputs(0, K, H, O)
    run_act(libs, Inputs(obs, "float32", params), "tanh", A, AJ.DRAWS[0])  # (every sentinel intact: checked by the reader)


# ---- 7. the binding -------------------------------------------------------------------------------------------------------------------
def test_act_sample_its_out_argument_and_the_module(libs):
    from pikazoo_amd import act, net, policy

    torch.manual_seed(0)
    model = net.ActorCritic(in_features=35, hidden=64, num_actions=18).to("cuda:0")
    with torch.no_grad():
        model.head.weight.mul_(100.0)  # (logits worth drawing from)
    n = 777
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    obs = {a: torch.rand((n, 35), device="cuda:0", generator=gen) for a in (A1, A2)}
    head = model.act(obs)
    want = policy.sample({a: h[:, :18] for a, h in head.items()}, seed=11, step=9, first_game=5)
    out = model.act_sample(obs, seed=11, step=9, first_game=5, head=True)
    ptrs = {k: {a: t.data_ptr() for a, t in v.items()} for k, v in out.items()}
    again = model.act_sample(obs, seed=11, step=9, first_game=5, head=True, out=out)
    plain = act.sample(obs, model.parameter_tensors(), 18, seed=11, step=torch.tensor([4], device="cuda:0") + 5, first_game=5, action_dtype=torch.int32)
    one = model.act_sample(obs[A1], seed=11, step=9, first_game=5)
    torch.cuda.synchronize()
    assert again is out and ptrs == {k: {a: t.data_ptr() for a, t in v.items()} for k, v in out.items()}
    assert list(out) == ["actions", "log_probs", "entropy", "values", "head"] and list(plain) == ["actions", "log_probs", "entropy", "values"]
    assert out["actions"][A1].dtype == torch.int64 and plain["actions"][A1].dtype == torch.int32 and isinstance(one["actions"], torch.Tensor)
    assert len(set(cpu(out["actions"][A1]).tolist())) > 4
    for a in (A1, A2):
        for key in ("actions", "log_probs", "entropy"):
            assert np.array_equal(bits(cpu(out[key][a])), bits(cpu(want[key][a]))), (a, key)
            assert np.array_equal(bits(cpu(plain[key][a]).astype(cpu(want[key][a]).dtype)), bits(cpu(want[key][a]))), (a, key)
        assert np.array_equal(bits(cpu(out["head"][a])), bits(cpu(head[a]))) and np.array_equal(bits(cpu(out["values"][a])), bits(cpu(head[a][:, 18])))
        assert np.array_equal(bits(cpu(plain["values"][a])), bits(cpu(out["values"][a])))
    for key in one:
        assert np.array_equal(bits(cpu(one[key])), bits(cpu(out[key][A1]))), key
    # a net without a value column: no "values"
    flat = [p.detach() for p in model.parameter_tensors()[:4]] + [model.head.weight.detach()[:18].contiguous(), model.head.bias.detach()[:18].contiguous()]
    assert list(act.sample(obs, flat, 18, seed=1)) == ["actions", "log_probs", "entropy"]
    for bad in (lambda: act.sample(obs, flat, 18, seed=1, out=out), lambda: model.act_sample(obs, seed=1, out=plain),
                lambda: model.act_sample(obs, seed=1, step=torch.zeros(1, dtype=torch.int64)),
                lambda: act.sample(obs, model.parameter_tensors(), 18, seed=1, head=True, out={**out, "head": obs}),
                lambda: act.sample(obs, model.parameter_tensors(), 18, seed=1, out={**plain, "values": {A1: obs[A1][:, 0], A2: obs[A2][:, 1]}})):
        with pytest.raises(ValueError):
            bad()


def test_graph_capture_with_a_device_step_counter():
    """one act launch and ``counter.add_(1)`` captured on a side stream: three replays equal three eager calls at steps t, t + 1
    and t + 2, bit for bit"""
    from pikazoo_amd import net

    torch.manual_seed(1)
    model = net.ActorCritic().to("cuda:0")
    with torch.no_grad():
        model.head.weight.mul_(100.0)
    n, t0 = 191, 40
    obs = {a: torch.rand((n, 35), device="cuda:0") for a in (A1, A2)}
    eager = []
    for step in range(t0, t0 + 3):
        out = model.act_sample(obs, seed=3, step=step, first_game=77)
        torch.cuda.synchronize()
        eager.append({key: {a: cpu(t).copy() for a, t in out[key].items()} for key in out})
    assert not np.array_equal(eager[0]["actions"][A1], eager[1]["actions"][A1])
    counter = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    held = model.act_sample(obs, seed=3, step=counter, first_game=77)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = model.act_sample(obs, seed=3, step=counter, first_game=77, out=held)
            counter.add_(1)
    assert captured is held
    torch.cuda.synchronize()
    counter.fill_(t0)
    torch.cuda.synchronize()
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for key in held:
            for a in (A1, A2):
                assert np.array_equal(bits(cpu(held[key][a])), bits(eager[step][key][a])), (step, key, a)
    assert int(counter.item()) == t0 + 3


def test_env_step_takes_the_actions_as_they_are():
    from pikazoo_amd import net, pikazoo_v0

    env = pikazoo_v0.env(num_envs=64, device="cuda:0", seed=5)
    obs, _ = env.reset()
    model = net.ActorCritic(in_features=obs[A1].shape[1]).to("cuda:0")
    out = None
    for t in range(3):
        out = model.act_sample(obs, seed=5, step=t, out=out)
        assert out["actions"][A1].dtype == torch.int64
        before = {a: out["actions"][a].data_ptr() for a in (A1, A2)}
        obs, rew, term, trunc, infos = env.step(out["actions"])
        assert {a: out["actions"][a].data_ptr() for a in (A1, A2)} == before
    env.unwrapped.check_actions()
    assert int(out["actions"][A1].max()) < 18 and int(out["actions"][A2].min()) >= 0


# ---- 8. the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native_batch", [False, True])
def test_the_example_returns_the_same_losses_with_the_fused_launch(native_batch):
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    kw = dict(num_envs=256, iters=2, steps=8, log=lambda *_: None, native_batch=native_batch)
    two = ppo_selfplay.main(**kw)
    fused = ppo_selfplay.main(fused_act=True, **kw)
    assert len(two) == 2 * 2 * 4 and all(np.isfinite(two)) and fused == two
