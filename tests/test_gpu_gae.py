"""GPU tests (``-m gpu``) of ``pz_gae`` (include/pikazoo_learn.h, the ``pz_learn::gae_kernel`` family) and of
``pikazoo_amd.learn.gae`` / ``raw_env.gae``.

The judge is tests/gae_judge.py: the header's arithmetic in numpy float32 (held to exact rational arithmetic and to the
float64 formula by tests/test_gae_host.py).  Every launch is compared with it BIT FOR BIT (uint32 views of the float32
outputs); no GPU result is ever the expected value.  Every C-ABI launch goes into sentinel-filled outputs with columns
beyond n and elements behind the last row, which must keep the sentinel; the inputs must be unchanged; a second launch
must give the same bits.
"""
import numpy as np
import pytest
import torch

import gae_judge as J

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
SENT = -7   # the int32 pattern the outputs hold before a launch (as float32 a NaN no arithmetic here produces)
TAIL = 64   # elements behind the last row of every buffer
GAMMA, LAM = 0.99, 0.95
TORCH_VALUE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def cpu(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from pikazoo_amd import learn

    return learn.load()


def device_rows(host, pitch, fill):
    """host [rows, n] -> a flat device tensor of rows * pitch + TAIL elements holding it at `pitch`, `fill` elsewhere"""
    rows, n = host.shape
    flat = np.full(rows * pitch + TAIL, fill, host.dtype)
    flat[:rows * pitch].reshape(rows, pitch)[:, :n] = host
    if flat.dtype == np.uint16:  # (bfloat16 patterns: the launch takes a pointer, torch an integer type it knows)
        flat = flat.view(np.int16)
    return torch.from_numpy(flat).to("cuda:0")


def check_abi_case(lib, c, reward_dtype, value_dtype, pitches=(J.PITCH,) * 4, both=True, gamma=GAMMA, lam=LAM, nan_rows=()):
    """one case of gae_judge.make_case through the C ABI at the pitches (reward, flag, value, output); `nan_rows`: rows
    whose outputs the case makes non-finite -- a NaN that arithmetic produces has no pinned sign, so these rows must be
    non-finite where the judge's are and are not compared as bits"""
    k, n = c["k"], c["n"]
    rp, tp, vp, op = pitches
    sides = 2 if both else 1
    rew_h = [np.ascontiguousarray(r) for r in c["rew"][:sides]]
    val_h = [J.value_bits(v, value_dtype) for v in c["val"][:sides]]
    rew = [device_rows(r, rp, r.dtype.type(9)) for r in rew_h]
    val = [device_rows(v, vp, v.dtype.type(3)) for v in val_h]
    term = device_rows(c["d"], tp, np.uint8(1))
    before = [cpu(t).copy() for t in rew + val + [term]]
    fmt_r, fmt_v = J.REWARD_DTYPES.index(reward_dtype), J.VALUE_DTYPES.index(value_dtype)
    stream = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        outs = [torch.full((k * op + TAIL,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(2 * sides)]
        adv, ret = outs[:sides], outs[sides:]
        err = lib.pz_gae(rew[0].data_ptr(), rew[1].data_ptr() if both else None, fmt_r, term.data_ptr(), val[0].data_ptr(),
                         val[1].data_ptr() if both else None, fmt_v, k, n, rp, tp, vp, op, gamma, lam, adv[0].data_ptr(),
                         adv[1].data_ptr() if both else None, ret[0].data_ptr(), ret[1].data_ptr() if both else None, stream)
        assert err == 0
        torch.cuda.synchronize()
        runs.append([cpu(o) for o in outs])
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two launches differ"
    for side in range(sides):
        want_adv, want_ret = J.judge(c["rew"][side], c["d"], c["val"][side], gamma, lam)
        for got, want, what in ((runs[0][side], want_adv, "advantages"), (runs[0][sides + side], want_ret, "returns")):
            rows = got[:k * op].reshape(k, op)
            where = (k, n, reward_dtype, value_dtype, pitches, side, what)
            keep = [t for t in range(k) if t not in nan_rows]
            assert np.array_equal(rows[keep, :n].view(np.uint32), bits(want[keep])), where
            for t in nan_rows:
                assert np.array_equal(np.isfinite(rows[t, :n].view(np.float32)), np.isfinite(want[t])) and not np.isfinite(want[t]).all(), where
            assert (rows[:, n:] == SENT).all() and (got[k * op:] == SENT).all(), where
    for t, b in zip(rew + val + [term], before):
        assert cpu(t).tobytes() == b.tobytes(), "an input changed"  # (as bytes: a planted NaN equals itself)


@pytest.mark.parametrize("n", J.N_EDGES)
def test_sizes_and_chunk_edges(lib, n):
    """every k of gae_judge.K_EDGES -- 1, 2, 130 and both sides of 8, 16, 24 and 32 (kChunk = 8 rows per load-ahead buffer,
    two chunks per trip of the main loop: tests/gae_judge.py) -- at n below, at and above one wave, pitch 256"""
    for k in J.K_EDGES:
        check_abi_case(lib, J.make_case(k, n, "random10", seed=1), "float32", "float32")


def test_pitch_equal_to_n(lib):
    for k, n in ((33, 200), (8, 65)):
        check_abi_case(lib, J.make_case(k, n, "random10", seed=2), "float32", "float32", pitches=(n,) * 4)


@pytest.mark.parametrize("pattern", J.FLAG_PATTERNS)
def test_flag_patterns(lib, pattern):
    for k in (1, 17, 130):
        check_abi_case(lib, J.make_case(k, 200, pattern, seed=3), "float32", "float32")


@pytest.mark.parametrize("value_dtype", J.VALUE_DTYPES)
@pytest.mark.parametrize("reward_dtype", J.REWARD_DTYPES)
def test_formats(lib, reward_dtype, value_dtype):
    for k, n in ((33, 200), (7, 65)):
        check_abi_case(lib, J.make_case(k, n, "random10", reward_dtype, value_dtype, seed=4), reward_dtype, value_dtype)


def test_one_side_only(lib):
    for rf, vf in (("int32", "float32"), ("float32", "bfloat16")):
        check_abi_case(lib, J.make_case(33, 200, "random10", rf, vf, seed=5), rf, vf, both=False)


def test_four_different_pitches(lib):
    for rf, vf in (("float32", "float32"), ("int32", "float16")):
        check_abi_case(lib, J.make_case(33, 200, "random50", rf, vf, seed=6), rf, vf, pitches=(256, 320, 208, 264))


def test_lambda_and_gamma_at_their_ends(lib):
    """lam = 1: bootstrapped Monte-Carlo returns; lam = 0: TD(0); gamma = 0: the reward minus the value"""
    for gamma, lam in ((0.99, 1.0), (0.99, 0.0), (0.0, 0.95), (1.0, 1.0)):
        check_abi_case(lib, J.make_case(17, 65, "random10", seed=7), "float32", "float32", gamma=gamma, lam=lam)


def test_nothing_crosses_an_episode_end(lib):
    """an infinite or NaN value behind a flagged row must not reach the rows in front of it: a select, not a multiply"""
    c = J.make_case(9, 65, "none", seed=8)
    c["d"][4] = 1
    for v in c["val"]:
        v[5, ::2], v[5, 1::2] = np.inf, np.nan
    check_abi_case(lib, c, "float32", "float32", nan_rows=(5,))
    adv, ret = J.judge(c["rew"][0], c["d"], c["val"][0], GAMMA, LAM)
    assert np.isfinite(adv[:5]).all() and np.isfinite(ret[:5]).all() and not np.isfinite(adv[5]).any()
    assert np.isfinite(adv[6:]).all()  # (row 5's value is row 4's v[t+1] alone: row 4 is flagged)


# ---- through the env -------------------------------------------------------------------------------------------------
TABLE = (0.0, -0.01, 0.0, 0.01, 0.0, 0.01, 0.0, -0.01)


def recipe_env(kind):
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd.wrappers import RewardByBallPosition

    rc = J.RECIPE
    kw = dict(num_envs=rc["n"], device="cuda:0", seed=rc["seed"], winning_score=rc["winning_score"], env_id_base=rc["env_id_base"])
    if kind == "frame_skip4":
        env = pikazoo_v0.env(frame_skip=4, **kw)
    else:
        env = pikazoo_v0.env(**kw)
    if kind == "ball_position":
        wrapped = RewardByBallPosition(env, additional_reward=TABLE, x_line=216, y_line=176)
        assert wrapped.fused
    env.reset()
    raw = env.unwrapped
    if kind == "frame_skip4":
        return raw, raw.rollout_random_held(rc["action_seed"], k=32)
    return raw, raw.rollout_random(rc["action_seed"], k=rc["frames"])


@pytest.fixture(scope="module", params=["plain", "ball_position", "frame_skip4"])
def trajectory(request):
    raw, traj = recipe_env(request.param)
    torch.cuda.synchronize()
    want = {"plain": torch.int32, "ball_position": torch.float32, "frame_skip4": torch.int32}[request.param]
    assert traj["rewards"][A1].dtype == want
    d = cpu(traj["terminations"]).astype(np.uint8)
    assert d.any() and not d.all()
    if request.param != "frame_skip4":  # (the recipe's census: tests/test_gae_host.py runs it on the CPU)
        assert (d.astype(np.int64).sum(0) >= 2).sum() >= 200
    return raw, traj, d


@pytest.mark.parametrize("value_dtype", ["float32", "bfloat16"])
def test_env_gae_equals_the_judge_on_the_trajectory(trajectory, value_dtype):
    raw, traj, d = trajectory
    k, n = d.shape
    rng = np.random.default_rng(21)
    val_h = {a: J.as_value_dtype(rng.normal(0.0, 1.5, size=(k + 1, n)).astype(np.float32), value_dtype) for a in (A1, A2)}
    values = {a: torch.from_numpy(v).to("cuda:0").to(TORCH_VALUE[value_dtype]) for a, v in val_h.items()}
    for a in (A1, A2):  # (the device tensor holds exactly the judge's values)
        assert np.array_equal(cpu(values[a].to(torch.float32)), val_h[a])
    out = raw.gae(traj, values, gamma=GAMMA, lam=LAM)
    torch.cuda.synchronize()
    assert list(out) == ["advantages", "returns"] and list(out["advantages"]) == [A1, A2]
    for a in (A1, A2):
        adv, ret = J.judge(cpu(traj["rewards"][a]), d, val_h[a], GAMMA, LAM)
        assert np.array_equal(bits(cpu(out["advantages"][a])), bits(adv)), a
        assert np.array_equal(bits(cpu(out["returns"][a])), bits(ret)), a
    # one side as a bare tensor: player_1, the same bits, and the buffers of out= are the ones written
    one = raw.gae(traj, values[A1], gamma=GAMMA, lam=LAM)
    again = raw.gae(traj, values, gamma=GAMMA, lam=LAM, out=out)
    torch.cuda.synchronize()
    assert again is out and isinstance(one["advantages"], torch.Tensor)
    assert torch.equal(one["advantages"].view(torch.int32), out["advantages"][A1].view(torch.int32))
    assert torch.equal(one["returns"].view(torch.int32), out["returns"][A1].view(torch.int32))


def test_row_strides_and_uint8_flags():
    """learn.gae on views with row strides of their own (every second row of a taller tensor, a column window)"""
    from pikazoo_amd import learn

    c = J.make_case(17, 200, "random10", "int32", "float16", seed=9)
    k, n = c["k"], c["n"]
    big_r = torch.zeros((2 * k, n + 8), dtype=torch.int32, device="cuda:0")
    big_v = torch.zeros((k + 1, n + 24), dtype=torch.float16, device="cuda:0")
    r, v = big_r[::2, 8:], big_v[:, 3:n + 3]
    r.copy_(torch.from_numpy(c["rew"][0]))
    v.copy_(torch.from_numpy(c["val"][0]))
    d = torch.from_numpy(c["d"]).to("cuda:0")
    want_adv, want_ret = J.judge(c["rew"][0], c["d"], c["val"][0], GAMMA, LAM)
    for flags in (d, d.view(torch.bool)):
        out = learn.gae(r, v, flags, GAMMA, LAM)
        torch.cuda.synchronize()
        assert np.array_equal(bits(cpu(out["advantages"])), bits(want_adv)) and np.array_equal(bits(cpu(out["returns"])), bits(want_ret))


def test_graph_capture_replays_to_the_eager_bits():
    from pikazoo_amd import learn

    c = J.make_case(33, 200, "random10", seed=10)
    rew = {a: torch.from_numpy(r).to("cuda:0") for a, r in zip((A1, A2), c["rew"])}
    val = {a: torch.from_numpy(v).to("cuda:0") for a, v in zip((A1, A2), c["val"])}
    d = torch.from_numpy(c["d"]).to("cuda:0").view(torch.bool)
    eager = learn.gae(rew, val, d, GAMMA, LAM)
    torch.cuda.synchronize()
    want = {key: {a: cpu(t).copy() for a, t in eager[key].items()} for key in eager}
    prev = learn.gae(rew, val, d, GAMMA, LAM)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = learn.gae(rew, val, d, GAMMA, LAM, out=prev)
    assert captured is prev
    torch.cuda.synchronize()
    for key in prev:
        for t in prev[key].values():
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for key in want:
        for a in (A1, A2):
            assert np.array_equal(bits(cpu(prev[key][a])), bits(want[key][a])), (key, a)
            assert np.array_equal(bits(want[key][a]), bits(J.judge(c["rew"][(A1, A2).index(a)], c["d"], c["val"][(A1, A2).index(a)],
                                                                  GAMMA, LAM)[key == "returns"]))


def test_mismatched_shapes_devices_dtypes_and_ranges_raise_value_error():
    from pikazoo_amd import learn

    dev = "cuda:0"
    r, v, d = torch.zeros(4, 8, device=dev), torch.zeros(5, 8, device=dev), torch.zeros(4, 8, dtype=torch.bool, device=dev)
    learn.gae(r, v, d)
    for bad in (lambda: learn.gae(r, torch.zeros(4, 8, device=dev), d),            # values need k + 1 rows
                lambda: learn.gae(r, v, torch.zeros(4, 9, dtype=torch.bool, device=dev)),
                lambda: learn.gae(r, v.cpu(), d),                                   # another device
                lambda: learn.gae(r, v, d.cpu()),
                lambda: learn.gae(r.to(torch.float64), v, d),                       # dtypes
                lambda: learn.gae(r, v.to(torch.float64), d),
                lambda: learn.gae(r, v, d.to(torch.int32)),
                lambda: learn.gae({A1: r, A2: r.to(torch.int32)}, {A1: v, A2: v}, d),
                lambda: learn.gae(r, v, d, gamma=1.5),                              # ranges
                lambda: learn.gae(r, v, d, lam=float("nan")),
                lambda: learn.gae(r.t().contiguous().t(), v, d),                    # the last dimension must be contiguous
                lambda: learn.gae(r, v, d, out={"advantages": torch.zeros(4, 9, device=dev), "returns": torch.zeros(4, 8, device=dev)})):
        with pytest.raises(ValueError):
            bad()
