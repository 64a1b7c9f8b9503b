"""GPU tests (``-m gpu``) of the policy-rollout launch (include/pikazoo_rollout.h: ``pz_rollout_policy``), of
``raw_env.rollout_policy`` and of ``ActorCritic.rollout``.

Two references, kept apart.  (1) The header's promise: two envs from the same seed, one runs ``rollout_policy(k)``, the other
``k`` x (``act.sample`` -- what ``model.act_sample`` calls --; ``env.step``) and then ``net.forward`` for the bootstrap value;
every slab of every output, the final state, ``steps_done``, the episode statistics and the episode counter are compared for
equality, one axis swept per test.  (2) Independent of the older kernels: the C oracle, stepped with the actions the launch
reported, reproduces the observations, rewards, flags and the final state, and the float64 judge of tests/act_judge.py passes
each slab's (observations, action, log-prob, entropy, value) within its own derived tolerance and ambiguity width.  One case
goes through the C ABI with every output between sentinel guards -- in front, behind and in the pad rows of every slab -- and
NaN patterns around the parameters.  The sweep over the launch's runtime configurations, from planted states, lives in
tests/test_gpu_policy_rollout_configs.py (its cases: tests/policy_rollout_configs.py).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import act_judge as AJ
import net_judge as N
import policy_judge as J
import policy_rollout_cases as RC
from test_gpu_net import device_params
from test_gpu_policy import SENT, TAIL, cpu, stream

pytestmark = pytest.mark.gpu

A1, A2 = "player_1", "player_2"
AGENTS = (A1, A2)
REPO = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
TABLE = (0.0, -0.01, 0.0, 0.01, 0.0, 0.01, 0.0, -0.01)
FRONT = 8  # elements in front of every output (8: an int64 vector stays aligned)


def make_env(n, stack="plain", auto_reset=True, winning_score=15, seed=RC.ENV_SEED):
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd.wrappers import NormalizeObservation, RecordEpisodeStatistics, RewardByBallPosition, SimplifyAction

    env = pikazoo_v0.env(num_envs=n, device=DEV, seed=seed, winning_score=winning_score, auto_reset=auto_reset)
    if stack == "normalize":
        env = NormalizeObservation(env)
    elif stack == "stats":
        env = RecordEpisodeStatistics(NormalizeObservation(env))
    elif stack == "full":      # every wrapper the kernel fuses: 13 actions, float rewards, float32 rows, statistics
        env = RecordEpisodeStatistics(NormalizeObservation(RewardByBallPosition(SimplifyAction(env), TABLE)))
    elif stack == "reward above normalize":   # RewardByBallPosition then reads NORMALISED coordinates: it runs outside the kernel
        return RecordEpisodeStatistics(RewardByBallPosition(NormalizeObservation(SimplifyAction(env)), TABLE))
    else:
        assert stack == "plain"
    assert not env.unwrapped._unfused
    return env


def oracle_env(n, stack, auto_reset=True, winning_score=15, seed=RC.ENV_SEED):
    from oracle import pz_oracle as po

    kw = dict(winning_score=winning_score, auto_reset=auto_reset, seed=seed)
    if stack in ("normalize", "stats", "full"):
        kw["normalize_obs"] = True
    if stack == "stats":
        kw["episode_stats"] = 1
    if stack == "full":
        kw.update(simplify_action=True, additional_reward=TABLE, episode_stats=2)
    return po.OracleEnv(n, po.make_config(**kw))


def host_params(H, A, seed):
    return N.make_params(35, H, A + 1, seed)


def make_model(H, A, activation="tanh", seed=1):
    """an ActorCritic whose parameters are net_judge's (logits far enough from uniform for the draw to matter)"""
    from pikazoo_amd import net

    model = net.ActorCritic(in_features=35, hidden=H, num_actions=A, activation=activation).to(DEV)
    with torch.no_grad():
        for p, value in zip(model.parameter_tensors(), host_params(H, A, seed)):
            p.copy_(torch.from_numpy(value))
    return model


def parameter_sets(models):
    """what act.sample and net.forward take: one sequence (shared weights) or a dict of them"""
    if isinstance(models, dict):
        return {a: m.parameter_tensors() for a, m in models.items()}, models[A1].activation
    return models.parameter_tensors(), models.activation


def launches_route(env, models, k, seed, step=0, first_game=0, action_dtype=torch.int64, obs=None):
    """the launches the rollout replaces: k x (act.sample; env.step), then net.forward for the bootstrap value"""
    from pikazoo_amd import act, net

    raw = env.unwrapped
    A = raw.n_actions
    params, activation = parameter_sets(models)
    obs = obs if obs is not None else raw._pack_obs()
    rec = {key: {a: [] for a in AGENTS} for key in ("obs", "actions", "log_probs", "values", "entropy", "rewards")}
    rec["terminations"] = []
    with torch.no_grad():
        for t in range(k):
            picked = act.sample(obs, params, A, seed, step=step + t, first_game=first_game, activation=activation, action_dtype=action_dtype)
            for a in AGENTS:
                rec["obs"][a].append(obs[a].clone())
                for key in ("actions", "log_probs", "values", "entropy"):
                    rec[key][a].append(picked[key][a].clone())
            obs, rewards, terminations, _, _ = env.step(picked["actions"])
            for a in AGENTS:
                rec["rewards"][a].append(rewards[a].clone())
            rec["terminations"].append(terminations[A1].clone())
        head = net.forward(obs, params, activation)
    for a in AGENTS:
        rec["obs"][a].append(obs[a].clone())
        rec["values"][a].append(head[a][:, A].clone())
    out = {key: {a: torch.stack(rec[key][a]) for a in AGENTS} for key in rec if key != "terminations"}
    out["terminations"] = torch.stack(rec["terminations"])
    return out


def bits(t):
    x = np.ascontiguousarray(cpu(t))
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same_buffers(got, want, what, entropy=True):
    for key in ("obs", "actions", "log_probs", "values", "rewards") + (("entropy",) if entropy else ()):
        for a in AGENTS:
            g, w = got[key][a], want[key][a]
            assert g.shape == w.shape and g.dtype == w.dtype, (what, key, a, g.shape, w.shape, g.dtype, w.dtype)
            diff = bits(g) != bits(w)
            assert not diff.any(), (what, key, a, int(diff.sum()), "elements differ, first slab", int(np.nonzero(diff.reshape(diff.shape[0], -1).any(1))[0][0]))
    assert entropy or "entropy" not in got
    assert got["terminations"].dtype == torch.bool and np.array_equal(cpu(got["terminations"]), cpu(want["terminations"])), (what, "terminations")


def same_envs(a, b, what):
    ra, rb = a.unwrapped, b.unwrapped
    assert np.array_equal(cpu(ra.read_state()), cpu(rb.read_state())), (what, "the final state")
    assert ra.steps_done == rb.steps_done, (what, "steps_done")
    assert ra.episodes_done == rb.episodes_done, (what, "the episode counter")
    if ra.episode_returns is not None:
        assert np.array_equal(cpu(ra.episode_returns).view(np.uint64), cpu(rb.episode_returns).view(np.uint64)), (what, "episode returns")
        assert np.array_equal(cpu(ra.episode_lengths), cpu(rb.episode_lengths)), (what, "episode lengths")
    # the env-owned single-frame views follow the last slab
    for x, y in zip(ra._pack_obs().values(), rb._pack_obs().values()):
        assert np.array_equal(bits(x), bits(y)), (what, "the env's own observation rows")
    for x, y in zip(ra._rewards(), rb._rewards()):
        assert np.array_equal(bits(x), bits(y)), (what, "the env's own rewards")
    assert np.array_equal(cpu(ra._term), cpu(rb._term)), (what, "the env's own flags")


def both_routes(n, k, models, stack="plain", seed=7, step=0, first_game=0, action_dtype=torch.int64, entropy=True, **env_kw):
    """(the rollout's result, the launches' records, the two envs)"""
    ea, eb = make_env(n, stack, **env_kw), make_env(n, stack, **env_kw)
    ea.reset()
    eb.reset()
    got = ea.unwrapped.rollout_policy(models, k, seed, step=step, first_game=first_game, action_dtype=action_dtype, entropy=entropy)
    want = launches_route(eb, models, k, seed, step=step, first_game=first_game, action_dtype=action_dtype)
    torch.cuda.synchronize()
    return got, want, ea, eb


# ---- 1. the bits of the launches it replaces ---------------------------------------------------------------------------------------
# 4, 28: a partial tile; 32: exactly one; 36: one and a part (the second pair of waves has live rows); 64: a whole workgroup;
# 68, 132: more than one workgroup, the last one partial.  The grid is one workgroup per 64 games without a cap: no workgroup
# takes two groups at any n.
@pytest.mark.parametrize("n", (4, 28, 32, 36, 64, 68, 132))
def test_batch_sizes_return_the_bits_of_the_launches(n):
    model = make_model(64, 18)
    got, want, ea, eb = both_routes(n, 5, model)
    same_buffers(got, want, f"n = {n}")
    same_envs(ea, eb, f"n = {n}")
    assert got["obs"][A1].shape == (6, n, 35) and got["values"][A2].shape == (6, n) and got["actions"][A1].shape == (5, n)
    assert len({int(x) for x in cpu(got["actions"][A1]).ravel()}) > 4   # (a draw worth comparing)


@pytest.mark.parametrize("k", (1, 2, 5))
@pytest.mark.parametrize("weights", ("shared", "separate"))
def test_steps_and_weights(k, weights):
    """k = 1 at a batch that is no multiple of 4 (its slabs are not 16-byte aligned: the dword flush), and normalised rows"""
    models = make_model(64, 18) if weights == "shared" else {A1: make_model(64, 18, seed=1), A2: make_model(64, 18, seed=2)}
    n = 67 if k == 1 else 68
    got, want, ea, eb = both_routes(n, k, models, stack="normalize", step=3)
    same_buffers(got, want, f"k = {k} {weights}")
    same_envs(ea, eb, f"k = {k} {weights}")
    assert got["obs"][A1].dtype == torch.float32 and ea.unwrapped.steps_done == k
    if weights == "separate":   # the second agent really runs on its own net
        other, _, _, _ = both_routes(n, k, models[A1], stack="normalize", step=3)
        assert np.array_equal(bits(other["values"][A1][0]), bits(got["values"][A1][0]))
        assert not np.array_equal(bits(other["values"][A2][0]), bits(got["values"][A2][0]))


@pytest.mark.parametrize("activation", N.ACTIVATIONS)
@pytest.mark.parametrize("hidden", (32, 64, 128))
def test_hidden_widths_and_activations(hidden, activation):
    """shared and separate weights at every width; hidden 128 with a set per agent does not fit the LDS and is refused"""
    n, k = 36, 2
    shared = make_model(hidden, 18, activation, seed=3)
    got, want, ea, eb = both_routes(n, k, shared, step=11)
    same_buffers(got, want, f"{hidden} {activation} shared")
    same_envs(ea, eb, f"{hidden} {activation} shared")
    pair = {A1: shared, A2: make_model(hidden, 18, activation, seed=4)}
    if hidden == 128:
        env = make_env(n)
        env.reset()
        before = cpu(env.unwrapped.read_state())
        with pytest.raises(ValueError, match="LDS"):
            env.unwrapped.rollout_policy(pair, k, 7)
        assert np.array_equal(cpu(env.unwrapped.read_state()), before) and env.unwrapped.steps_done == 0
        return
    got, want, ea, eb = both_routes(n, k, pair, step=11)
    same_buffers(got, want, f"{hidden} {activation} separate")
    same_envs(ea, eb, f"{hidden} {activation} separate")


@pytest.mark.parametrize("action_dtype", (torch.int32, torch.int64))
def test_the_full_wrapper_stack(action_dtype):
    """RecordEpisodeStatistics(NormalizeObservation(RewardByBallPosition(SimplifyAction(env)))), the order in which the kernel
    fuses all four: 13 actions, float rewards, float32 rows, statistics; both action dtypes; entropy asked for and not"""
    n, k = 132, 5
    model = make_model(64, 13, seed=5)
    entropy = action_dtype == torch.int32
    got, want, ea, eb = both_routes(n, k, model, stack="full", action_dtype=action_dtype, entropy=entropy, step=2)
    same_buffers(got, want, f"full stack {action_dtype}", entropy=entropy)
    same_envs(ea, eb, f"full stack {action_dtype}")
    assert got["actions"][A1].dtype == action_dtype and int(cpu(got["actions"][A1]).max()) < 13
    assert got["rewards"][A1].dtype == torch.float32 and got["obs"][A2].dtype == torch.float32
    assert float(cpu(ea.unwrapped.episode_lengths).min()) == k


def test_a_stack_with_a_wrapper_outside_the_kernel_is_refused():
    """RecordEpisodeStatistics(RewardByBallPosition(NormalizeObservation(SimplifyAction(env)))): a RewardByBallPosition ABOVE
    NormalizeObservation reads normalised coordinates (as the reference's does), which the kernel does not fuse; it and the
    statistics above it run on the step's outputs, and the launch refuses the env before it touches it"""
    env = make_env(36, "reward above normalize")
    env.reset()
    raw = env.unwrapped
    assert raw._unfused == ["RewardByBallPosition", "RecordEpisodeStatistics"]
    before = cpu(raw.read_state())
    with pytest.raises(ValueError, match="RewardByBallPosition, RecordEpisodeStatistics of this stack run outside the kernel"):
        raw.rollout_policy(make_model(64, 13, seed=5), 2, 7)
    assert np.array_equal(cpu(raw.read_state()), before) and raw.steps_done == 0


@pytest.mark.parametrize("n,auto_reset", RC.TERMINATING_CASES)
def test_games_that_end_inside_the_launch(n, auto_reset):
    """winning_score = 1 and the k of tests/test_policy_rollout_host.py: games end before the last slab; with auto_reset they
    are reset in place by the next step's frame and play on inside the launch, without they freeze"""
    k = RC.TERMINATING_K
    model = make_model(64, 18, seed=6)
    got, want, ea, eb = both_routes(n, k, model, stack="stats", winning_score=1, auto_reset=auto_reset, entropy=False)
    term = cpu(got["terminations"])
    first = np.where(term.any(0), term.argmax(0), k)
    early = first < k - 1
    print(f"n = {n} auto_reset = {auto_reset}: {int(early.sum())} games end before the last slab, the first at t = {int(first.min())}")
    assert early.any(), "no game ended before the last slab: the case proves nothing about the in-launch reset"
    for g in np.nonzero(early)[0]:
        if auto_reset:
            assert not term[first[g] + 1, g]   # reset in place and playing
        else:
            assert term[first[g]:, g].all() and not cpu(got["rewards"][A1])[first[g] + 1:, g].any()   # frozen: flag up, reward 0
    same_buffers(got, want, f"terminating n = {n} auto_reset = {auto_reset}", entropy=False)
    same_envs(ea, eb, f"terminating n = {n} auto_reset = {auto_reset}")


def test_step_on_the_device_and_game_ids_beyond_32_bits():
    """`step` by value beyond 2^32, on the device, and first_game > 2^32: the draws of the launches at the same counters"""
    n, k = 36, 2
    model = make_model(64, 18, seed=7)
    first_game, step = (1 << 32) + 5, (1 << 33) + 1
    for how in ("value", "device"):
        ea, eb = make_env(n), make_env(n)
        ea.reset()
        eb.reset()
        counter = torch.tensor([step], dtype=torch.int64, device=DEV)
        got = ea.unwrapped.rollout_policy(model, k, 7, step=step if how == "value" else counter, first_game=first_game)
        want = launches_route(eb, model, k, 7, step=step, first_game=first_game)
        same_buffers(got, want, f"step by {how}", entropy=False)
        same_envs(ea, eb, f"step by {how}")
        assert int(counter.item()) == step   # (the launch reads the counter; the caller moves it)
    plain = make_env(n)
    plain.reset()
    other = plain.unwrapped.rollout_policy(model, k, 7)
    assert not np.array_equal(cpu(other["actions"][A1]), cpu(got["actions"][A1]))


def test_a_second_call_reuses_the_buffers_and_the_forwarder():
    """out= the previous result: no new tensors, the next k steps; ActorCritic.rollout forwards to the env's method"""
    n, k = 68, 2
    model = make_model(64, 18, seed=8)
    ea, eb = make_env(n, "normalize"), make_env(n, "normalize")
    ea.reset()
    eb.reset()
    first = model.rollout(ea, k, seed=9, step=0, entropy=True)
    kept = {key: {a: t.clone() for a, t in first[key].items()} for key in ("obs", "actions", "log_probs", "values", "rewards", "entropy")}
    kept["terminations"] = first["terminations"].clone()
    ptrs = [first[key][a].data_ptr() for key in ("obs", "actions", "log_probs", "values", "rewards", "entropy") for a in AGENTS]
    want = launches_route(eb, model, 2 * k, 9, step=0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second = ea.unwrapped.rollout_policy(model, k, 9, step=k, entropy=True, out=first)
    assert second is first and ptrs == [second[key][a].data_ptr() for key in ("obs", "actions", "log_probs", "values", "rewards", "entropy") for a in AGENTS]
    assert torch.cuda.memory_allocated() == before
    head = lambda d, lo, hi, more: {key: ({a: t[lo:hi + (more if key in ("obs", "values") else 0)] for a, t in v.items()} if isinstance(v, dict) else v[lo:hi])  # noqa: E731
                                    for key, v in d.items()}
    # (row k of the first call's values is a bootstrap value, row k of the launches' record the same number: the value of obs[k])
    same_buffers(kept, head(want, 0, k, 1), "the first call")
    same_buffers(second, head(want, k, 2 * k, 1), "the second call, into the first one's buffers")
    same_envs(ea, eb, "two calls")
    with pytest.raises(ValueError, match="previous result"):
        ea.unwrapped.rollout_policy(model, k + 1, 9, out=first)
    with pytest.raises(ValueError, match="previous result"):
        ea.unwrapped.rollout_policy(model, k, 9, entropy=False, out=first)


def test_a_captured_graph_replayed_twice_against_the_eager_route():
    """the launch is captured with a device step counter and `counter += k` behind it; two replays are 2 k policy steps"""
    n, k, t0 = 64, 2, 40
    model = make_model(64, 18, seed=9)
    ea, eb = make_env(n), make_env(n)
    ea.reset()
    eb.reset()
    raw = ea.unwrapped
    start = raw.read_state()
    counter = torch.tensor([t0], dtype=torch.int64, device=DEV)
    held = raw.rollout_policy(model, k, 5, step=counter)      # (eager once: the library is loaded, the buffers exist)
    torch.cuda.synchronize()
    raw.set_state(start)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = raw.rollout_policy(model, k, 5, step=counter, out=held)
            counter.add_(k)
    assert captured is held
    torch.cuda.synchronize()
    assert np.array_equal(cpu(raw.read_state()), cpu(start))   # (a capture runs nothing)
    counter.fill_(t0)
    want = launches_route(eb, model, 2 * k, 5, step=t0)
    part = lambda d, lo, hi: {key: ({a: t[lo:hi + (1 if key in ("obs", "values") else 0)] for a, t in v.items()} if isinstance(v, dict) else v[lo:hi])  # noqa: E731
                              for key, v in d.items()}
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        same_buffers(held, part(want, replay * k, (replay + 1) * k), f"replay {replay}", entropy=False)
    assert int(counter.item()) == t0 + 2 * k
    assert np.array_equal(cpu(raw.read_state()), cpu(eb.unwrapped.read_state()))


# ---- 2. independent of the older kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack,hidden,activation", (("plain", 64, "tanh"), ("full", 32, "relu"), ("normalize", 128, "tanh")))
def test_the_oracle_and_the_judge(stack, hidden, activation):
    """the C oracle, stepped with the actions the launch reported, reproduces obs[1:], rewards, flags and the final state; the
    float64 judge passes every slab's actions, log-probs, entropies and values on the slab's observations.  The head the judge
    needs is pz_mlp_forward's on the slab's rows -- which the judge holds to its own float64 head first"""
    from pikazoo_amd import net

    n, k, seed, step, first_game = 132, 5, 7, 1, 3
    A = 13 if stack == "full" else 18
    models = {A1: make_model(hidden, A, activation, seed=1), A2: make_model(hidden, A, activation, seed=2)} if hidden < 128 else make_model(hidden, A, activation, seed=1)
    env = make_env(n, stack)
    env.reset()
    got = env.unwrapped.rollout_policy(models, k, seed, step=step, first_game=first_game, entropy=True)
    params, _ = parameter_sets(models)
    heads = [net.forward({a: got["obs"][a][t] for a in AGENTS}, params, activation) for t in range(k + 1)]
    torch.cuda.synchronize()
    ref = oracle_env(n, stack)
    r1, r2 = ref.reset()
    assert np.array_equal(bits(got["obs"][A1][0]), bits(torch.from_numpy(r1))) and np.array_equal(bits(got["obs"][A2][0]), bits(torch.from_numpy(r2)))
    for t in range(k):
        robs, rrew, rterm = ref.step(cpu(got["actions"][A1][t]), cpu(got["actions"][A2][t]))
        for s, a in enumerate(AGENTS):
            assert np.array_equal(bits(got["obs"][a][t + 1]), bits(torch.from_numpy(robs[s]))), (t, a, "observations")
            assert np.array_equal(bits(got["rewards"][a][t]), bits(torch.from_numpy(rrew[s]))), (t, a, "rewards")
        assert np.array_equal(cpu(got["terminations"][t]).astype(np.uint8), rterm), (t, "terminations")
    assert np.array_equal(cpu(env.unwrapped.read_state()), ref.state), "the final state"
    if stack == "full":
        assert np.array_equal(cpu(env.unwrapped.episode_returns), ref.episode_returns) and np.array_equal(cpu(env.unwrapped.episode_lengths), ref.episode_lengths)
    host = [host_params(hidden, A, 1), host_params(hidden, A, 2 if hidden < 128 else 1)]
    for t in range(k):
        us = J.uniforms(seed, first_game, step + t, None, n)
        for s, a in enumerate(AGENTS):
            slab = dict(head=cpu(heads[t][a]), actions=cpu(got["actions"][a][t]), log_probs=cpu(got["log_probs"][a][t]),
                        entropy=cpu(got["entropy"][a][t]), values=cpu(got["values"][a][t]))
            amb, fails = AJ.verdict(slab, cpu(got["obs"][a][t]), host[s], activation, A, us[s], what=f"{stack} slab {t} {a}")
            assert not fails, fails
    for s, a in enumerate(AGENTS):   # the bootstrap row: the value of the last observations
        want, tol = N.judge(cpu(got["obs"][a][k]), host[s], activation)
        assert np.array_equal(bits(got["values"][a][k]), bits(heads[k][a][:, A].contiguous()))
        assert N.worst_share(cpu(heads[k][a]), want, tol)[0] <= 1


# ---- 3. through the C ABI, between sentinels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (4, 3))
def test_the_c_abi_writes_its_rows_and_nothing_else(pad):
    """pitch = n + pad games between slabs (pad 3: slabs that are not 16-byte aligned): every output keeps the sentinel in front
    of its first element, behind its last and in the pad rows of every slab; NaN patterns around the parameters; the rows
    are the ones the binding returns"""
    from pikazoo_amd import rollout

    lib = rollout.load()
    n, k, seed, step = 36, 3, 7, 5
    pitch = n + pad
    model = make_model(64, 18, seed=10)
    ea, eb = make_env(n), make_env(n)
    ea.reset()
    eb.reset()
    want = eb.unwrapped.rollout_policy(model, k, seed, step=step, entropy=True)
    raw = ea.unwrapped
    _keep, ptrs = device_params(host_params(64, 18, 10), offset=1)

    def buffer(slabs, width, dtype):
        return torch.full((FRONT + slabs * pitch * width + TAIL,), SENT & 0xFF if dtype == torch.uint8 else SENT, dtype=dtype, device=DEV)

    obs = [buffer(k + 1, 35, torch.int32) for _ in AGENTS]
    act = [buffer(k, 1, torch.int64) for _ in AGENTS]
    logp, ent, rew = ([buffer(k, 1, torch.int32) for _ in AGENTS] for _ in range(3))
    val = [buffer(k + 1, 1, torch.int32) for _ in AGENTS]
    term = buffer(k, 1, torch.uint8)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)   # episodes_done: the C ABI counts the games that end; the binding passes NULL
    at = lambda ts: [t.data_ptr() + FRONT * t.element_size() for t in ts]  # noqa: E731
    err = lib.pz_rollout_policy(raw._state_ptr, n, raw._stride, raw._cfg_ref, k, 64, 19, 0, *ptrs, *[None] * 6, seed, 0, step, None, 1, pitch,
                                *at(obs), *at(act), *at(logp), *at(val), *at(ent), *at(rew), *at([term]), None, counter.data_ptr(), stream())
    assert err == 0
    torch.cuda.synchronize()

    def rows(t, slabs, width):
        flat = cpu(t)
        sent = SENT & 0xFF if flat.dtype == np.uint8 else SENT
        body = flat[FRONT:FRONT + slabs * pitch * width].reshape(slabs, pitch, width)
        assert (flat[:FRONT] == sent).all() and (flat[FRONT + slabs * pitch * width:] == sent).all(), "written outside the tensor"
        assert (body[:, n:] == sent).all(), "a pad row was written"
        return np.ascontiguousarray(body[:, :n]).reshape((slabs, n, width) if width > 1 else (slabs, n))

    for s, a in enumerate(AGENTS):
        assert np.array_equal(rows(obs[s], k + 1, 35), cpu(want["obs"][a]))
        assert np.array_equal(rows(act[s], k, 1), cpu(want["actions"][a]))
        assert np.array_equal(rows(logp[s], k, 1).view(np.uint32), bits(want["log_probs"][a]))
        assert np.array_equal(rows(ent[s], k, 1).view(np.uint32), bits(want["entropy"][a]))
        assert np.array_equal(rows(val[s], k + 1, 1).view(np.uint32), bits(want["values"][a]))
        assert np.array_equal(rows(rew[s], k, 1), cpu(want["rewards"][a]))
    assert np.array_equal(rows(term, k, 1), cpu(want["terminations"]).astype(np.uint8))
    assert np.array_equal(cpu(raw.read_state()), cpu(eb.unwrapped.read_state()))
    assert int(counter.item()) == int(cpu(want["terminations"]).sum()) and raw.episodes_done == 0


# ---- 4. the example -----------------------------------------------------------------------------------------------------------------
def test_the_example_returns_the_same_losses_with_the_fused_rollout():
    sys.path.insert(0, str(REPO / "examples"))
    import ppo_selfplay

    kw = dict(num_envs=64, iters=2, steps=4, log=lambda line: None)
    loop = ppo_selfplay.main(**kw)
    fused = ppo_selfplay.main(fused_rollout=True, **kw)
    assert len(loop) == len(fused) == 2 * 2 * 4 and loop == fused, (loop, fused)
    with pytest.raises(ValueError, match="fused_rollout"):
        ppo_selfplay.main(fused_rollout=True, native_batch=True, **kw)
