"""The six ``rollout_policy_kernel<H, ACT>`` (include/pikazoo_rollout.h: ``pz_rollout_policy``) under the runtime configurations
of tests/policy_rollout_configs.py, from planted states.

tests/test_gpu_policy_rollout.py holds the launch to the launches it replaces from ``reset()``, one axis at a time, while the
serve is still falling.  Here every instantiation runs from kernel_configs.plant_states (random valid states, a quarter of the
games one point from the end, an eighth over) over the runtime branches inside its step loop: the serve rules with env ids whose
low word wraps inside the batch, winning scores 1 / 3 / 15, the frozen path without auto_reset, every shaping table and line,
RewardInNormalState inside and outside, both row formats, the statistics modes (and a mode without a pointer), a state stride
and a slab pitch beyond n across workgroups, n = 67 with the dword flush, game ids and steps that cross 2^32 inside the launch,
masked heads and heads whose rows are bad.  One test per configuration (id: the instantiation and the configuration's index),
through the C ABI:
  * every output, the state and the statistics sit between sentinels -- in front, behind, in the pad rows of every slab and
    past lane n -- which must all survive;
  * policy_rollout_configs.compare: the C oracle stepped with the reported actions (rows, rewards, flags, final state,
    statistics, *episodes_done, bit for bit), the float64 wrapper judge under check_config's rule, act_judge.verdict per slab
    and agent on the head pz_mlp_forward gives for the slab's rows, the masked and the bad rows;
  * the promise of bits: k x (pz_mlp_act; pz_step) through the C ABI from the same planted states, for equality;
  * where the binding can repeat the launch, ``raw_env.rollout_policy`` after ``set_state(planted)``, for equality, with
    ``steps_done`` and the env's own single-frame views.
tests/test_policy_rollout_configs_host.py shows on the CPU that every configuration bites and that the comparison rejects
eleven mutants.  One more test runs the launch with observation bases at 4 mod 16.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_configs as kc
import policy_rollout_configs as pc
from test_gpu_net import device_params
from test_gpu_policy import SENT, TAIL, cpu, stream

pytestmark = pytest.mark.gpu

CONFIGS = pc.configs()
A1, A2 = "player_1", "player_2"
AGENTS = (A1, A2)
DEV = "cuda:0"
FRONT = 8       # elements in front of every output (8: an int64 vector stays aligned, a row buffer 16-byte aligned)
PAD = 0xA5      # what the statistics buffer holds around the lanes of the launch
ADT = {"i32": torch.int32, "i64": torch.int64}


def native_config(c, oracle):
    from pikazoo_amd import _native

    cfg = _native.PzConfig.from_buffer_copy(oracle.make_config(**c.oracle_kwargs()))
    cfg.normalize_obs = c.obs_format
    cfg.action_format = _native.ACTION_FORMATS["int32" if c.action_format == "i32" else "int64"]   # (pz_step reads it; the rollout does not)
    return cfg


class Guarded:
    """`slabs` x `pitch` x `width` elements between sentinels: `front` elements in front, TAIL behind, pad rows n .. pitch - 1"""

    def __init__(self, slabs, pitch, n, width, dtype, front=FRONT):
        self.shape, self.n, self.front = (slabs, pitch, width), n, front
        self.sent = SENT & 0xFF if dtype == torch.uint8 else SENT
        self.t = torch.full((front + slabs * pitch * width + TAIL,), self.sent, dtype=dtype, device=DEV)
        self.ptr = self.t.data_ptr() + front * self.t.element_size()

    def body(self):
        slabs, pitch, width = self.shape
        return self.t[self.front:self.front + slabs * pitch * width].view(slabs, pitch, width)

    def rows(self, what):
        slabs, pitch, width = self.shape
        flat = cpu(self.t)
        body = flat[self.front:self.front + slabs * pitch * width].reshape(slabs, pitch, width)
        assert (flat[:self.front] == self.sent).all() and (flat[self.front + slabs * pitch * width:] == self.sent).all(), f"{what}: written outside the tensor"
        assert (body[:, self.n:] == self.sent).all(), f"{what}: a pad row was written"
        return np.ascontiguousarray(body[:, :self.n]).reshape((slabs, self.n, width) if width > 1 else (slabs, self.n))


def device_sets(c):
    """(kept tensors, agent 1's six addresses, agent 2's six or six times None) with NaN around every parameter"""
    sets = c.params()
    keep1, p1 = device_params(sets[0], offset=1)
    keep2, p2 = device_params(sets[1], offset=1) if c.separate else ([], [None] * 6)
    return keep1 + keep2, p1, p2


def launch(c, oracle, obs_front=(FRONT, FRONT)):
    """`c` through the C ABI from its planted states: restate()'s keys (without the head), every sentinel checked"""
    from pikazoo_amd import rollout

    lib = rollout.load()
    n, k, A, stride, pitch = c.n, c.k, c.n_actions, c.stride_games, c.pitch_games
    cfg = native_config(c, oracle)
    planted, _ = c.start_state()
    state = Guarded(44, stride, n, 1, torch.int32)
    state.body()[:, :n, 0] = torch.from_numpy(planted).to(DEV)
    stats = None
    if c.stats_ptr:   # double[2][stride] running returns, then int32[stride] lengths, between PAD bytes; the launch's lanes start at 0
        stats = torch.full((64 + 20 * stride + TAIL,), PAD, dtype=torch.uint8, device=DEV)
        stats[64:64 + 16 * stride].view(2, stride, 8)[:, :n] = 0
        stats[64 + 16 * stride:64 + 20 * stride].view(stride, 4)[:n] = 0
    keep, p1, p2 = device_sets(c)
    obs = [Guarded(k + 1, pitch, n, 35, torch.int32, front) for front in obs_front]
    act = [Guarded(k, pitch, n, 1, ADT[c.action_format]) for _ in AGENTS]
    logp, ent, rew = ([Guarded(k, pitch, n, 1, torch.int32) for _ in AGENTS] for _ in range(3))
    val = [Guarded(k + 1, pitch, n, 1, torch.int32) for _ in AGENTS]
    term = Guarded(k, pitch, n, 1, torch.uint8)
    done = torch.zeros(1, dtype=torch.int64, device=DEV)
    counter = torch.tensor([c.t0], dtype=torch.int64, device=DEV)
    by_value = c.step == "value"
    at = lambda gs: [g.ptr for g in gs]  # noqa: E731
    err = lib.pz_rollout_policy(state.ptr, n, stride, C.byref(cfg), k, c.hidden, A + 1, rollout.ACTIVATIONS[c.activation], *p1, *p2, c.policy_seed,
                                c.first_game, c.t0 if by_value else 0, None if by_value else counter.data_ptr(),
                                rollout.ACTION_FORMATS[ADT[c.action_format]], pitch, *at(obs), *at(act), *at(logp), *at(val),
                                *(at(ent) if c.entropy else (None, None)), *at(rew), term.ptr, stats.data_ptr() + 64 if c.stats_ptr else None,
                                done.data_ptr(), stream())
    assert err == 0, (c.name, err)
    torch.cuda.synchronize()
    assert int(counter.item()) == c.t0   # (the launch reads the counter; the caller moves it)
    f32 = lambda x: x.view(np.float32)  # noqa: E731
    got = dict(obs=[g.rows(f"observations {s}") for s, g in enumerate(obs)],
               actions=[g.rows(f"actions {s}").astype(np.int64) for s, g in enumerate(act)],
               log_probs=[f32(g.rows(f"log-probs {s}")) for s, g in enumerate(logp)],
               values=[f32(g.rows(f"values {s}")) for s, g in enumerate(val)],
               entropy=[f32(g.rows(f"entropy {s}")) for s, g in enumerate(ent)],
               rewards=[g.rows(f"rewards {s}") for s, g in enumerate(rew)], terminated=term.rows("terminated"),
               state=state.rows("state")[:, :], returns=None, lengths=None, episodes_done=int(done.item()))
    if not c.entropy:   # NULL entropy pointers: the buffers were not passed, and the result has none
        assert all((cpu(g.t) == SENT).all() for g in ent)
        got["entropy"] = None
    if c.stats_ptr:
        flat = cpu(stats)
        ret, lengths = flat[64:64 + 16 * stride].reshape(2, stride, 8), flat[64 + 16 * stride:64 + 20 * stride].reshape(stride, 4)
        assert (flat[:64] == PAD).all() and (flat[64 + 20 * stride:] == PAD).all(), "written outside the statistics"
        assert (ret[:, n:] == PAD).all() and (lengths[n:] == PAD).all(), "statistics past lane n"
        got["returns"] = np.ascontiguousarray(ret[:, :n]).view(np.float64).reshape(2, n)
        got["lengths"] = np.ascontiguousarray(lengths[:n]).view(np.int32).reshape(n)
    del keep
    return got


def torch_sets(c):
    """the parameters as net.forward takes them: one sequence (shared weights) or a dict of them"""
    sets = [[torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in ps] for ps in c.params()]
    return {A1: sets[0], A2: sets[1]} if c.separate else sets[0]


def heads_of(c, got):
    """pz_mlp_forward's head of every slab's rows, both agents: [k + 1][2] float32 [n, O]"""
    from pikazoo_amd import net

    params = torch_sets(c)
    rows = [torch.from_numpy(got["obs"][s]).to(DEV) for s in range(2)]
    if c.obs_format == kc.OBS_F32_NORM:
        rows = [r.view(torch.float32) for r in rows]
    out = []
    for t in range(c.k + 1):
        head = net.forward({A1: rows[0][t].contiguous(), A2: rows[1][t].contiguous()}, params, c.activation)
        out.append([cpu(head[A1]), cpu(head[A2])])
    return out


def launches_route(c, oracle):
    """k x (pz_mlp_act; pz_step) through the C ABI from the planted states, then pz_mlp_act's value of the last rows: the
    launches the header defines the rollout by.  restate()'s keys, as far as those launches produce them"""
    from pikazoo_amd import _native, act

    hip, actlib = _native.load(), act.load()
    n, k, A, stride = c.n, c.k, c.n_actions, c.stride_games
    cfg = native_config(c, oracle)
    planted, _ = c.start_state()
    state = torch.full((44, stride), SENT, dtype=torch.int32, device=DEV)
    state[:, :n] = torch.from_numpy(planted).to(DEV)
    stats = torch.zeros(20 * stride, dtype=torch.uint8, device=DEV) if c.stats_ptr else None
    keep, p1, p2 = device_sets(c)
    if not c.separate:
        p2 = p1   # (pz_mlp_act: shared weights are agent 1's pointers again)
    i32 = dict(dtype=torch.int32, device=DEV)
    obs = [torch.empty((n, 35), **i32) for _ in AGENTS]
    acts = [torch.empty(n, dtype=ADT[c.action_format], device=DEV) for _ in AGENTS]
    logp, ent, val, rew = ([torch.empty(n, **i32) for _ in AGENTS] for _ in range(4))
    term = torch.empty(n, dtype=torch.uint8, device=DEV)
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    rec = dict(obs=[[], []], actions=[[], []], log_probs=[[], []], entropy=[[], []], values=[[], []], rewards=[[], []], terminated=[])
    assert hip.pz_observe(state.data_ptr(), n, stride, cfg.normalize_obs, 0, *ptr(obs), stream()) == 0
    obs_format = act.OBS_FORMATS[torch.float32 if c.obs_format == kc.OBS_F32_NORM else torch.int32]

    def policy(t):
        err = actlib.pz_mlp_act(*ptr(obs), obs_format, n, 35, 35, c.hidden, A + 1, act.ACTIVATIONS[c.activation], *p1, *p2, A, c.policy_seed,
                                c.first_game, c.t0 + t, None, act.ACTION_FORMATS[ADT[c.action_format]], *ptr(acts), *ptr(logp), *ptr(ent), *ptr(val),
                                None, None, 0, stream())
        assert err == 0, (c.name, "pz_mlp_act", err)

    for t in range(k):
        policy(t)
        for s in range(2):
            rec["obs"][s].append(cpu(obs[s]))
            rec["actions"][s].append(cpu(acts[s]).astype(np.int64))
            for key, ts in (("log_probs", logp), ("entropy", ent), ("values", val)):
                rec[key][s].append(cpu(ts[s]).view(np.float32))
        err = hip.pz_step(state.data_ptr(), n, stride, C.byref(cfg), *ptr(acts), *ptr(obs), *ptr(rew), term.data_ptr(),
                          stats.data_ptr() if c.stats_ptr else None, None, stream())
        assert err == 0, (c.name, "pz_step", err)
        for s in range(2):
            rec["rewards"][s].append(cpu(rew[s]))
        rec["terminated"].append(cpu(term))
    policy(k)   # (the draw is not kept: the value of the last rows)
    for s in range(2):
        rec["obs"][s].append(cpu(obs[s]))
        rec["values"][s].append(cpu(val[s]).view(np.float32))
    torch.cuda.synchronize()
    want = {key: [np.stack(v[0]), np.stack(v[1])] for key, v in rec.items() if key != "terminated"}
    want["terminated"] = np.stack(rec["terminated"])
    want["state"] = cpu(state[:, :n])
    assert bool((state[:, n:] == SENT).all())
    if c.stats_ptr:
        flat = cpu(stats)
        want["returns"] = np.ascontiguousarray(flat[:16 * stride].reshape(2, stride, 8)[:, :n]).view(np.float64).reshape(2, n)
        want["lengths"] = np.ascontiguousarray(flat[16 * stride:].reshape(stride, 4)[:n]).view(np.int32).reshape(n)
    del keep
    return want


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else (x.view(np.uint64) if x.dtype == np.float64 else x)


def same_outputs(c, got, want, what):
    keys = ["obs", "actions", "log_probs", "values", "rewards"] + (["entropy"] if c.entropy else [])
    for key in keys:
        for s in range(2):
            g, w = bits(got[key][s]), bits(want[key][s])
            assert g.shape == w.shape and np.array_equal(g, w), (c.name, what, key, s, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))
    assert np.array_equal(got["terminated"], want["terminated"]), (c.name, what, "terminated")
    assert np.array_equal(got["state"], want["state"]), (c.name, what, "the final state")
    if c.stats_ptr:
        assert np.array_equal(bits(got["returns"]), bits(want["returns"])) and np.array_equal(got["lengths"], want["lengths"]), (c.name, what, "statistics")


def binding_route(c, oracle):
    """raw_env.rollout_policy on an env of `c`'s wrapper stack whose state was set to the planted one: (restate()'s keys, the env)"""
    import pikazoo_amd.wrappers as W
    from pikazoo_amd import pikazoo_v0

    env = pikazoo_v0.env(num_envs=c.n, device=DEV, seed=c.seed, env_id_base=c.env_id_base, winning_score=c.winning_score, serve=c.serve,
                         auto_reset=bool(c.auto_reset))
    for name, kw in pc.wrapper_stack(c):
        env = getattr(W, name)(env, **kw)
    raw = env.unwrapped
    assert not raw._unfused, (c.name, raw._unfused)
    mine = native_config(c, oracle)
    fields = ["winning_score", "serve_mode", "simplify_action", "ballpos_reward", "auto_reset", "normal_state_mode", "normalize_obs",
              "episode_stats_mode", "seed", "env_id_base"] + (["x_line", "y_line"] if c.shaped else []) + (["normal_state_reward"] if c.normal_state_mode else [])
    for f in fields:
        assert getattr(raw._cfg, f) == getattr(mine, f), (c.name, f, getattr(raw._cfg, f), getattr(mine, f))
    if c.shaped:
        assert list(raw._cfg.additional_reward) == list(mine.additional_reward)
    env.reset()
    planted, _ = c.start_state()
    raw.set_state(torch.from_numpy(planted).to(DEV))
    step = c.t0 if c.step == "value" else torch.tensor([c.t0], dtype=torch.int64, device=DEV)
    out = raw.rollout_policy(torch_sets(c), c.k, c.policy_seed, step=step, first_game=c.first_game, activation=c.activation,
                             action_dtype=ADT[c.action_format], entropy=bool(c.entropy))
    torch.cuda.synchronize()
    assert ("entropy" in out) == bool(c.entropy)
    i32 = lambda t: cpu(t.view(torch.int32) if t.dtype == torch.float32 else t)  # noqa: E731
    got = dict(obs=[i32(out["obs"][a]) for a in AGENTS], actions=[cpu(out["actions"][a]).astype(np.int64) for a in AGENTS],
               log_probs=[cpu(out["log_probs"][a]) for a in AGENTS], values=[cpu(out["values"][a]) for a in AGENTS],
               entropy=[cpu(out["entropy"][a]) for a in AGENTS] if c.entropy else None, rewards=[i32(out["rewards"][a]) for a in AGENTS],
               terminated=cpu(out["terminations"]).astype(np.uint8), state=cpu(raw.read_state()))
    if c.stats_ptr:
        got["returns"], got["lengths"] = cpu(raw.episode_returns), cpu(raw.episode_lengths)
    return got, raw


@pytest.mark.parametrize("c", CONFIGS, ids=[c.name for c in CONFIGS])
def test_policy_rollout_config(c, oracle):
    got = launch(c, oracle)
    got["head"] = heads_of(c, got)
    fails, ambiguous = pc.compare(c, got)
    worst = max(max(row) for row in ambiguous) if ambiguous else 0
    term = got["terminated"] != 0
    print(f"{c.name}: {int(term.any(0).sum())} games raise the flag, episodes_done {got['episodes_done']}, worst ambiguity {worst} of a cap of "
          f"{pc.AJ.CAP(c.n)}")
    assert not fails, (c.name, fails[:4])
    assert worst <= pc.AJ.CAP(c.n), (c.name, "the launch's own trajectory leaves the judge's cap", ambiguous)
    if c.k > 1:
        assert got["episodes_done"] > 0 or term.any(), "no game ended inside the launch"
    # the promise of bits: the launches the header defines the rollout by
    same_outputs(c, got, launches_route(c, oracle), "k x (pz_mlp_act; pz_step)")
    if c.binding:
        bound, raw = binding_route(c, oracle)
        same_outputs(c, bound, got, "raw_env.rollout_policy")
        assert raw.steps_done == c.k
        # the env-owned single-frame views follow the last slab
        for s, x in enumerate(raw._pack_obs().values()):
            assert np.array_equal(cpu(x.view(torch.int32) if x.dtype == torch.float32 else x), got["obs"][s][c.k]), (c.name, "the env's own rows")
        for s, x in enumerate(raw._rewards()):
            assert np.array_equal(cpu(x.view(torch.int32) if x.dtype == torch.float32 else x), got["rewards"][s][c.k - 1]), (c.name, "the env's own rewards")
        assert np.array_equal(cpu(raw._term).astype(np.uint8), got["terminated"][c.k - 1]), (c.name, "the env's own flags")


def test_observation_bases_at_4_mod_16(oracle):
    """The header asks 4-byte alignment of obs_*; with pitch % 4 == 0 the kernel flushes the rows in 16-byte stores.  n = 68,
    pitch = 68, k = 2, agent 1's rows 4 bytes and agent 2's 20 bytes behind a 16-byte boundary: the rows of the aligned run"""
    c = pc.misaligned_case()
    assert (c.n, c.k, c.pitch_games) == (68, 2, 68)
    aligned = launch(c, oracle)
    shifted = launch(c, oracle, obs_front=(1, 5))
    for g in aligned, shifted:
        g["head"] = heads_of(c, g)
        fails, _ = pc.compare(c, g)
        assert not fails, fails[:4]
    same_outputs(c, shifted, aligned, "bases at 4 mod 16 against the aligned run")
    assert shifted["episodes_done"] == aligned["episodes_done"]
