"""The oracle against the UNMODIFIED reference on runs of their own: seeds, configurations and planted states that the
fixtures of tests/test_oracle_golden.py do not hold.

The reference's side of every run is stored under tests/golden/live_*.npz (recorded by oracle/ref_capture.py, whose
``write_live_fixtures`` re-runs the capture harness on the same seeds where the reference checkout is present), so
these tests need nothing outside the repository.
"""
import json

import numpy as np
import pytest

from oracle import ref_capture as rc

GOLDEN = rc.GOLDEN
LIVE = rc.LIVE_RUNS


def _load(name):
    return dict(np.load(GOLDEN / f"{name}.npz"))


@pytest.mark.parametrize("name,kw,wr", LIVE)
def test_oracle_tracks_live_reference(oracle, name, kw, wr):
    lanes, steps, seed, aseed, base = 6, 2500, 424242, 31, 99
    d = _load(f"live_{name}")
    meta = json.loads(bytes(d["meta"]).decode())
    assert (meta["lanes"], meta["steps"], meta["seed"], meta["action_seed"], meta["env_id_base"]) == (lanes, steps, seed,
                                                                                                       aseed, base)
    opt = rc.fused_options(wr)
    cfg = oracle.make_config(winning_score=kw.get("winning_score", 15), serve=kw.get("serve", "winner"),
                             is_player1_computer=kw.get("is_player1_computer", False),
                             is_player2_computer=kw.get("is_player2_computer", False), seed=seed,
                             env_id_base=base, **opt)
    env = oracle.OracleEnv(lanes, cfg)
    assert np.array_equal(env.state, d["state_ctor"])
    env.reset()
    assert np.array_equal(env.state, d["state0"])
    float_obs, float_rew = bool(cfg.normalize_obs), env.float_rewards
    for t in range(steps):
        a = d["actions"][t].astype(np.int32)
        obs, rew, term = env.step(a[0], a[1])
        st = d["states"][t].astype(np.int32)
        st[43] = d["rng_counter"][t]
        assert np.array_equal(env.state, st), (name, t)
        exp = d["obs"][t].astype(np.float32) if float_obs else d["obs"][t]
        assert np.array_equal(obs[0], exp[0]) and np.array_equal(obs[1], exp[1]), (name, t)
        assert np.array_equal(term, d["term"][t]), (name, t)
        if float_rew:
            np.testing.assert_allclose(rew[0], d["rew"][t, 0], rtol=0, atol=1e-6)
        else:
            assert np.array_equal(rew[0], d["rew"][t, 0]) and np.array_equal(rew[1], d["rew"][t, 1])
        if cfg.episode_stats_mode:
            done = d["ep_l"][t] >= 0
            if done.any():
                assert np.array_equal(env.episode_lengths[done], d["ep_l"][t][done])
                np.testing.assert_allclose(env.episode_returns[:, done], d["ep_r"][t][:, done], rtol=0, atol=2e-6)
    assert meta["episodes"] == int(d["term"].sum()) and meta["episodes"] > 0


@pytest.mark.parametrize("kw", rc.LIVE_PLANTED)
def test_oracle_tracks_live_reference_from_planted_states(oracle, kw):
    """Planted states of their own on every configuration (tests/test_gpu_packed.py's fixtures hold another draw of
    them): every attribute of players / ball / scores at random over its valid range, plus the fast-ball corners,
    stepped by the reference."""
    stored = _load(f"live_planted_{rc.LIVE_PLANTED.index(kw)}")
    for kind in ("random", "fast"):
        d = {key[len(kind) + 1:]: v for key, v in stored.items() if key.startswith(kind + "_")}
        meta = json.loads(bytes(d["meta"]).decode())
        assert {k: meta["env_kwargs"][k] for k in kw} == kw and meta["frames"] == (10 if kind == "random" else 12)
        env = oracle.OracleEnv(meta["lanes"], oracle.make_config(
            winning_score=kw.get("winning_score", 15), serve=kw.get("serve", "winner"),
            is_player1_computer=kw.get("is_player1_computer", False),
            is_player2_computer=kw.get("is_player2_computer", False), seed=meta["seed"], env_id_base=meta["env_id_base"]))
        env.state[:] = d["planted"]
        for t in range(meta["frames"]):
            a1, a2 = oracle.random_actions(meta["lanes"], meta["env_id_base"], meta["action_seed"], meta["warm"] + t, 18)
            env.step(a1, a2)
            assert np.array_equal(env.state, d["states"][t]), (kw, t)


def test_draw_list_tracks_live_reference_on_planted_states():
    """render() of the reference on random planted states (every pose / mirroring / score digit / hyper ball, balls
    partly or wholly off screen): the oracle's draw list equals the recorded blits (punch effect aside)."""
    from oracle import render_oracle as ro

    d = _load("live_draw_lists")
    count = json.loads(bytes(d["meta"]).decode())["count"]
    assert count == rc.LIVE_DRAW_LISTS == 400 and d["sizes"].shape == (ro.SPRITE_COUNT, 2)
    sizes = [tuple(int(v) for v in wh) for wh in d["sizes"]]
    checked = 0
    for i in range(count):
        lo, hi = int(d["offsets"][i]), int(d["offsets"][i + 1])
        want = [tuple(int(v) for v in row) for row in d["blits"][lo:hi]]
        got = ro.draw_list(d["states"][i], sizes, d["scenery"][i])
        assert got == want, i
        checked += len(got)
    assert checked > 400 * 45
