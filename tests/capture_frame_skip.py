#!/usr/bin/env python3
"""tests/golden/frame_skip_k4.npz: the UNMODIFIED reference stepped with every action held for 4 frames (build machine only).

    python tests/capture_frame_skip.py

What a user of the reference writes for an action repeat, around ``pikazoo_v0.env()`` with the Philox stream of
oracle/ref_capture.py injected: per policy step up to k calls of ``env.step`` on the same two actions, the rewards
summed, the repeat CUT at the game's terminal frame (the reference empties ``agents`` there), the game ``reset()`` right
before its next repeat.  Stored: inputs and outputs only (actions, the 44 state words, observations, summed rewards,
terminations after every policy step); nothing of the reference's text.  tests/test_frame_skip_host.py holds the
oracle-driven judge to it, tests/test_gpu_frame_skip.py the env.
"""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle import pz_oracle as po  # noqa: E402
from oracle import ref_capture as rc  # noqa: E402

K, LANES, STEPS, SEED, ACTION_SEED, ENV_ID_BASE = 4, 6, 400, 777, 41, 500
ENV_KWARGS = dict(winning_score=2, is_player2_computer=True)


def capture():
    assert rc.reference_available(), "the reference checkout is not on this machine"
    envs = [rc.make_reference_env(SEED, ENV_ID_BASE + i, None, **ENV_KWARGS) for i in range(LANES)]
    for env, raw, shim in envs:
        env.reset()
    state0 = np.stack([rc.extract_state(raw, shim) for _, raw, shim in envs], axis=1)
    actions = np.zeros((STEPS, 2, LANES), np.uint8)
    states = np.zeros((STEPS, po.W, LANES), np.int64)
    obs_all = np.zeros((STEPS, 2, LANES, po.OBS), np.int64)
    rew = np.zeros((STEPS, 2, LANES), np.int64)
    term = np.zeros((STEPS, LANES), np.uint8)
    ended_inside = ended_last = 0
    for t in range(STEPS):
        a1, a2 = po.random_actions(LANES, ENV_ID_BASE, ACTION_SEED, t, 18)
        actions[t, 0], actions[t, 1] = a1, a2
        for i, (env, raw, shim) in enumerate(envs):
            if not raw.agents:  # the game ended in the previous repeat
                env.reset()
            for j in range(K):
                obs, rews, terms, truncs, infos = env.step({"player_1": int(a1[i]), "player_2": int(a2[i])})
                rew[t, 0, i] += rews["player_1"]
                rew[t, 1, i] += rews["player_2"]
                if terms["player_1"]:
                    ended_inside += j < K - 1
                    ended_last += j == K - 1
                    break
            obs_all[t, 0, i], obs_all[t, 1, i] = obs["player_1"], obs["player_2"]
            term[t, i] = int(terms["player_1"])
            states[t, :, i] = rc.extract_state(raw, shim)
    meta = dict(name="frame_skip_k4", frame_skip=K, lanes=LANES, steps=STEPS, seed=SEED, action_seed=ACTION_SEED,
                env_id_base=ENV_ID_BASE, env_kwargs=ENV_KWARGS, ended_inside=int(ended_inside), ended_last=int(ended_last),
                fields=po.FIELD_NAMES)
    assert ended_inside > 0 and ended_last > 0, meta
    out = dict(meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), state0=state0.astype(np.int32),
               actions=actions, states=states.astype(np.int16), rng_counter=states[:, po.E_RNG_COUNTER, :].astype(np.int32),
               obs=obs_all.astype(np.int16), rew=rew.astype(np.int32), term=term)
    assert np.array_equal(out["states"].astype(np.int64)[:, :po.E_RNG_COUNTER], states[:, :po.E_RNG_COUNTER])  # lossless
    assert np.array_equal(out["obs"].astype(np.int64), obs_all)
    return out


if __name__ == "__main__":
    path = REPO / "tests" / "golden" / "frame_skip_k4.npz"
    np.savez_compressed(path, **capture())
    print(path, path.stat().st_size, "bytes")
