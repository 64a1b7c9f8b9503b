"""The judge of a batch whose games differ in who plays (pz_step_mixed), and the cases of its tests.

Games share nothing and a game's draws depend on its global id alone, so a mixed batch is, lane by lane, the reference env
constructed with that lane's two flags.  `MixedJudge` therefore runs the unchanged CPU oracle four times -- role code 0
(nobody), 1 (player 1), 2 (player 2), 3 (both) is the computer -- on the same seed, ids and actions, every run on all the
lanes, and takes each lane's state, outputs and statistics from the run that has its roles.  A role change copies the
lane's oracle state (and statistics) from the run it leaves into the run it joins, at the switch frame.

`cases()` are the GPU cases of tests/test_gpu_mixed.py; tests/test_mixed_host.py checks on the judge alone that they
bite (every lane's final state differs from its final state under each other role code).
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

N, STRIDE = 200, 256          # three full waves and a tail of 8 lanes; the columns' pitch is not the batch size
FRAMES = 320                  # chosen on the CPU: test_mixed_host.test_every_lane_depends_on_its_role_code
WINNING_SCORE = 2
SEED, ACTION_SEED, ENV_ID_BASE = 20261018, 0xAC7, 1 << 20
CODES = (0, 1, 2, 3)
EX_WORD = 36                  # ball.expected_landing_point_x
TABLE = (0.0, -0.01, 0.25, 0.01, -0.5, 0.01, 0.0, -0.01)
NORMAL_STATE_REWARD = -0.25


def role_codes(n=N, seed=SEED):
    """uint8[n]: wave 0 all 0, wave 1 all 3, wave 2 cycling 0-3 by lane, the tail random"""
    codes = np.zeros(n, np.uint8)
    codes[64:128] = 3
    codes[128:192] = np.arange(64) % 4
    codes[192:] = np.random.default_rng(seed).integers(0, 4, max(n - 192, 0))
    return codes[:n]


def rows_as(ref_obs, fmt):
    """One frame's rows as the buffer of observation format `fmt` (enum pz_obs_format) holds them, bit for bit: the
    oracle's rows -- int32, or the float32 NormalizeObservation quotient of the normalized formats -- as values / bit
    patterns, 2-byte rows widened to int32."""
    import torch

    if fmt == 1:
        return ref_obs.view(np.int32)
    if fmt in (0, 2):
        return ref_obs
    dt = torch.float16 if fmt in (3, 5) else torch.bfloat16
    rows = torch.from_numpy(np.ascontiguousarray(ref_obs)).to(torch.float32).to(dt)
    return rows.view(torch.int16).numpy().astype(np.int32)


class MixedJudge:
    def __init__(self, oracle, n, codes, start_state=None, **config):
        """config: oracle.make_config's kwargs but the two role flags"""
        self.oracle, self.n = oracle, n
        self.codes = np.array(codes, np.uint8)
        self.runs = [oracle.OracleEnv(n, oracle.make_config(is_player1_computer=bool(c & 1), is_player2_computer=bool(c & 2),
                                                            **config)) for c in CODES]
        if start_state is not None:
            for r in self.runs:
                r.state[:] = start_state

    def _pick(self, get):
        parts = [np.asarray(get(r)) for r in self.runs]
        out = parts[0].copy()
        for c in CODES[1:]:
            lanes = self.codes == c
            out[..., lanes] = parts[c][..., lanes]
        return out

    def reset(self, mask=None):
        for r in self.runs:
            r.reset(mask)

    def step(self, a1, a2):
        for r in self.runs:
            r.step(a1, a2)

    def set_codes(self, codes):
        """A role change between two frames: every lane continues from its own state under its new roles."""
        codes = np.array(codes, np.uint8)
        state, stats = self.state, self.stats
        for c in CODES:
            lanes = (codes == c) & (self.codes != c)
            self.runs[c].state[:, lanes] = state[:, lanes]
            if stats is not None:
                ret, length = self.runs[c].episode_returns, self.runs[c].episode_lengths
                ret[:, lanes] = stats[0][:, lanes]
                length[lanes] = stats[1][lanes]
        self.codes = codes

    # what the mixed batch holds: lane l from run codes[l]
    @property
    def state(self):
        return self._pick(lambda r: r.state)

    def obs(self, player):
        return self._pick(lambda r: r.obs[player].T).T

    def rew(self, player):
        return self._pick(lambda r: r.rew[player])

    @property
    def term(self):
        return self._pick(lambda r: r.term)

    @property
    def stats(self):
        """(float64[2, n] episode returns, int32[n] episode lengths), or None without statistics"""
        if self.runs[0].stats is None:
            return None
        return self._pick(lambda r: r.episode_returns), self._pick(lambda r: r.episode_lengths)

    def state_under(self, code):
        """the whole batch as role code `code` plays it (the non-vacuity checks)"""
        return self.runs[code].state


@dataclass(frozen=True)
class Case:
    name: str
    packed: bool = False
    tables: str = "both"          # both / power_hit / none
    simplify_action: bool = False
    shaped: bool = False          # RewardInNormalState inside RewardByBallPosition, statistics on the wrapped rewards
    obs_format: int = 0           # enum pz_obs_format
    action_format: str = "i32"
    auto_reset: bool = True
    planted: bool = False

    def oracle_kwargs(self):
        kw = dict(winning_score=WINNING_SCORE, seed=SEED, env_id_base=ENV_ID_BASE, auto_reset=self.auto_reset,
                  simplify_action=self.simplify_action)
        if self.shaped:
            kw.update(additional_reward=TABLE, normal_state_reward=NORMAL_STATE_REWARD, episode_stats=2)
        kw["normalize_obs"] = self.obs_format in (1, 5, 6)
        return kw

    def start_state(self):
        """None: the constructor's state; planted: the recipe of tests/kernel_configs.py -- random valid states, balls
        outside the flight tables' domain among them, an eighth of the games over"""
        if not self.planted:
            return None
        from kernel_configs import plant_states

        return plant_states(SimpleNamespace(seed=SEED, winning_score=WINNING_SCORE, matrix=False, n=N))[0]


def cases():
    plain = [Case(f"{'packed' if packed else 'int32'}-{tables}", packed=packed, tables=tables)
             for packed in (False, True) for tables in ("both", "power_hit", "none")]
    return plain + [
        Case("wrapper-stack", simplify_action=True, shaped=True, obs_format=1),
        Case("wrapper-stack-packed-none", packed=True, tables="none", simplify_action=True, shaped=True, obs_format=1),
        Case("bf16-rows", obs_format=4),
        Case("int64-actions", action_format="i64", tables="power_hit"),
        Case("no-auto-reset", auto_reset=False),
        Case("planted", planted=True),
        Case("planted-packed-none", planted=True, packed=True, tables="none"),
    ]


def judge_for(oracle, case, codes=None):
    return MixedJudge(oracle, N, role_codes() if codes is None else codes, start_state=case.start_state(),
                      **case.oracle_kwargs())


def actions(oracle, t, n_actions):
    return oracle.random_actions(N, ENV_ID_BASE, ACTION_SEED, t, n_actions)

