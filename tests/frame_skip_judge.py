"""The judge of the frame-skip tests (tests/test_frame_skip_host.py, tests/test_gpu_frame_skip.py): the CPU oracle driven
as the loop that DEFINES ``frame_skip = k`` -- per ``step`` k single-frame oracle steps with the same two actions, the
first with the configured ``auto_reset``, the others with ``auto_reset = 0`` (a game that ends inside the repeat stays
frozen at its terminal frame), the rewards summed in frame order: int32 exactly, float32 in numpy float32 starting from
+0.0.  Nothing under oracle/ knows about frame skip; this only toggles the one configuration word between its calls.
"""
import numpy as np


class HeldOracle:
    """``OracleEnv`` stepped k frames per :meth:`step` on held actions.  Counts, per game and launch, where games ended:
    ``ended_inside`` (a frame before the last: the rest of the repeat is frozen) and ``ended_last``.  ``on_frame``
    (optional; set it on the instance) is called behind every single frame as ``on_frame(j, env, frozen)`` -- the frame's
    index in the repeat, the oracle env (its ``rew`` / ``term`` / ``state`` are that frame's) and the games the frame
    found frozen -- and changes nothing here."""

    def __init__(self, po, n, k, cfg, nthreads=8):
        self.po, self.k, self.auto_reset = po, int(k), int(cfg.auto_reset)
        self.env = po.OracleEnv(n, cfg, nthreads=nthreads)
        self.ended_inside = self.ended_last = 0
        self.on_frame = None

    def __getattr__(self, name):  # state, reset, episode_returns, episode_lengths, float_rewards ...
        return getattr(self.env, name)

    def step(self, a1, a2):
        env = self.env
        total = [np.zeros(env.n, r.dtype) for r in env.rew]  # (+0.0 for float32 rewards)
        frozen = (env.state[self.po.E_GAME_ENDED] != 0) & (self.auto_reset == 0)
        try:
            for j in range(self.k):
                env.cfg.auto_reset = self.auto_reset if j == 0 else 0
                obs, rew, term = env.step(a1, a2)
                total = [t + r for t, r in zip(total, rew)]  # numpy keeps float32 + float32 in float32
                assert all(t.dtype == r.dtype for t, r in zip(total, rew))
                ended_now = int(((term != 0) & ~frozen).sum())
                if j == self.k - 1:
                    self.ended_last += ended_now
                else:
                    self.ended_inside += ended_now
                if self.on_frame is not None:
                    self.on_frame(j, env, frozen)
                frozen = term != 0
        finally:
            env.cfg.auto_reset = self.auto_reset
        return obs, total, term
