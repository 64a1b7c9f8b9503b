"""What tests/test_policy_rollout_host.py (no GPU) and tests/test_gpu_policy_rollout.py share: the cases in which games must
end INSIDE a policy-rollout launch, and the k they need.

With ``winning_score=1`` a game ends with its first rally: the serve falls from y = 0 and meets the ground -- or a player
under it -- some twenty frames after a reset.  TERMINATING_K = 32 policy steps are enough for a good part of the games to end
before the last slab, and with ``auto_reset`` to be reset and played on inside the launch; the host test proves that on the C
oracle under uniformly random actions (a proxy for the sampled ones: the net's head starts near uniform), the GPU test asserts
it on the launch's own termination flags.
"""
import numpy as np

TERMINATING_K = 32
ENV_SEED = 11
# (n, auto_reset): the GPU test's cases with winning_score = 1
TERMINATING_CASES = ((64, True), (132, True), (64, False))
PROXY_SEED = 5


def proxy_play(n, auto_reset, k=TERMINATING_K):
    """The oracle under uniformly random actions: (terminated [k, n], frames played by each game behind its first end)"""
    from oracle import pz_oracle as po

    env = po.OracleEnv(n, po.make_config(winning_score=1, auto_reset=auto_reset, seed=ENV_SEED))
    env.reset()
    rng = np.random.default_rng(PROXY_SEED)
    term = np.zeros((k, n), np.uint8)
    moved_after = np.zeros(n, np.int64)
    ended = np.zeros(n, bool)
    for t in range(k):
        before = env.state.copy()
        _, _, flags = env.step(rng.integers(0, 18, n), rng.integers(0, 18, n))
        term[t] = flags
        moved_after += ended & (env.state != before).any(0)
        ended |= flags != 0
    return term, moved_after
