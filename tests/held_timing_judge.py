"""The judge tools/time_held_rollout.py checks its timed variants with.  It lives here because the tuning tools never link
the CPU oracle themselves (tests/test_cabi_and_host.py holds tools/ to that): ``HeldOracle`` of tests/frame_skip_judge.py
on the tool's configuration."""
from frame_skip_judge import HeldOracle


def timing_judge(m, frames, computer, action_seed):
    """The judge of the first m games of the tool's runs (winning score 15, seed 0, auto_reset, player 2 the computer or
    not) at `frames` frames per step, reset, and its policy stream t -> (a1, a2)."""
    from oracle import pz_oracle as po

    po.build()
    judge = HeldOracle(po, m, frames, po.make_config(winning_score=15, is_player2_computer=computer, auto_reset=True, seed=0))
    judge.reset()
    return judge, lambda t: po.random_actions(m, 0, action_seed, t, 18)
