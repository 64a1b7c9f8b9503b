"""Every instantiation of the two frame-skip kernel families -- ``hold_kernel`` (``pz_step_held``) and
``held_traj_kernel`` (``pz_step_many_held`` / ``pz_rollout_random_held``) -- under the runtime configurations of
tests/held_configs.py, against the judge (tests/frame_skip_judge.py: the CPU oracle driven as the loop that defines frame
skip).

tests/test_gpu_frame_skip.py and tests/test_gpu_held_rollout.py walk the structure of these launches from reset plus
random play, on the winner's serve and the default shaping lines.  Here every instantiation runs from planted random
valid states (a quarter of the games one point from the end, an eighth over) over the runtime branches inside it: the
serve rules (the random serve draws from the env's stream at a round's end and at the in-launch reset, next to the
deferred boldness draw), winning scores 1 / 3 / 15, the frozen path without auto_reset, every shaping table and line
with its frame sum, RewardInNormalState inside and outside, row formats 0 - 6, the statistics modes (and a mode without
a pointer), env ids whose low word wraps inside the launch and a policy index crossing 2^32, a stride of n, the four
action element types of ``pz_step_held``, holds of 2 - 8 frames and 1 - 70 policy steps.  One test per configuration (id:
the instantiation and the configuration's index) through test_gpu_held_rollout.check_case: the dispatched kernel by
name, nothing written past lane n / slab k / through a NULL statistics pointer, and rows, rewards, ``terminated``,
actions, final state, statistics and episodes_done bit for bit against the judge -- every lane below the size switch,
three slices of 512 at it -- plus the float64 bound on the float32 reward sums.  tests/test_held_configs_host.py shows on
the judge alone that every configuration bites; what it showed is asserted again here on the launch's own judge.
"""
import pytest

from held_configs import configs
from test_gpu_held_rollout import check_case

pytestmark = pytest.mark.gpu

CONFIGS = configs()


@pytest.mark.parametrize("c", CONFIGS, ids=[c.name for c in CONFIGS])
def test_held_config_vs_the_judge(c, oracle):
    inside, last, revived, _ = check_case(c, oracle)
    assert inside + last > 0, "no game terminated inside the launch"
    assert inside > 0, "no game ended inside a repeat"
    if c.auto_reset and c.k >= 5:
        assert revived > 0, "no game was terminated in one slab and running in the next"
