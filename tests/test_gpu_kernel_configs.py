"""Every step-kernel instantiation under the runtime configurations of tests/kernel_configs.py, against the oracle.

tests/test_gpu_kernel_matrix.py launches each instantiation under one fixed recipe; the runtime branches inside a
kernel -- the winning score and the serve rule, the frozen path without auto-reset, the reward shaping lines and tables,
RewardInNormalState inside and outside RewardByBallPosition, the observation formats, the statistics modes (and a mode
without a pointer: the PLAIN form of a k-frame kernel), the action element types, env ids above 2^32 and a t0 crossing
2^32, a stride of n -- are exercised here, at both batch sizes of the switch.  One test per configuration (id: the
instantiation and the configuration's index), through test_gpu_kernel_matrix.check_config: the same checks as a matrix
row, the float64 judge of the float outputs, and for every shaped configuration a post-step ball exactly on a line.
"""
import pytest

from kernel_configs import configs
from test_gpu_kernel_matrix import buffers, check_config  # noqa: F401 (buffers: the module's fixture)

pytestmark = pytest.mark.gpu

CONFIGS = configs()


@pytest.mark.parametrize("c", CONFIGS, ids=[c.name for c in CONFIGS])
def test_kernel_config_vs_oracle(c, oracle, buffers):  # noqa: F811
    check_config(c, oracle, buffers)
