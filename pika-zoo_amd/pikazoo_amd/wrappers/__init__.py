"""Wrappers with the reference's names and constructor signatures (pikazoo/wrappers/__init__.py).

All six classes of the reference are here.  Five of them do not post-process on the host: they switch
on the corresponding fused branch of the HIP step kernel (``ConvertSingleAgent`` is a thin view).
``PixelObservation`` is this package's own: the grey, downsampled screen as the observation (``pz_render_gray``).
``EgocentricObservation`` too: ``player_2``'s rows mirrored, so that it sees the court as ``player_1`` does (``pz_ego_rows``).
"""
from .base import BaseParallelWrapper
from .convert_single_agent import ConvertSingleAgent
from .egocentric_observation import EgocentricObservation
from .normalize_observation import NormalizeObservation
from .pixel_observation import PixelObservation
from .record_episode_statistics import RecordEpisodeStatistics
from .reward_by_ball_position import RewardByBallPosition
from .reward_in_normal_state import RewardInNormalState
from .simplify_action import SimplifyAction

__all__ = ["BaseParallelWrapper", "SimplifyAction", "RewardByBallPosition", "RewardInNormalState",
           "NormalizeObservation", "RecordEpisodeStatistics", "ConvertSingleAgent", "PixelObservation",
           "EgocentricObservation"]
