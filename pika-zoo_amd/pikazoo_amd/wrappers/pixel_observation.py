"""PixelObservation: the screen instead of the 35 numbers (no counterpart in the reference's wrappers; the usual route
there is ``supersuit``'s ``color_reduction`` and ``resize`` around ``render()``).

``reset`` and ``step`` return, for both agents, the same ``uint8[N, 304 // scale, 432 // scale]`` tensor: one screen, the
grey, box-filtered frame of ``raw_env.render_observations`` (``pz_render_gray``, one launch behind the step, the RGB frame
never stored).  The buffer is allocated once and overwritten by every call -- copy what has to outlive the next step
(``render_observations(out=stack[:, j])`` on the unwrapped env writes a frame stack without copies).  Rewards,
terminations, truncations and infos pass through.  Outermost wrapper: what the wrapped env returns as observations is
dropped.  With ``frame_skip`` the frame shows the state after the held frames.  ``step_many`` / ``rollout_*`` are not
wrapped: they stay reachable through ``unwrapped`` and return vector observations.  On an int32-state env a step
synchronises no more than the wrapped env's does (it can be captured into a graph).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import render as _render
from ..spaces import Box
from .base import BaseParallelWrapper


class PixelObservation(BaseParallelWrapper):
    def __init__(self, env, scale: int = 4):
        super().__init__(env)
        raw = env.unwrapped
        self.scale = _render.gray_scale(scale)
        self.shape = (_render.HEIGHT // self.scale, _render.WIDTH // self.scale)
        self._frames = torch.zeros((raw.num_envs, *self.shape), dtype=torch.uint8, device=raw.device)
        self._draw()  # refuses here what render_observations refuses; loads the sprites and the grey background

    def _draw(self):
        raw = self.env.unwrapped
        frame = raw.render_observations(self.scale, out=self._frames)  # (scalar_api: game 0's frame as a numpy array)
        return {a: frame for a in raw.possible_agents}

    def reset(self, seed=None, options=None, **kw):
        _, infos = self.env.reset(seed=seed, options=options, **kw)
        return self._draw(), infos

    def step(self, actions):
        out = self.env.step(actions)
        return (self._draw(),) + tuple(out[1:])

    def observation_space(self, agent):
        return Box(0, 255, self.shape, np.uint8)
