"""EgocentricObservation: ``player_2`` sees the court as ``player_1`` does (no counterpart in the reference's wrappers: its
``SimplifyAction`` offers relative directions for the ACTIONS through a table per side, its observation rows stay absolute).

``reset`` and ``step`` return the named agents' rows mirrored about the court's centre line (``ego.mirror``, one launch per
agent behind the step; the definition is include/pikazoo_ego.h's): the row of ``player_2`` is then, bit for bit in the raw
integer formats, the row ``player_1`` is handed in the mirrored game.  Together with the fused ``SimplifyAction`` the interface
is side-symmetric -- one net, either side:

    env = EgocentricObservation(NormalizeObservation(SimplifyAction(env)))

The mirrored rows live in buffers this wrapper owns, as many sets as the env's ``output_ring`` and rotated with it.  They are
never written in place of the env's rows: ``reset(mask=)`` makes the env rewrite its whole buffer from the state, the unmasked
rows unchanged, and a wrapper that had mirrored that buffer in place could not tell which rows still carry its mirror.  The
other agents' rows, rewards, terminations, truncations and infos pass through.

The row format is read from the unwrapped env on every call, so a ``NormalizeObservation`` fused later, above this wrapper,
gives the rows of one fused below it.  (An UN-fused one above it -- int16 rows -- divides by the bounds of this wrapper's
``observation_space``, whose ball x is [0, 412]: its column 26 is ``(432 - x) / 412`` where the other orders give
``(412 - x) / 412``.)

Actions.  Where the wrapped env's ``action_space`` of a named agent is ``Discrete(18)`` -- absolute directions -- the agent's
actions go through the left-right involution ``ego.PI`` into a buffer of this wrapper (``ego.mirror_actions``, one launch)
before the inner ``step``; a value outside [0, 18) passes through, so that the env's range check still sees it.  Where it is
``Discrete(13)`` they pass through untouched: the fused ``SimplifyAction`` already maps them per side.

``observation_space``: in the raw formats the ball's x of a mirrored agent has the bounds [0, 412] (``432 - [20, 432]``), all
other bounds are symmetric; the normalised Box(0, 1) stays as it is.  ``step_many`` / ``rollout_*`` are not wrapped: they stay
reachable through ``unwrapped``, and ``ego.mirror`` takes their ``[k, n, 35]`` slabs.  A step synchronises no more than the
wrapped env's and can be captured into a graph once the buffers exist (after the first ``reset`` and ``step``).
"""
from __future__ import annotations

import torch

from ..spaces import Box
from .base import BaseParallelWrapper
from .pixel_observation import PixelObservation

_NORMALIZED = (1, 5, 6)  # enum pz_obs_format
_COURT_WIDTH = 432


class EgocentricObservation(BaseParallelWrapper):
    def __init__(self, env, agents=("player_2",)):
        super().__init__(env)
        from .. import ego  # (on first use: importing the wrappers imports no learner binding)

        raw = env.unwrapped
        if raw.scalar_api:
            raise ValueError("EgocentricObservation works on the batched API: this env was made with scalar_api=True")
        below = env
        while below is not raw:
            if isinstance(below, PixelObservation):
                raise ValueError("EgocentricObservation mirrors the 35-element rows: there is a PixelObservation below it")
            below = below.env
        agents = (agents,) if isinstance(agents, str) else tuple(agents)
        unknown = [a for a in agents if a not in raw.possible_agents]
        if unknown or not agents:
            raise ValueError(f"agents must name some of {raw.possible_agents}, got {list(agents)}")
        self.mirrored = tuple(a for a in raw.possible_agents if a in agents)
        self._ego = ego
        self._rows = {}     # {(ring slot, agent): the mirrored rows}
        self._actions = {}  # {agent: the mapped actions}
        self._boxes = {}

    def _mirror(self, obs):
        raw = self.env.unwrapped
        slot, out = raw._ring_pos, dict(obs)
        for a in self.mirrored:
            rows = obs[a]
            buf = self._rows.get((slot, a))
            if buf is None or buf.dtype != rows.dtype or buf.shape != rows.shape:
                buf = self._rows[slot, a] = torch.empty(rows.shape, dtype=rows.dtype, device=rows.device)
            half = rows.dtype in (torch.float16, torch.bfloat16)
            out[a] = self._ego.mirror(rows, normalized=(raw._cfg.normalize_obs in _NORMALIZED) if half else None, out=buf)
        return out

    def reset(self, seed=None, options=None, **kw):
        obs, infos = self.env.reset(seed=seed, options=options, **kw)
        return self._mirror(obs), infos

    def step(self, actions):
        mapped = None
        for a in self.mirrored:
            if self.env.action_space(a).n != 18:
                continue  # Discrete(13): SimplifyAction's table of that side is the mirror already
            v = self.env.unwrapped._action_tensor(actions[a])  # KeyError on a missing agent
            buf = self._actions.get(a)
            if buf is None or buf.dtype != v.dtype:
                buf = self._actions[a] = torch.empty_like(v)
            mapped = dict(actions) if mapped is None else mapped
            mapped[a] = self._ego.mirror_actions(v, out=buf)
        out = self.env.step(actions if mapped is None else mapped)
        return (self._mirror(out[0]),) + tuple(out[1:])

    def observation_space(self, agent):
        inner = self.env.observation_space(agent)
        if agent not in self.mirrored or inner.high[26] != _COURT_WIDTH:
            return inner  # (normalised rows: Box(0, 1) as it is)
        key = (agent, str(inner.dtype))
        if key not in self._boxes:
            low, high = inner.low.copy(), inner.high.copy()
            low[26], high[26] = _COURT_WIDTH - inner.high[26], _COURT_WIDTH - inner.low[26]
            self._boxes[key] = Box(low=low, high=high, shape=(35,), dtype=inner.dtype)
        return self._boxes[key]
