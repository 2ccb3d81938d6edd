"""Scripted agents of the reference that drive the hot path in its README loop.

``RandomAgent`` mirrors /root/reference/src/agents/random_agent.py:4-9 (``act`` = action_space.sample()).
``WacuumCleaner`` is the reference's scripted sweep baseline (src/agents/baseline_wacuum_cleaner.py), the yardstick for learned
leaders; the device runs the same state machine inside ``evac_policy_evaluate`` (csrc/evac_evaluate.h, ``vacuum_action``)."""
from __future__ import annotations

import numpy as np

SWITCH_DISTANCE_TO_LEADER = 0.2      # src/env/constants.py:35


class BaseAgent:
    def __init__(self, action_space):
        self.action_space = action_space

    def act(self, obs):
        raise NotImplementedError


class RandomAgent(BaseAgent):
    def act(self, obs):
        return self.action_space.sample()


class WacuumCleaner(BaseAgent):
    """The reference's sweep baseline (baseline_wacuum_cleaner.py:7-82): ``WacuumCleaner(env)`` reads ``env.area.width / height /
    step_size`` and ``env.area.exit.position``; ``act(obs)`` reads ``obs["agent_position"]`` (float32 [2]) and returns one of
    the four float32 unit vectors, or ``exit_position - position``.

    A state machine of a phase, a sweep direction and a countdown:

    * ``CLIMB``: up while ``y < T_y``; the first step that finds ``y >= T_y`` goes right and starts the sweep;
    * ``SWEEP``: right while ``x < T_x`` (left while ``x > -T_x``); the step that finds the wall near goes down, flips the
      direction and arms a countdown of 25: each of the next 25 steps goes down as long as ``y > -T_y``, and the first of them
      that finds ``y <= -T_y`` ends the sweep;
    * ``EXIT``: ``exit_position - position`` for ever.

    ``T = extent - SWITCH_DISTANCE_TO_LEADER / 2 + step_size`` is formed in double, as the reference forms it, and compared
    with the float32 position in float32 -- which is how NumPy 2 compares a float32 scalar with a Python float.

    The reference's object is never reset: after its first episode it would head for the exit for ever.  Here an agent is
    FRESH FOR EVERY EPISODE: call ``reset()`` (or make a new object) at every episode start; the device agent of
    ``policy_evaluate("vacuum_cleaner")`` clears its two state words at every autoreset."""

    CLIMB, SWEEP, EXIT = 0, 1, 2
    COUNTDOWN = 25

    def __init__(self, env):
        area = env.area
        self.up = np.array([0., 1.], dtype=np.float32)
        self.right = np.array([1., 0.], dtype=np.float32)
        self.left = np.array([-1., 0.], dtype=np.float32)
        self.down = np.array([0., -1.], dtype=np.float32)
        self.exit_position = area.exit.position
        self.step_size = area.step_size
        # float32 of the double expression: the value NumPy 2 compares a float32 coordinate with
        self.threshold_x = np.float32(area.width - SWITCH_DISTANCE_TO_LEADER / 2 + area.step_size)
        self.threshold_y = np.float32(area.height - SWITCH_DISTANCE_TO_LEADER / 2 + area.step_size)
        self.reset()

    def reset(self) -> None:
        """A fresh agent: climbing, sweeping to the right first, no countdown."""
        self.phase, self.going_left, self.countdown = self.CLIMB, False, 0

    def act(self, obs):
        pos = obs["agent_position"]
        x, y = np.float32(pos[0]), np.float32(pos[1])
        if self.phase == self.CLIMB:
            if y < self.threshold_y:
                return self.up
            self.phase = self.SWEEP
            return self.right
        if self.phase == self.SWEEP:
            if self.countdown > 0:
                self.countdown -= 1
                if y > -self.threshold_y:
                    return self.down
                self.phase = self.EXIT
            elif (x > -self.threshold_x) if self.going_left else (x < self.threshold_x):
                return self.left if self.going_left else self.right
            else:
                self.going_left = not self.going_left
                self.countdown = self.COUNTDOWN
                return self.down
        return self.exit_position - pos
