#!/usr/bin/env python3
"""Record the reference's scripted sweep baseline (src/agents/baseline_wacuum_cleaner.py) -- build container only.

    python tests/golden/make_golden_agents.py     # rewrites tests/golden/agent_vacuum_cleaner.npz

The reference env comes from ``_reference_loader.load_full()``.  The agent's source file is loaded under a stand-in parent
package that provides ``BaseAgent`` and nothing else: the reference's own ``src/agents/__init__.py`` pulls in the trainer, which
this image cannot import.  The fixture is data only: per step the leader position the agent was shown and the action it returned
(both float32), the episode boundaries, the three settings the agent reads (width, height, step_size) and whether the reference
object had reached its third task when the episode ended.  A FRESH reference object drives every episode (the reference's own
object is never reset and would head for the exit for ever after its first episode)."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _reference_loader as L  # noqa: E402

# (name, seed, EnvConfig kwargs): whole episodes, to termination or truncation
EPISODES = (
    ("n10", 21, dict(number_of_pedestrians=10)),
    ("n60", 22, dict(number_of_pedestrians=60)),
    ("n33_step05", 23, dict(number_of_pedestrians=33, step_size=0.05)),
    ("n20_room07x13_step03", 24, dict(number_of_pedestrians=20, width=0.7, height=1.3, step_size=0.03)),
)


def load_reference_agent(ref):
    """The reference's WacuumCleaner class, its file loaded as ``refagents.baseline_wacuum_cleaner``."""
    import importlib
    sys.modules["env"] = ref                                              # the file says `from env import EvacuationEnv`
    sys.modules["env.constants"] = importlib.import_module("src.env.constants")
    parent = types.ModuleType("refagents")
    parent.__path__ = [os.path.join(L.REFERENCE_ROOT, "src", "agents")]

    class BaseAgent:
        def __init__(self, action_space):
            self.action_space = action_space

    parent.BaseAgent = BaseAgent
    sys.modules["refagents"] = parent
    path = os.path.join(L.REFERENCE_ROOT, "src", "agents", "baseline_wacuum_cleaner.py")
    spec = importlib.util.spec_from_file_location("refagents.baseline_wacuum_cleaner", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.WacuumCleaner


def record_episode(ref, Agent, seed, cfg_kw):
    cfg = ref.EnvConfig(wandb_enabled=False, path_logs=L.log_dir(), giff_freq=10 ** 9, **cfg_kw)
    env = ref.EvacuationEnv(cfg)
    np.random.seed(seed)
    obs, _ = env.reset()
    agent = Agent(env)
    positions, actions = [], []
    while True:
        pos = np.array(obs["agent_position"], copy=True)
        act = agent.act(obs)
        assert pos.dtype == np.float32 and act.dtype == np.float32, (pos.dtype, act.dtype)
        positions.append(pos)
        actions.append(np.array(act, copy=True))
        obs, _, terminated, truncated, _ = env.step(np.array(act, copy=True))     # (the env divides its argument in place)
        if terminated or truncated:
            break
    settings = np.array([env.area.width, env.area.height, env.area.step_size], dtype=np.float64)
    return np.stack(positions), np.stack(actions), settings, bool(agent.task_done[1])


def main():
    ref = L.load_full()
    Agent = load_reference_agent(ref)
    pos, act, start, settings, third, names = [], [], [0], [], [], []
    for name, seed, kw in EPISODES:
        p, a, s, t = record_episode(ref, Agent, seed, kw)
        print(f"{name}: {len(p)} steps, third task reached: {t}")
        pos.append(p)
        act.append(a)
        start.append(start[-1] + len(p))
        settings.append(s)
        third.append(t)
        names.append(name)
    assert any(third), "no recorded episode reaches the third task: pick other seeds"
    out = os.path.join(HERE, "agent_vacuum_cleaner.npz")
    np.savez_compressed(out, positions=np.concatenate(pos), actions=np.concatenate(act), episode_start=np.array(start, dtype=np.int64),
                        settings=np.stack(settings), third_task=np.array(third), names=np.array(names))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
