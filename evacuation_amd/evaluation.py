"""Evaluation of a fixed agent over whole episodes on the device (``evac_policy_evaluate``, csrc/evac_evaluate.h).

The episode records that fall out of the trainer's collection phase carry the exploration noise, a normaliser that keeps moving
and episodes cut at the ``num_steps`` window.  ``PolicyEvaluator`` answers "how good is this leader?" instead: every env runs
whole episodes under the network's MEAN action (or its sampled one) with the observation statistics FROZEN, or under the
reference's scripted sweep baseline (src/agents/baseline_wacuum_cleaner.py) -- from the same start states, reset draws and
pedestrian-noise streams for every agent, so two agents are compared on the same episodes."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional

import torch

from .config import EnvConfig, EnvWrappersConfig
from .vector_env import STATS_FIELDS, STATS_INT_FIELDS, BatchedEvacuationEnv, stats_int_view

_STATE = ("ped", "status", "agent", "clock", "acc")


@dataclasses.dataclass
class EvaluationResult:
    """``episodes``: ``STATS_FIELDS`` -> float32 [n_episodes, E] and ``STATS_INT_FIELDS`` -> int32 [n_episodes, E] (episode k
    of env e); ``steps``: int32 [E], the env-steps each env took; ``n_pedestrians``: the room's N."""

    episodes: Dict[str, torch.Tensor]
    steps: torch.Tensor
    n_pedestrians: int

    @classmethod
    def from_records(cls, records: torch.Tensor, steps: torch.Tensor, n_pedestrians: int) -> "EvaluationResult":
        """``records``: float32 [n_episodes, E, 10] of ``evac_episode_stats_t``."""
        eps = {k: records[..., i] for i, k in enumerate(STATS_FIELDS)}
        ints = stats_int_view(records)
        eps.update({k: ints[..., i] for i, k in enumerate(STATS_INT_FIELDS)})
        return cls(eps, steps, int(n_pedestrians))

    def summary(self) -> Dict[str, float]:
        """Python floats over all episodes of all envs: mean and (population) std of ``episode_reward``, mean
        ``episode_length``, mean share of the pedestrians that escaped, and the share of episodes in which everybody did."""
        r = self.episodes["episode_reward"].double()
        esc = self.episodes["escaped_pedestrians"].double()
        host = torch.stack([r.mean(), r.std(unbiased=False), self.episodes["episode_length"].double().mean(),
                            (esc / self.n_pedestrians).mean(), (esc == self.n_pedestrians).double().mean()]).cpu().tolist()
        keys = ("episode_reward_mean", "episode_reward_std", "episode_length_mean", "escaped_fraction_mean", "all_escaped_share")
        out = dict(zip(keys, host))
        out["episodes"] = int(r.numel())
        return out


class PolicyEvaluator:
    """An evaluation batch of ``num_envs`` envs with a handle of its own, reset ONCE; the state of that reset is kept, and every
    ``evaluate`` restores it first: all evaluations see the same start states, and -- because the Philox counters of the reset
    draws and of the pedestrians' noise come from ``clock`` -- the same reset draws and noise streams."""

    def __init__(self, env_config: EnvConfig, wrap_config: Optional[EnvWrappersConfig] = None, num_envs: int = 1, seed: int = 0,
                 device="cuda:0", options=None):
        self.env = BatchedEvacuationEnv(env_config, wrap_config, num_envs=num_envs, device=device, seed=seed, autoreset=True,
                                        options=options)
        self.env.reset()
        self.snapshot = {k: getattr(self.env, k).clone() for k in _STATE}
        self.num_envs = self.env.num_envs
        self.launches = 0                      # launches of the last evaluate()

    def restore(self) -> None:
        for k in _STATE:
            getattr(self.env, k).copy_(self.snapshot[k])

    def evaluate(self, agent, n_episodes: int = 1, *, deterministic: bool = True, norm_state: Optional[torch.Tensor] = None,
                 obs_clip: float = 1.0, epsilon: float = 1e-8, max_steps_per_launch: int = 4096) -> EvaluationResult:
        """``n_episodes`` whole episodes per env under ``agent`` (a network with RPOLinearNetwork's attribute names, or
        ``"vacuum_cleaner"``).  ``norm_state``: the trainer's statistics ([rows, 3 D + 4] float64, any number of rows: row
        ``e mod rows`` serves env ``e`` -- the trainer's normaliser is per env and the evaluation batch need not have its
        size), applied frozen.  Launches of at most ``max_steps_per_launch`` steps until every env has finished; the one host
        read per launch is ``progress[:, 0].min()``."""
        env, E = self.env, self.num_envs
        norm = None
        if norm_state is not None:
            W = 3 * env.obs_dim + 4
            if norm_state.dim() != 2 or norm_state.shape[1] != W or norm_state.dtype != torch.float64 or norm_state.shape[0] < 1:
                raise ValueError(f"evaluate: norm_state must be float64 [rows, {W}], got {norm_state.dtype} {tuple(norm_state.shape)}")
            rows = torch.arange(E, device=env.device) % norm_state.shape[0]
            norm = (norm_state.to(env.device)[rows].contiguous(), float(obs_clip), float(epsilon))
        self.restore()
        progress = out = None
        self.launches = 0
        # (every step either ends an episode or brings it one step nearer to max_timesteps: the loop below ends by itself;
        # the bound turns a launch that made no progress into an error instead of a hang)
        bound = -(-int(n_episodes) * int(env.env_config.max_timesteps) // int(max_steps_per_launch)) + 1
        while True:
            if self.launches >= bound:
                raise RuntimeError(f"evaluate: {self.launches} launches of {max_steps_per_launch} steps did not finish {n_episodes} episodes")
            progress, out = env.policy_evaluate(agent, n_episodes, max_steps_per_launch, progress, out, deterministic=deterministic,
                                                _norm=norm)
            self.launches += 1
            if int(progress[:, 0].min()) >= int(n_episodes):
                break
        return EvaluationResult.from_records(out, progress[:, 1].clone(), env.n_ped)

    def close(self) -> None:
        self.env.close()
