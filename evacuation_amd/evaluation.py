"""Evaluation of a fixed agent over whole episodes on the device (``evac_policy_evaluate``, csrc/evac_evaluate.h).

The episode records that fall out of the trainer's collection phase carry the exploration noise, a normaliser that keeps moving
and episodes cut at the ``num_steps`` window.  ``PolicyEvaluator`` answers "how good is this leader?" instead: every env runs
whole episodes under the network's MEAN action (or its sampled one) with the observation statistics FROZEN, or under the
reference's scripted sweep baseline (src/agents/baseline_wacuum_cleaner.py) -- from the same start states, reset draws and
pedestrian-noise streams for every agent, so two agents are compared on the same episodes.  ``PopulationEvaluator`` does the
same for the S learners of a ``PolicyPopulation``, a ``DeepSetsPopulation`` or a ``TransformerPopulation`` in one set of launches
(``evac_policy_evaluate_population``, ``evac_policy_evaluate_population_deepsets``,
``evac_policy_evaluate_population_transformer``)."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import torch

from .config import EnvConfig, EnvWrappersConfig
from .vector_env import STATS_FIELDS, STATS_INT_FIELDS, BatchedEvacuationEnv, stats_int_view

_STATE = ("ped", "status", "agent", "clock", "acc")
_SUMMARY_KEYS = ("episode_reward_mean", "episode_reward_std", "episode_length_mean", "escaped_fraction_mean", "all_escaped_share")


@dataclasses.dataclass
class EvaluationResult:
    """``episodes``: ``STATS_FIELDS`` -> float32 [n_episodes, E] and ``STATS_INT_FIELDS`` -> int32 [n_episodes, E] (episode k
    of env e); ``steps``: int32 [E], the env-steps each env took; ``n_pedestrians``: the room's N; ``capture``: ``None``, or
    the recorded frames of envs ``0..K-1`` (``policy_evaluate``'s ``capture``: ``{"frames": [F, K, N+1, 3], "starts":
    [n_episodes, K, N+1, 3]}``), which ``episode_memory`` cuts into episodes."""

    episodes: Dict[str, torch.Tensor]
    steps: torch.Tensor
    n_pedestrians: int
    capture: Optional[Dict[str, torch.Tensor]] = None

    @classmethod
    def from_records(cls, records: torch.Tensor, steps: torch.Tensor, n_pedestrians: int) -> "EvaluationResult":
        """``records``: float32 [n_episodes, E, 10] of ``evac_episode_stats_t``."""
        eps = {k: records[..., i] for i, k in enumerate(STATS_FIELDS)}
        ints = stats_int_view(records)
        eps.update({k: ints[..., i] for i, k in enumerate(STATS_INT_FIELDS)})
        return cls(eps, steps, int(n_pedestrians))

    def episode_memory(self, env: int, episode: int, status_cls=None):
        """``(pedestrians.memory, agent.memory)`` of episode ``episode`` of recorded env ``env`` in the reference's format
        (``trajectory.episode_to_memory``; feed them to ``trajectory.feed_reference_env``): with ``L`` the episode's recorded
        length, ``L + 1`` pedestrian frames -- the start state first -- and ``L`` leader positions.  ``IndexError``: no
        capture was made, ``env >= K``, or an episode the env has not finished; ``ValueError``: frames beyond ``max_frames``."""
        from .trajectory import episode_to_memory
        if self.capture is None:
            raise IndexError("episode_memory: this evaluation recorded no frames (evaluate(..., capture_envs=K))")
        frames, starts = self.capture["frames"], self.capture["starts"]
        if not 0 <= int(env) < int(frames.shape[1]):
            raise IndexError(f"episode_memory: env {int(env)} was not recorded (envs 0..{int(frames.shape[1]) - 1} were)")
        return episode_to_memory(frames, starts, self.episodes["episode_length"][:, int(env)], env, episode, status_cls)

    def summary(self) -> Dict[str, float]:
        """Python floats over all episodes of all envs: mean and (population) std of ``episode_reward``, mean
        ``episode_length``, mean share of the pedestrians that escaped, and the share of episodes in which everybody did."""
        out = dict(zip(_SUMMARY_KEYS, self._summary_scalars().cpu().tolist()))
        out["episodes"] = int(self.episodes["episode_reward"].numel())
        return out

    def _summary_scalars(self) -> torch.Tensor:
        """The five reductions of ``summary()`` as one float64 [5] tensor on the episodes' device (no host transfer)."""
        r = self.episodes["episode_reward"].double()
        esc = self.episodes["escaped_pedestrians"].double()
        return torch.stack([r.mean(), r.std(unbiased=False), self.episodes["episode_length"].double().mean(),
                            (esc / self.n_pedestrians).mean(), (esc == self.n_pedestrians).double().mean()])

    @staticmethod
    def summaries(results: Sequence["EvaluationResult"]) -> List[Dict[str, float]]:
        """``[r.summary() for r in results]`` with ONE host transfer for all of them (the S learners of
        ``PopulationEvaluator.evaluate``): every result's reductions are ``summary()``'s own, so the values are its bits, and
        they are gathered on the device and read once -- the S synchronising reads are what the per-result loop costs."""
        results = list(results)
        if not results:
            return []
        host = torch.stack([res._summary_scalars() for res in results]).cpu().tolist()
        out = []
        for res, row in zip(results, host):
            d = dict(zip(_SUMMARY_KEYS, row))
            d["episodes"] = int(res.episodes["episode_reward"].numel())
            out.append(d)
        return out


class _Evaluator:
    """What the two evaluators share: ``env`` (reset once), ``snapshot`` (the state every evaluation starts from) and the launch
    loop."""

    launches = 0                               # launches of the last evaluate()

    def restore(self) -> None:
        for k in _STATE:
            getattr(self.env, k).copy_(self.snapshot[k])

    def _run(self, n_episodes: int, max_steps_per_launch: int, launch):
        """``restore()``, then ``progress, out = launch(progress, out)`` until every env has finished ``n_episodes`` episodes;
        returns the two.  The one host read per launch is ``progress[:, 0].min()``."""
        self.restore()
        progress = out = None
        self.launches = 0
        # (every step either ends an episode or brings it one step nearer to max_timesteps: the loop below ends by itself;
        # the bound turns a launch that made no progress into an error instead of a hang)
        bound = -(-int(n_episodes) * int(self.env.env_config.max_timesteps) // int(max_steps_per_launch)) + 1
        while True:
            if self.launches >= bound:
                raise RuntimeError(f"evaluate: {self.launches} launches of {max_steps_per_launch} steps did not finish {n_episodes} episodes")
            progress, out = launch(progress, out)
            self.launches += 1
            if int(progress[:, 0].min()) >= int(n_episodes):
                return progress, out

    def close(self) -> None:
        self.env.close()


class PolicyEvaluator(_Evaluator):
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

    def evaluate(self, agent, n_episodes: int = 1, *, deterministic: bool = True, norm_state: Optional[torch.Tensor] = None,
                 obs_clip: float = 1.0, epsilon: float = 1e-8, max_steps_per_launch: int = 4096, capture_envs: int = 0,
                 max_frames: Optional[int] = None) -> EvaluationResult:
        """``n_episodes`` whole episodes per env under ``agent`` (a network with RPOLinearNetwork's attribute names -- with the
        reference's set encoder ``deep_sets`` or attention encoder ``embedding`` in front, if it has one -- or
        ``"vacuum_cleaner"``).  ``norm_state``: the trainer's statistics ([rows, 3 D + 4] float64, any number of rows: row
        ``e mod rows`` serves env ``e`` -- the trainer's normaliser is per env and the evaluation batch need not have its
        size), applied frozen.  Launches of at most ``max_steps_per_launch`` steps until every env has finished; the one host
        read per launch is ``progress[:, 0].min()``.  ``capture_envs = K > 0``: the frames of envs ``0..K-1`` are recorded in
        the same launches (``policy_evaluate``'s ``capture``) and come back as ``result.capture`` -- ``max_frames`` rows per
        env (default ``n_episodes x max_timesteps``, which every env fits), NaN where no step wrote -- for
        ``result.episode_memory(env, episode)``."""
        env, E = self.env, self.num_envs
        capture, K = None, int(capture_envs)
        if K:
            F = int(n_episodes) * int(env.env_config.max_timesteps) if max_frames is None else int(max_frames)
            if not 1 <= K <= E or F < 1 or int(n_episodes) < 1:
                raise ValueError(f"evaluate: capture_envs must be in 0..{E} and max_frames, n_episodes >= 1, got {K}, {F}, {n_episodes}")
            nan = lambda rows: torch.full((rows, K, env.n_ped + 1, 3), float("nan"), dtype=torch.float32, device=env.device)  # noqa: E731
            capture = {"frames": nan(F), "starts": nan(int(n_episodes))}       # (once per evaluation: every launch gets the same two)
        norm = None
        if norm_state is not None:
            W = 3 * env.obs_dim + 4
            if norm_state.dim() != 2 or norm_state.shape[1] != W or norm_state.dtype != torch.float64 or norm_state.shape[0] < 1:
                raise ValueError(f"evaluate: norm_state must be float64 [rows, {W}], got {norm_state.dtype} {tuple(norm_state.shape)}")
            rows = torch.arange(E, device=env.device) % norm_state.shape[0]
            norm = (norm_state.to(env.device)[rows].contiguous(), float(obs_clip), float(epsilon))
        progress, out = self._run(n_episodes, max_steps_per_launch, lambda progress, out: env.policy_evaluate(
            agent, n_episodes, max_steps_per_launch, progress, out, deterministic=deterministic, _norm=norm, capture=capture))
        result = EvaluationResult.from_records(out, progress[:, 1].clone(), env.n_ped)
        result.capture = capture
        return result


def check_population_norm_state(norm_state, num_learners: int, obs_dim: int):
    """``PopulationEvaluator.evaluate``'s ``norm_state``: float64 [S, rows, 3 D + 4], or a sequence of S float64 [rows_s, 3 D + 4]
    (rows >= 1).  Returns the S tensors; ``ValueError`` otherwise."""
    S, W = int(num_learners), 3 * int(obs_dim) + 4
    parts = list(norm_state.unbind(0)) if isinstance(norm_state, torch.Tensor) and norm_state.dim() == 3 else norm_state
    if isinstance(parts, torch.Tensor) or not isinstance(parts, (list, tuple)) or len(parts) != S:
        if isinstance(parts, torch.Tensor):
            got = f"a tensor {tuple(parts.shape)}"
        else:
            got = f"{type(parts).__name__} of {len(parts)}" if hasattr(parts, "__len__") else type(parts).__name__
        raise ValueError(f"evaluate: norm_state must be float64 [{S}, rows, {W}] or a sequence of {S} tensors [rows, {W}], got {got}")
    for s, t in enumerate(parts):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != W or t.dtype != torch.float64 or t.shape[0] < 1:
            what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"evaluate: norm_state of learner {s} must be float64 [rows, {W}], got {what}")
    return parts


class PopulationEvaluator(_Evaluator):
    """``PolicyEvaluator`` for the S learners of a ``PolicyPopulation``, a ``DeepSetsPopulation`` or a ``TransformerPopulation`` in
    one set of launches (``evac_policy_evaluate_population`` / ``evac_policy_evaluate_population_deepsets`` /
    ``evac_policy_evaluate_population_transformer``): ONE handle of
    ``num_learners x num_envs`` envs, reset once; learner s evaluates in envs ``[s E_l, (s + 1) E_l)`` with the global ids of
    envs ``[0, E_l)``, so every learner's result is, bit for bit, what
    ``PolicyEvaluator(num_envs=E_l, seed=seed).evaluate(nets[s], ...)`` gives -- the learners are compared on the same episodes.
    The snapshot is the reset state of envs ``[0, E_l)`` tiled S times: envs of one seed and the same global ids are identical,
    so no second handle is needed to take it from."""

    def __init__(self, env_config: EnvConfig, wrap_config: Optional[EnvWrappersConfig] = None, num_learners: int = 1,
                 num_envs: int = 1, seed: int = 0, device="cuda:0", options=None):
        from .population import MAX_LEARNERS
        S, E_l = int(num_learners), int(num_envs)
        if not 1 <= S <= MAX_LEARNERS:
            raise ValueError(f"PopulationEvaluator: {S} learners; expected 1..{MAX_LEARNERS}")
        if E_l < 1:
            raise ValueError(f"PopulationEvaluator: num_envs must be >= 1, got {E_l}")
        self.num_learners, self.num_envs = S, E_l
        self.env = BatchedEvacuationEnv(env_config, wrap_config, num_envs=S * E_l, device=device, seed=seed, autoreset=True,
                                        options=options)
        self.env.reset()
        self.snapshot = {}
        for k in _STATE:
            t = getattr(self.env, k)
            self.snapshot[k] = t[:E_l].repeat((S,) + (1,) * (t.dim() - 1))

    def evaluate(self, population, n_episodes: int = 1, *, deterministic: bool = True, norm_state=None, obs_clip: float = 1.0,
                 epsilon: float = 1e-8, max_steps_per_launch: int = 4096) -> List[EvaluationResult]:
        """``n_episodes`` whole episodes per env under every learner of ``population`` (any of the three kinds; a bare network, or
        a stand-in holding networks with an encoder, is a ``ValueError``): S ``EvaluationResult``s
        whose tensors are views of ONE records tensor [n_episodes, S, E_l, 10].  ``norm_state``: float64 [S, rows, 3 D + 4] or a list of S tensors
        [rows_s, 3 D + 4]; row ``i mod rows`` of learner s serves its env i, applied frozen.  Launches of at most
        ``max_steps_per_launch`` steps until every env of every learner has finished; the one host read per launch is
        ``progress[:, 0].min()`` over all learners."""
        from .policy import refuse_deepsets, refuse_transformer
        from .population import DeepSetsPopulation
        refuse_transformer(population, "PopulationEvaluator.evaluate")   # (a network where the population goes)
        if not isinstance(population, DeepSetsPopulation):
            refuse_deepsets(population, "PopulationEvaluator.evaluate")
        env, S, E_l = self.env, self.num_learners, self.num_envs
        if int(getattr(population, "num_learners", -1)) != S:
            raise ValueError(f"evaluate: the population has {getattr(population, 'num_learners', None)} learners, the evaluator {S}")
        norm = None
        if norm_state is not None:
            parts = check_population_norm_state(norm_state, S, env.obs_dim)
            rows = torch.arange(E_l, device=env.device)
            state = torch.cat([t.to(env.device)[rows % t.shape[0]] for t in parts]).contiguous()
            norm = (state, float(obs_clip), float(epsilon))
        progress, out = self._run(n_episodes, max_steps_per_launch, lambda progress, out: env.policy_evaluate_population(
            population, n_episodes, max_steps_per_launch, progress, out, deterministic=deterministic, shared_episodes=True, _norm=norm))
        records, steps = out.view(int(n_episodes), S, E_l, out.shape[-1]), progress[:, 1].clone().view(S, E_l)
        return [EvaluationResult.from_records(records[:, s], steps[s], env.n_ped) for s in range(S)]
