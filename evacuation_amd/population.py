"""Population training: S independent RPO learners in one set of launches, of one configuration or one each.

What the reference's users run is a sweep -- ``for sweep in 1 .. 10`` independent training processes per setting
(run_scripts/run_article_sweeps-*.sh).  At the reference's shape (3 envs x 2048 steps, minibatches of 192) one learner's
update is a chain of small launches on a nearly idle chip; here learner s rides in the same launches as learner 0:

* ``PolicyPopulation``: the 13 tensors of the actor-critic stacked ``[S, ...]``; ``nets[s]`` is a ``LinearActorCritic`` whose
  parameters (and ``.grad``) are views of row s, initialised exactly as ``torch.manual_seed(seeds[s]); LinearActorCritic(D)``.
* ``PopulationAdam``: the optimiser's moments stacked the same way and ``[S]`` headers; ``learners[s]`` is a ``DeviceAdam`` over
  row s.
* ``BatchedEvacuationEnv.policy_rollout_population``: the collection phase of all learners in one launch; learner s owns envs
  ``[s E_l, (s + 1) E_l)`` of one env of ``S E_l`` envs.
* ``rpo_update_population``: every learner's epochs and minibatches in one host call, four launches per minibatch step as for
  one learner (``evac_rpo_update_population``).
* ``PopulationTrainer``: one iteration of the reference's loop for all learners per ``update()``; ``evaluate()`` runs every
  learner's whole episodes in one set of launches (``evaluation.PopulationEvaluator``, ``evac_policy_evaluate_population``).
* ``DeepSetsPopulation``: the same for the deep-sets leader -- 19 stacked tensors, ``nets[s]`` a ``DeepSetsActorCritic`` of
  views.  ``PopulationAdam``, ``policy_rollout_population`` and ``PopulationTrainer`` take one as they take a ``PolicyPopulation``;
  its update is ``deepsets_update_population`` (``evac_deepsets_update_population``: seven launches per minibatch step, as for one
  such learner), its evaluation ``evac_policy_evaluate_population_deepsets`` (``PopulationEvaluator`` and ``evaluate()`` take
  it as they take a ``PolicyPopulation``).  A sweep of such learners is opt-in: the last item.
* ``TransformerPopulation``: the transformer leader's 13 + 16 per block stacked tensors, ``nets[s]`` a ``TransformerActorCritic``
  of views.  What runs such learners ON A HANDLE'S ENVS takes one -- ``policy_rollout_population``
  (``evac_policy_rollout_population_transformer``), ``policy_evaluate_population`` and ``PopulationEvaluator``
  (``evac_policy_evaluate_population_transformer``).  Their UPDATE is opt-in under names of its own, as ``TransformerAdam``
  stands beside ``DeviceAdam``: ``TransformerPopulationAdam`` (the 29 or 45 stacks of moments, ``learners[s]`` a
  ``TransformerAdam`` on row s), ``transformer_update_population`` (``evac_transformer_update_population``: 6 + num_blocks +
  norm_adv launches per minibatch step, as for one such learner) and ``PopulationTrainer(..., optimizer="device_transformer")``,
  under ONE configuration.  The default faces -- ``PopulationAdam(population)`` and ``PopulationTrainer(env, population, cfg)``
  -- keep refusing one; a sweep of such learners is opt-in: the last item.
* Sweeps: every float-valued hyperparameter (``SWEEP_FIELDS``) may differ per learner -- ``PopulationTrainer(env, population,
  [cfg_0, .., cfg_S-1])``, ``rpo_update_population(cfg=[...])``, ``gae(gamma=[...])``, ``policy_rollout_population(gammas=[...])``;
  ``sweep_configs`` makes the cartesian product.  The learners' values ride in the kernel arguments beside their seeds
  (``evac_rpo_update_sweep``, ``evac_gae_learners``, ``evac_policy_rollout_sweep``).  What fixes launch geometry, step counts
  or storage shape (``STRUCTURAL_FIELDS``) stays one value for all.
* Sweeps of the two encoder populations, opt-in under names of their own (every default face keeps its refusal):
  ``policy_rollout_sweep(population, .., gammas)`` on both envs (``evac_policy_rollout_sweep_deepsets`` / ``_transformer``),
  ``deepsets_update_sweep`` / ``transformer_update_sweep`` (``evac_deepsets_update_sweep`` / ``evac_transformer_update_sweep``: the
  population's launches, the loss coefficients in the kernel arguments, the optimiser's values in a table at the workspace's
  tail that one small launch per call fills) and ``PopulationTrainer(env, population, cfgs, ..., encoder_sweep=True)``.

Learner s is BIT FOR BIT the ``RPOTrainer(optimizer="device", one_call=True)`` it would be alone on an env of ``E_l`` envs with the
population env's seed and ``env_id_offset`` further by ``s E_l``, with its own configuration, ``cfg.seed = seeds[s]`` and the
same reset state (wrapped, for a gamma sweep, with its own gamma).  Env settings are per population."""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .policy import (HIDDEN, SET_HIDDEN, DeepSetsActorCritic, LinearActorCritic, TransformerActorCritic, _check_encoder,
                     _check_structure, _check_transformer, _transformer_grads, _transformer_struct, all_tensors, mlp_tensors,
                     refuse_deepsets, refuse_dropout, refuse_transformer)
from .trainer import (BATCH_KEYS, DeviceAdam, RPOTrainingConfig, TransformerAdam, _f32, _loss_config, _stream, _u64, decode_header,
                      flatten_batch, gae, update_steps)
from .vector_env import STATS_FIELDS, _ptr

MAX_LEARNERS = _lib.MAX_LEARNERS
# what may differ between the learners of one population, and what may not (launch geometry, step counts, storage shape)
SWEEP_FIELDS = ("learning_rate", "anneal_lr", "gamma", "gae_lambda", "clip_coef", "ent_coef", "vf_coef", "rpo_alpha", "max_grad_norm",
                "target_kl")
STRUCTURAL_FIELDS = ("num_envs", "num_steps", "total_timesteps", "num_minibatches", "update_epochs", "norm_adv", "clip_vloss")


def _per_learner(value, n: int, name: str) -> list:
    """One value for all learners, or a sequence of ``n``."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} entries for {n} learners")
        return list(value)
    return [value] * n


def check_structure(cfgs: Sequence, what: str = "configuration") -> None:
    """Every learner's structural fields are learner 0's, or a ``ValueError`` naming the field and the learner."""
    for s, c in enumerate(cfgs):
        for f in STRUCTURAL_FIELDS:
            if getattr(c, f, None) != getattr(cfgs[0], f, None):
                raise ValueError(f"{what}: {f} = {getattr(c, f, None)!r} of learner {s} differs from learner 0's "
                                 f"{getattr(cfgs[0], f, None)!r}; {f} fixes the launches' shape and is one value per population")


def sweep_configs(base: RPOTrainingConfig, grid: Dict[str, Sequence], seeds: Optional[Sequence[int]] = None, net=None) -> list:
    """The cartesian product of ``grid`` (field of ``RPOTrainingConfig`` -> its values) over ``seeds`` (default: ``base.seed``)
    as a list of ``(seed, cfg)``, ``cfg = replace(base, seed=seed, **setting)``: the first field varies slowest, the seeds
    fastest (a setting's seeds are neighbours).  ``ValueError`` for an unknown field or more than ``MAX_LEARNERS`` learners, and
    for a ``net`` (the network the sweep is meant for, optional) with a set encoder: populations are the linear network's."""
    refuse_deepsets(net, "sweep_configs")
    names = {f.name for f in dataclasses.fields(base)}
    for f, values in grid.items():
        if f not in names or f == "seed":
            raise ValueError(f"sweep_configs: {f!r} is not a field of {type(base).__name__} to sweep")
        if len(values) < 1:
            raise ValueError(f"sweep_configs: no values for {f!r}")
    seeds = [int(base.seed)] if seeds is None else [int(s) for s in seeds]
    n = len(seeds)
    for values in grid.values():
        n *= len(values)
    if not 1 <= n <= MAX_LEARNERS:
        raise ValueError(f"sweep_configs: {n} learners; a population holds 1..{MAX_LEARNERS}")
    out = []
    for setting in itertools.product(*grid.values()):
        for seed in seeds:
            out.append((seed, dataclasses.replace(base, seed=seed, **dict(zip(grid, setting)))))
    return out


def population_rows(inds: torch.Tensor, learner, envs_per_learner: int, num_learners: int) -> torch.Tensor:
    """Sample ``i`` of a learner's own batch ``[T, E_l]`` (flattened) -> its row of the common batch ``[T, S E_l]`` (flattened):
    ``(i // E_l) (S E_l) + s E_l + i % E_l``.  ``learner``: an int, or a tensor that broadcasts against ``inds``."""
    E_l, S = int(envs_per_learner), int(num_learners)
    return torch.div(inds, E_l, rounding_mode="floor") * (S * E_l) + learner * E_l + inds % E_l


def _bind_row(net, tensors, grads, s: int) -> None:
    """The parameters of ``net`` (``all_tensors`` order: 13, or 19 with a set encoder, or 13 + 16 per block with an attention
    encoder) become views of row s of ``tensors`` (and their ``.grad`` views of row s of ``grads``)."""
    a, c = net.actor_mean, net.critic
    owners = [(a[0], "weight"), (a[0], "bias"), (a[2], "weight"), (a[2], "bias"), (a[4], "weight"), (a[4], "bias"),
              (net, "actor_logstd"), (c[0], "weight"), (c[0], "bias"), (c[2], "weight"), (c[2], "bias"), (c[4], "weight"), (c[4], "bias")]
    if len(tensors) == 19:
        phi, rho = net.deep_sets.transform_phi, net.deep_sets.transform_rho
        owners += [(phi[0], "weight"), (phi[0], "bias"), (phi[2], "weight"), (phi[2], "bias"), (rho[0], "weight"), (rho[0], "bias")]
    elif len(tensors) > 13:                   # (``policy._BLOCK_TENSORS``' order, block by block)
        for blk in net.embedding:
            at = blk.attention
            owners += [(m, name) for m in (at.Wq, at.Wk, at.Wv, at.dense, blk.ff[0], blk.ff[3], blk.norm1, blk.norm2)
                       for name in ("weight", "bias")]
    for i, (mod, name) in enumerate(owners):
        prm = nn.Parameter(tensors[i][s])
        prm.grad = grads[i][s]
        setattr(mod, name, prm)


class PolicyPopulation:
    """S actor-critics of observation width ``obs_dim`` as 13 stacked tensors ``[S, ...]`` on ``device``; see the module's
    docstring.  ``tensors`` / ``grads``: the stacks, in ``evac_mlp_policy_t`` order; ``strides``: a learner's distance in each."""

    def __init__(self, obs_dim: int, seeds: Sequence[int], device="cuda:0", net=None):
        """``net``: the network the learners are meant to copy, optional and only checked -- the learners are
        ``LinearActorCritic``s; one with a set encoder is a ``ValueError``."""
        refuse_deepsets(net, "PolicyPopulation")
        seeds = [int(s) for s in seeds]
        if not 1 <= len(seeds) <= MAX_LEARNERS:
            raise ValueError(f"PolicyPopulation: {len(seeds)} learners; expected 1..{MAX_LEARNERS}")
        self.obs_dim, self.seeds, self.device = int(obs_dim), seeds, torch.device(device)
        self.num_learners = len(seeds)
        fresh = []
        with torch.random.fork_rng(devices=[]):                # (the caller's generator is left where it was)
            for seed in seeds:
                torch.manual_seed(seed)
                fresh.append(LinearActorCritic(self.obs_dim))
        with torch.no_grad():
            self.tensors = [torch.stack([mlp_tensors(n)[i].detach() for n in fresh]).to(self.device).contiguous() for i in range(13)]
        self.grads = [torch.zeros_like(t) for t in self.tensors]
        self.nets: List[LinearActorCritic] = []
        for s, net in enumerate(fresh):
            self._bind(net, s)
            self.nets.append(net)
            _check_structure(net, self.obs_dim, self.device)
        self.strides = _lib.EvacMlpPolicyStrides(*(int(t[0].numel()) for t in self.tensors))
        self._policy = _lib.EvacMlpPolicy(self.obs_dim, HIDDEN, *(t.data_ptr() for t in self.tensors))

    def _bind(self, net: LinearActorCritic, s: int) -> None:
        """The parameters of ``net`` become views of row s (and their ``.grad`` views of the gradients' row s)."""
        _bind_row(net, self.tensors, self.grads, s)

    def policy_struct(self) -> "_lib.EvacMlpPolicy":
        """``evac_mlp_policy_t`` of learner 0, the base the strides count from (every learner's views were checked when made)."""
        return self._policy


class DeepSetsPopulation:
    """S deep-sets leaders (``DeepSetsActorCritic(obs_dim, number_of_pedestrians)``) as 19 stacked tensors ``[S, ...]`` on
    ``device``: the actor-critic's 13 in ``evac_mlp_policy_t`` order, then the set encoder's 6 in ``evac_deepsets_t`` order
    (``all_tensors``).  ``nets[s]`` is a ``DeepSetsActorCritic`` whose parameters (and ``.grad``) are views of row s, initialised
    exactly as ``torch.manual_seed(seeds[s]); DeepSetsActorCritic(obs_dim, number_of_pedestrians)``: ``policy_rollout``,
    ``policy_evaluate``, ``PolicyEvaluator`` and ``DeviceAdam`` take a learner as they take any such network.  ``strides`` /
    ``encoder_strides``: a learner's distance in each of the 13 / the 6."""

    def __init__(self, obs_dim: int, number_of_pedestrians: int, seeds: Sequence[int], device="cuda:0"):
        seeds = [int(s) for s in seeds]
        if not 1 <= len(seeds) <= MAX_LEARNERS:
            raise ValueError(f"DeepSetsPopulation: {len(seeds)} learners; expected 1..{MAX_LEARNERS}")
        self.obs_dim, self.number_of_pedestrians = int(obs_dim), int(number_of_pedestrians)
        self.seeds, self.device, self.num_learners = seeds, torch.device(device), len(seeds)
        fresh = []
        with torch.random.fork_rng(devices=[]):                # (the caller's generator is left where it was)
            for seed in seeds:
                torch.manual_seed(seed)
                fresh.append(DeepSetsActorCritic(self.obs_dim, self.number_of_pedestrians))
        with torch.no_grad():
            self.tensors = [torch.stack([all_tensors(n)[i].detach() for n in fresh]).to(self.device).contiguous() for i in range(19)]
        self.grads = [torch.zeros_like(t) for t in self.tensors]
        self.nets: List[DeepSetsActorCritic] = []
        for s, net in enumerate(fresh):
            _bind_row(net, self.tensors, self.grads, s)
            self.nets.append(net)
            _check_structure(net, self.obs_dim, self.device)
            self.set_elem_dim = _check_encoder(net, self.obs_dim, self.device, self.number_of_pedestrians)
        sizes = [int(t[0].numel()) for t in self.tensors]
        self.strides = _lib.EvacMlpPolicyStrides(*sizes[:13])
        self.encoder_strides = _lib.EvacDeepSetsStrides(*sizes[13:])
        self._policy = _lib.EvacMlpPolicy(self.obs_dim, HIDDEN, *(t.data_ptr() for t in self.tensors[:13]))
        self._encoder = _lib.EvacDeepSets(self.set_elem_dim, SET_HIDDEN, *(t.data_ptr() for t in self.tensors[13:]))

    def policy_struct(self) -> "_lib.EvacMlpPolicy":
        """``evac_mlp_policy_t`` of learner 0, the base the strides count from (every learner's views were checked when made)."""
        return self._policy

    def encoder_struct(self) -> "_lib.EvacDeepSets":
        """``evac_deepsets_t`` of learner 0, the base ``encoder_strides`` count from."""
        return self._encoder


class TransformerPopulation:
    """S transformer leaders (``TransformerActorCritic(obs_dim, number_of_pedestrians, num_blocks=..., use_resid=...)``, dropout 0)
    as ``13 + 16 num_blocks`` stacked tensors ``[S, ...]`` on ``device``: the actor-critic's 13 in ``evac_mlp_policy_t`` order,
    then each block's 16 in ``evac_transformer_block_t`` order (``all_tensors``).  ``nets[s]`` is a ``TransformerActorCritic``
    whose parameters (and ``.grad``) are views of row s, initialised exactly as ``torch.manual_seed(seeds[s]);
    TransformerActorCritic(obs_dim, number_of_pedestrians, num_blocks=..., use_resid=...)``: ``policy_rollout``,
    ``policy_evaluate``, ``PolicyEvaluator`` and ``TransformerAdam`` take a learner as they take any such network.  ``strides``
    / ``encoder_strides``: a learner's distance in each of the 13 / of the blocks' 16.  The blocks' number, the token width and
    ``use_resid`` are one value per population.  The entries that run the learners on a handle's envs take the object
    (``policy_rollout_population``, ``policy_evaluate_population``, ``PopulationEvaluator``); the learners' update in one set
    of launches is opt-in (``TransformerPopulationAdam``, ``transformer_update_population``,
    ``PopulationTrainer(..., optimizer="device_transformer")``): the default faces refuse one with ``UPDATE_NOT_BUILT``."""

    UPDATE_NOT_BUILT = ("the update of transformer learners is not built into PopulationAdam(population) and "
                        "PopulationTrainer(env, population, cfg): these two default faces do not take a TransformerPopulation.  Its "
                        "gradient, clip and Adam in one set of launches are opt-in: TransformerPopulationAdam, "
                        "transformer_update_population and PopulationTrainer(..., optimizer=\"device_transformer\"); what else takes one "
                        "is policy_rollout_population, policy_evaluate_population and PopulationEvaluator, and a learner trains alone "
                        "with RPOTrainer(grad_fn=transformer_kernel_grad, optimizer=\"device_transformer\") on nets[s]")

    def __init__(self, obs_dim: int, number_of_pedestrians: int, seeds: Sequence[int], device="cuda:0", num_blocks: int = 2,
                 use_resid: bool = False):
        seeds = [int(s) for s in seeds]
        if not 1 <= len(seeds) <= MAX_LEARNERS:
            raise ValueError(f"TransformerPopulation: {len(seeds)} learners; expected 1..{MAX_LEARNERS}")
        self.obs_dim, self.number_of_pedestrians = int(obs_dim), int(number_of_pedestrians)
        if self.number_of_pedestrians < 0 or self.obs_dim % (self.number_of_pedestrians + 2):
            raise ValueError(f"TransformerPopulation: an observation of {self.obs_dim} floats is not a whole number of floats for each "
                             f"of the {self.number_of_pedestrians} + 2 tokens (a Box observation is needed)")
        self.seeds, self.device, self.num_learners = seeds, torch.device(device), len(seeds)
        fresh = []
        with torch.random.fork_rng(devices=[]):                # (the caller's generator is left where it was)
            for seed in seeds:
                torch.manual_seed(seed)
                fresh.append(TransformerActorCritic(self.obs_dim, self.number_of_pedestrians, num_blocks=int(num_blocks),
                                                    use_resid=bool(use_resid)))
        count = len(all_tensors(fresh[0]))                      # 13 + 16 per block
        with torch.no_grad():
            self.tensors = [torch.stack([all_tensors(n)[i].detach() for n in fresh]).to(self.device).contiguous() for i in range(count)]
        self.grads = [torch.zeros_like(t) for t in self.tensors]
        self.nets: List[TransformerActorCritic] = []
        for s, net in enumerate(fresh):
            _bind_row(net, self.tensors, self.grads, s)
            self.nets.append(net)
            _check_structure(net, self.obs_dim, self.device)
            found = _check_transformer(net, self.obs_dim, self.device, self.number_of_pedestrians)
        self.token_dim, self.num_blocks, self.use_resid = found
        sizes = [int(t[0].numel()) for t in self.tensors]
        self.strides = _lib.EvacMlpPolicyStrides(*sizes[:13])
        self.encoder_strides = _lib.EvacTransformerStrides()
        for b in range(self.num_blocks):
            self.encoder_strides.blocks[b] = _lib.EvacTransformerBlockStrides(*sizes[13 + 16 * b:29 + 16 * b])
        self._policy = _lib.EvacMlpPolicy(self.obs_dim, HIDDEN, *(t.data_ptr() for t in self.tensors[:13]))
        self._encoder = _transformer_struct(found, self.tensors[13:])

    def policy_struct(self) -> "_lib.EvacMlpPolicy":
        """``evac_mlp_policy_t`` of learner 0, the base the strides count from (every learner's views were checked when made)."""
        return self._policy

    def encoder_struct(self) -> "_lib.EvacTransformer":
        """``evac_transformer_t`` of learner 0, the base ``encoder_strides`` count from."""
        return self._encoder


class PopulationAdam:
    """``DeviceAdam`` for every learner of ``population``: the moments stacked ``[S, ...]``, ``headers`` ``[S, 8]`` (64 bytes a
    learner).  ``learners[s]`` is a ``DeviceAdam`` whose state is row s and whose ``param_groups`` are its own: ``lr`` and
    ``max_grad_norm`` (one value or a sequence of S) may differ per learner, the betas and eps are one value for all.
    ``param_groups[s]`` is learner s's group; ``state_dict(s)`` / ``load_state_dict(s, sd)`` are its, in ``DeviceAdam``'s
    format, and touch no other learner.  For a ``DeepSetsPopulation`` the stacks are its 19 and ``learners[s]`` a ``DeviceAdam``
    over all 19 tensors of row s.  A ``TransformerPopulation`` is a ``ValueError``: its optimiser is
    ``TransformerPopulationAdam``."""

    def __init__(self, population, lr=3e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm=0.5):
        if isinstance(population, TransformerPopulation):
            raise ValueError(f"PopulationAdam: {TransformerPopulation.UPDATE_NOT_BUILT}")
        self._setup(population, lr, betas, eps, max_grad_norm, DeviceAdam)

    def _setup(self, population, lr, betas, eps, max_grad_norm, make) -> None:
        """The constructor's body; ``make``: the learners' optimiser (``DeviceAdam``, ``TransformerAdam``)."""
        self.population = population
        S, dev = population.num_learners, population.device
        lrs, norms = _per_learner(lr, S, "lr"), _per_learner(max_grad_norm, S, "max_grad_norm")
        self.headers = torch.zeros(S, 8, dtype=torch.int64, device=dev)
        self.exp_avg = [torch.zeros_like(t) for t in population.tensors]
        self.exp_avg_sq = [torch.zeros_like(t) for t in population.tensors]
        self.learners = [make(net, lr=lrs[s], betas=betas, eps=eps, max_grad_norm=norms[s],
                              storage=(self.headers[s], [m[s] for m in self.exp_avg], [v[s] for v in self.exp_avg_sq]))
                         for s, net in enumerate(population.nets)]
        self.header_stride_bytes = 64
        self.moment_strides = population.strides
        self.encoder_moment_strides = (population.encoder_strides
                                       if isinstance(population, (DeepSetsPopulation, TransformerPopulation)) else None)

    @property
    def param_groups(self) -> List[dict]:
        """Learner s's group at index s (read at every call, as ``DeviceAdam.param_groups[0]``)."""
        return [opt.param_groups[0] for opt in self.learners]

    def set_lr(self, lr) -> None:
        """``lr``: one value for all learners or a sequence of S."""
        for opt, x in zip(self.learners, _per_learner(lr, len(self.learners), "lr")):
            opt.param_groups[0]["lr"] = float(x)

    def uniform(self) -> bool:
        """Every learner's ``lr`` and ``max_grad_norm`` are learner 0's."""
        g0 = self.learners[0].param_groups[0]
        return all(o.param_groups[0]["lr"] == g0["lr"] and o.param_groups[0]["max_grad_norm"] == g0["max_grad_norm"]
                   for o in self.learners)

    def config(self, learner: int = 0) -> "_lib.EvacAdamConfig":
        """``evac_adam_config_t`` of one learner.  The betas and eps are shared by all: a learner whose differ is an error."""
        g0 = self.learners[0].param_groups[0]
        for s, opt in enumerate(self.learners):
            g = opt.param_groups[0]
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise ValueError(f"PopulationAdam: betas / eps of learner {s} differ from learner 0's; they are one value per population")
        return self.learners[learner].config()

    def read_headers(self) -> List[dict]:
        host = self.headers.cpu()
        return [decode_header(h) for h in host]

    def state_dict(self, learner: int) -> dict:
        return self.learners[learner].state_dict()

    def load_state_dict(self, learner: int, sd: dict) -> None:
        self.learners[learner].load_state_dict(sd)


class TransformerPopulationAdam(PopulationAdam):
    """``PopulationAdam`` for a ``TransformerPopulation``: the same interface and body over its 13 + 16 per block stacks (29 or
    45), ``learners[s]`` a ``TransformerAdam`` whose state is row s, ``encoder_moment_strides`` the population's
    ``encoder_strides``.  A class of its own because ``PopulationAdam(population)`` stays a ``ValueError`` for such a
    population.  Anything but a ``TransformerPopulation`` is a ``ValueError``."""

    def __init__(self, population, lr=3e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm=0.5):
        if not isinstance(population, TransformerPopulation):
            raise ValueError(f"TransformerPopulationAdam: a TransformerPopulation is expected, got {type(population).__name__} "
                             "(a PolicyPopulation's or DeepSetsPopulation's optimiser is PopulationAdam)")
        self._setup(population, lr, betas, eps, max_grad_norm, TransformerAdam)


def _batch_ptrs(batch: Dict[str, torch.Tensor]):
    b_obs = batch["b_obs"]
    B, D = b_obs.shape
    _f32(b_obs, (B, D), "b_obs")
    _f32(batch["b_actions"], (B, 2), "b_actions")
    for k in BATCH_KEYS[2:]:
        _f32(batch[k], (B,), k)
    return int(B), int(D), [int(B)] + [_ptr(batch[k]) for k in BATCH_KEYS]


def population_workspace_bytes(obs_dim: int, minibatch_size: int, num_learners: int, *, deepsets: bool = False,
                               transformer: bool = False, sweep: bool = False) -> int:
    """The update's workspace for a ``PolicyPopulation``, or with ``deepsets`` for a ``DeepSetsPopulation``, or with
    ``transformer`` for a ``TransformerPopulation`` (both at once is a ``ValueError``).  ``sweep``: what
    ``deepsets_update_sweep`` / ``transformer_update_sweep`` need (``evac_*_sweep_workspace_bytes``: the population's, then the
    table of the learners' optimiser values); a ``PolicyPopulation``'s sweep needs no more than its population."""
    if deepsets and transformer:
        raise ValueError("population_workspace_bytes: deepsets and transformer name two kinds of population")
    kind = "transformer" if transformer else "deepsets" if deepsets else "rpo"
    sizer = f"evac_{kind}_{'sweep' if sweep and kind != 'rpo' else 'population'}_workspace_bytes"
    need = int(getattr(_lib.load(), sizer)(int(obs_dim), int(minibatch_size), int(num_learners)))
    if need < 0:
        raise _lib.EvacError(need, f"{sizer}({obs_dim}, {minibatch_size}, {num_learners})")
    return need


def learner_hypers(cfgs: Sequence, opt: Optional[PopulationAdam] = None):
    """``evac_learner_hyper_t[S]`` of the configurations; with ``opt`` the learning rate and ``max_grad_norm`` are the
    optimiser's (``opt.learners[s].param_groups[0]``: the annealed rate), as ``rpo_update`` takes them from its ``DeviceAdam``."""
    S = len(cfgs)
    col = lambda f, default: [getattr(c, f, default) for c in cfgs]
    groups = None if opt is None else opt.param_groups
    return _lib.learner_hypers(
        S, learning_rate=col("learning_rate", 3e-4) if groups is None else [g["lr"] for g in groups],
        max_grad_norm=col("max_grad_norm", 0.5) if groups is None else [g["max_grad_norm"] for g in groups],
        target_kl=col("target_kl", None), gamma=col("gamma", 0.99), gae_lambda=col("gae_lambda", 0.95), clip_coef=col("clip_coef", 0.2),
        ent_coef=col("ent_coef", 0.0), vf_coef=col("vf_coef", 0.5), rpo_alpha=col("rpo_alpha", 0.5))


def rpo_update_population(population: PolicyPopulation, batch: Dict[str, torch.Tensor], rows: torch.Tensor, cfg, opt: PopulationAdam, *,
                          minibatch_size: Optional[int] = None, rpo_noise: Optional[torch.Tensor] = None,
                          seeds: Optional[Sequence[int]] = None, first_draw_counters: Optional[Sequence[int]] = None,
                          stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``rpo_update`` for every learner in one host call (``evac_rpo_update_population``).  ``batch``: the COMMON flat arrays
    (``flatten_batch`` of the population's storage); ``rows`` int64 ``[S, epochs, B_l]``: per learner and epoch the rows of the
    common batch in the order the learner visits them (``population_rows`` of its permutation of ``[0, B_l)``).  Learner s draws
    its RPO perturbation from Philox keyed ``seeds[s]`` (default ``population.seeds``) at ``first_draw_counters[s] + k`` for step
    k, or reads ``rpo_noise[s, k]`` (``[S, steps, M, 2]``).  Returns (``stats`` ``[S, steps, 8]``, ``opt.headers``); rows beyond a
    learner's ``steps_run`` keep what they held.  No host synchronisation; four launches per minibatch step.
    ``cfg``: one configuration, or a sequence of S (``evac_rpo_update_sweep``): learner s's loss runs with ``cfg[s]``'s
    ``clip_coef`` / ``ent_coef`` / ``vf_coef`` / ``rpo_alpha`` / ``target_kl`` and its optimiser with
    ``opt.learners[s].param_groups[0]``'s ``lr`` / ``max_grad_norm``, bit for bit ``rpo_update(..., cfg[s], DeviceAdam(lr, ...))``
    alone; ``norm_adv``, ``clip_vloss`` and the minibatch size are learner 0's and must be everybody's.  With one ``cfg`` the
    optimiser's per-learner values are honoured in the same way."""
    if isinstance(population, DeepSetsPopulation):
        raise ValueError("rpo_update_population: a DeepSetsPopulation's update is deepsets_update_population")
    return _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace,
                              "rpo_update_population")


def deepsets_update_population(population: DeepSetsPopulation, batch: Dict[str, torch.Tensor], rows: torch.Tensor, cfg,
                               opt: PopulationAdam, *, minibatch_size: Optional[int] = None, rpo_noise: Optional[torch.Tensor] = None,
                               seeds: Optional[Sequence[int]] = None, first_draw_counters: Optional[Sequence[int]] = None,
                               stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``deepsets_update`` for every learner of a ``DeepSetsPopulation`` in one host call (``evac_deepsets_update_population``):
    ``rpo_update_population``'s arguments and returns, with ONE configuration -- learner s is, bit for bit,
    ``deepsets_update(population.nets[s], its own rows, cfg, DeviceAdam(nets[s]), seed=seeds[s],
    first_draw_counter=first_draw_counters[s])`` alone.  Seven launches per minibatch step (six without ``norm_adv``), no host
    synchronisation.  A sequence of configurations, or an optimiser whose learners differ in ``lr`` / ``max_grad_norm``, is a
    ``ValueError`` here ("sweeps of deep-sets learners are not built" into this entry): that is ``deepsets_update_sweep``."""
    if not isinstance(population, DeepSetsPopulation):
        raise ValueError("deepsets_update_population: a DeepSetsPopulation is expected (a PolicyPopulation's update is "
                         "rpo_update_population)")
    if isinstance(cfg, (list, tuple)) or not opt.uniform():
        raise ValueError("deepsets_update_population: sweeps of deep-sets learners are not built: one configuration, and one lr / "
                         "max_grad_norm, for all learners")
    return _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace,
                              "deepsets_update_population")


def transformer_update_population(population: TransformerPopulation, batch: Dict[str, torch.Tensor], rows: torch.Tensor, cfg,
                                  opt: TransformerPopulationAdam, *, minibatch_size: Optional[int] = None,
                                  rpo_noise: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None,
                                  first_draw_counters: Optional[Sequence[int]] = None, stats: Optional[torch.Tensor] = None,
                                  workspace: Optional[torch.Tensor] = None):
    """``transformer_update`` for every learner of a ``TransformerPopulation`` in one host call
    (``evac_transformer_update_population``): ``deepsets_update_population``'s arguments and returns, with ONE configuration --
    learner s is, bit for bit, ``transformer_update(population.nets[s], its own rows, cfg, TransformerAdam(nets[s]),
    seed=seeds[s], first_draw_counter=first_draw_counters[s])`` alone.  ``6 + num_blocks`` launches per minibatch step and one
    more with ``norm_adv``, no host synchronisation.  A sequence of configurations, or an optimiser whose learners differ in
    ``lr`` / ``max_grad_norm``, is a ``ValueError`` here ("sweeps of transformer learners are not built" into this entry): that is
    ``transformer_update_sweep``."""
    if not isinstance(population, TransformerPopulation):
        raise ValueError("transformer_update_population: a TransformerPopulation is expected (a PolicyPopulation's update is "
                         "rpo_update_population, a DeepSetsPopulation's deepsets_update_population)")
    if not isinstance(opt, TransformerPopulationAdam):
        raise ValueError(f"transformer_update_population: a TransformerPopulationAdam is expected, got {type(opt).__name__}")
    if isinstance(cfg, (list, tuple)) or not opt.uniform():
        raise ValueError("transformer_update_population: sweeps of transformer learners are not built: one configuration, and one "
                         "lr / max_grad_norm, for all learners")
    for net in population.nets:
        refuse_dropout(net, "transformer_update_population")
    return _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace,
                              "transformer_update_population")


def deepsets_update_sweep(population: DeepSetsPopulation, batch: Dict[str, torch.Tensor], rows: torch.Tensor, cfg, opt: PopulationAdam,
                          *, minibatch_size: Optional[int] = None, rpo_noise: Optional[torch.Tensor] = None,
                          seeds: Optional[Sequence[int]] = None, first_draw_counters: Optional[Sequence[int]] = None,
                          stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``deepsets_update_population`` with a configuration per learner (``evac_deepsets_update_sweep``): the same arguments and
    returns; ``cfg`` is one configuration or a sequence of S, and the optimiser's per-learner ``lr`` / ``max_grad_norm`` are
    honoured.  Learner s is, bit for bit, ``deepsets_update(population.nets[s], its own rows, cfg[s], DeviceAdam(nets[s],
    lr=.., max_grad_norm=..), seed=seeds[s], first_draw_counter=first_draw_counters[s])`` alone: its loss runs with
    ``cfg[s]``'s ``clip_coef`` / ``ent_coef`` / ``vf_coef`` / ``rpo_alpha`` / ``target_kl``.  ``norm_adv``, ``clip_vloss`` and the
    minibatch size are learner 0's and must be everybody's.  The population's launches and one small one per call; the
    workspace is ``population_workspace_bytes(..., deepsets=True, sweep=True)``."""
    if not isinstance(population, DeepSetsPopulation):
        raise ValueError("deepsets_update_sweep: a DeepSetsPopulation is expected (a PolicyPopulation's sweep is "
                         "rpo_update_population with a sequence of configurations)")
    return _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace,
                              "deepsets_update_sweep", sweep=True)


def transformer_update_sweep(population: TransformerPopulation, batch: Dict[str, torch.Tensor], rows: torch.Tensor, cfg,
                             opt: TransformerPopulationAdam, *, minibatch_size: Optional[int] = None,
                             rpo_noise: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None,
                             first_draw_counters: Optional[Sequence[int]] = None, stats: Optional[torch.Tensor] = None,
                             workspace: Optional[torch.Tensor] = None):
    """``transformer_update_population`` with a configuration per learner (``evac_transformer_update_sweep``), as
    ``deepsets_update_sweep`` is ``deepsets_update_population``'s: learner s is, bit for bit, ``transformer_update(
    population.nets[s], its own rows, cfg[s], TransformerAdam(nets[s], lr=.., max_grad_norm=..), seed=seeds[s],
    first_draw_counter=first_draw_counters[s])`` alone.  A dropout probability other than 0 is a ``ValueError``."""
    if not isinstance(population, TransformerPopulation):
        raise ValueError("transformer_update_sweep: a TransformerPopulation is expected (a PolicyPopulation's sweep is "
                         "rpo_update_population with a sequence of configurations, a DeepSetsPopulation's deepsets_update_sweep)")
    if not isinstance(opt, TransformerPopulationAdam):
        raise ValueError(f"transformer_update_sweep: a TransformerPopulationAdam is expected, got {type(opt).__name__}")
    for net in population.nets:
        refuse_dropout(net, "transformer_update_sweep")
    return _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace,
                              "transformer_update_sweep", sweep=True)


def _update_population(population, batch, rows, cfg, opt, minibatch_size, rpo_noise, seeds, first_draw_counters, stats, workspace, what,
                       sweep=False):
    """The body of ``rpo_update_population``, ``deepsets_update_population``, ``transformer_update_population`` and the two
    encoder sweeps (``what``: the caller's name; ``sweep``: an encoder population goes to its ``evac_*_update_sweep``)."""
    deepsets = isinstance(population, DeepSetsPopulation)
    transformer = isinstance(population, TransformerPopulation)
    if opt.population is not population:
        raise ValueError("the PopulationAdam was made for another population")
    S, dev = population.num_learners, population.device
    cfgs = None
    if isinstance(cfg, (list, tuple)):
        cfgs = list(cfg)
        if len(cfgs) != S:
            raise ValueError(f"{what}: {len(cfgs)} configurations for {S} learners")
        for s, c in enumerate(cfgs):
            for f in ("norm_adv", "clip_vloss") + (("minibatch_size",) if minibatch_size is None else ()):
                if getattr(c, f, True) != getattr(cfgs[0], f, True):
                    raise ValueError(f"{what}: {f} of learner {s} differs from learner 0's")
        cfg = cfgs[0]
    elif sweep or not opt.uniform():
        cfgs = [cfg] * S
    B, D, b_args = _batch_ptrs(batch)
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.device != batch["b_obs"].device or \
            not rows.is_contiguous() or rows.dim() != 3 or rows.shape[0] != S or rows.shape[1] < 1 or rows.shape[2] < 1:
        raise ValueError(f"rows: expected a contiguous int64 device tensor of shape [{S}, epochs, B_l]")
    n_epochs, B_l = int(rows.shape[1]), int(rows.shape[2])
    M = int(cfg.minibatch_size if minibatch_size is None else minibatch_size)
    norm_adv = bool(getattr(cfg, "norm_adv", True))
    if M < (2 if norm_adv else 1):
        raise ValueError(f"{what}: minibatch_size = {M}")
    M = min(M, B_l)
    steps = n_epochs * len(update_steps(B_l, M, norm_adv))
    if rpo_noise is not None:
        _f32(rpo_noise, (S, steps, M, 2), "rpo_noise")
    if stats is None:
        stats = torch.zeros(S, steps, 8, dtype=torch.float32, device=dev)
    else:
        _f32(stats, (S, steps, 8), "stats")
    need = population_workspace_bytes(D, M, S, deepsets=deepsets, transformer=transformer, sweep=sweep)
    if workspace is None or workspace.numel() < need or workspace.device != dev:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    seeds = population.seeds if seeds is None else [int(x) for x in seeds]
    counters = [0] * S if first_draw_counters is None else [int(x) for x in first_draw_counters]
    if len(seeds) != S or len(counters) != S:
        raise ValueError(f"{what}: seeds and first_draw_counters must have {S} entries")
    u64 = C.c_uint64 * S
    if D != population.obs_dim:
        raise ValueError(f"{what}: b_obs has {D} columns, the population's observation has {population.obs_dim}")
    pol = population.policy_struct()
    params = _lib.EvacMlpPolicyGrads(*(t.data_ptr() for t in population.tensors[:13]))
    grads = _lib.EvacMlpPolicyGrads(*(g.data_ptr() for g in population.grads[:13]))
    target_kl = getattr(cfg, "target_kl", None)
    lc, oc = _loss_config(cfg), opt.config()
    rest = [opt.header_stride_bytes, C.byref(lc), C.byref(oc), C.byref(opt.learners[0].state_struct()), *b_args,
            B_l, M, n_epochs, _ptr(rows), _ptr(rpo_noise), u64(*(_u64(x) for x in seeds)), u64(*(_u64(x) for x in counters))]
    tail = [_ptr(stats), _ptr(workspace), _stream(dev)]
    if deepsets or transformer:               # (every struct of the 13 followed by the encoder's)
        enc_struct = _transformer_grads if transformer else _lib.EvacDeepSetsGrads
        enc_params = enc_struct(*(t.data_ptr() for t in population.tensors[13:]))
        enc_grads = enc_struct(*(g.data_ptr() for g in population.grads[13:]))
        es = population.encoder_strides
        entry = getattr(_lib.load(), f"evac_{'transformer' if transformer else 'deepsets'}_update_{'sweep' if sweep else 'population'}")
        values = [learner_hypers(cfgs, opt)] if sweep else [int(target_kl is not None), float(target_kl or 0.0)]
        rc = entry(
            S, C.byref(pol), C.byref(population.encoder_struct()), C.byref(params), C.byref(enc_params), C.byref(grads), C.byref(enc_grads),
            C.byref(population.strides), C.byref(es), C.byref(population.strides), C.byref(es), C.byref(opt.moment_strides),
            C.byref(opt.encoder_moment_strides), *rest, *values, *tail)
        _lib.check(rc)
        return stats, opt.headers
    head = [S, C.byref(pol), C.byref(params), C.byref(grads), C.byref(population.strides), C.byref(population.strides),
            C.byref(opt.moment_strides), *rest]
    if cfgs is None:
        rc = _lib.load().evac_rpo_update_population(*head, int(target_kl is not None), float(target_kl or 0.0), *tail)
    else:
        rc = _lib.load().evac_rpo_update_sweep(*head, learner_hypers(cfgs, opt), *tail)
    _lib.check(rc)
    return stats, opt.headers


class PopulationTrainer:
    """``RPOTrainer(optimizer="device", one_call=True)`` for every learner of ``population`` at once.  ``env``: a
    ``NormalizedVectorEnv`` or ``BatchedEvacuationEnv`` of ``S x cfg.num_envs`` envs (learner s owns the s-th share);
    ``population``: a ``PolicyPopulation``, or a ``DeepSetsPopulation`` (learner s is then ``RPOTrainer(grad_fn=deepsets_kernel_grad,
    optimizer="device", one_call=True)`` alone, under ONE configuration: differing ones are a ``ValueError``); ``cfgs``: ONE
    configuration for all, or a sequence of S that may differ in ``SWEEP_FIELDS`` (a differing ``STRUCTURAL_FIELDS`` entry is a
    ``ValueError``); ``seed`` unused -- learner s's permutations come from a generator seeded ``population.seeds[s]`` and
    its RPO perturbation from Philox keyed with the same seed.  With a sequence learner s anneals its own rate, its reward
    normaliser runs with its own gamma (whatever the env was wrapped with) and its advantages, loss, clip and ``target_kl`` are
    its own.  ``update()``: anneal, one collection launch, one ``gae``, the permutations, one ``rpo_update_population``, ONE host
    transfer; returns a list of S logs with ``RPOTrainer.update()``'s keys, ``learning_rate`` the learner's own and ``config``
    its fields that differ from learner 0's.  A ``TransformerPopulation`` is a ``ValueError`` by default; with
    ``optimizer="device_transformer"`` it trains as a ``DeepSetsPopulation`` does, under ONE configuration (learner s is then
    ``RPOTrainer(grad_fn=transformer_kernel_grad, optimizer="device_transformer", one_call=True)`` alone; ``self.optimizer`` is a
    ``TransformerPopulationAdam``, the update ``transformer_update_population``; a dropout probability other than 0 in any
    learner is a ``ValueError``).  That value with any other population is a ``ValueError``.  ``encoder_sweep=True``: a
    ``DeepSetsPopulation`` (or, with ``optimizer="device_transformer"``, a ``TransformerPopulation``) trains under S
    configurations that may differ in ``SWEEP_FIELDS`` as a ``PolicyPopulation``'s may -- collection through
    ``policy_rollout_sweep``, ``gae`` per learner, the update ``deepsets_update_sweep`` / ``transformer_update_sweep`` -- and
    learner s is the lone trainer above with ``cfgs[s]`` on an env wrapped with its own gamma; the keyword with a
    ``PolicyPopulation`` is a ``ValueError`` (its default path already sweeps)."""

    def __init__(self, env, population, cfgs, *, optimizer: Optional[str] = None, encoder_sweep: bool = False):
        if optimizer not in (None, "device_transformer"):
            raise ValueError(f"PopulationTrainer: optimizer = {optimizer!r}: expected None or \"device_transformer\"")
        refuse_deepsets(population, "PopulationTrainer")       # (a network where the population goes)
        self.transformer = isinstance(population, TransformerPopulation)
        if self.transformer and optimizer is None:
            raise ValueError(f"PopulationTrainer: {TransformerPopulation.UPDATE_NOT_BUILT}")
        if optimizer is not None and not self.transformer:
            raise ValueError("PopulationTrainer(optimizer=\"device_transformer\") trains a TransformerPopulation; "
                             f"got {type(population).__name__}")
        self.deepsets = isinstance(population, DeepSetsPopulation)
        self.encoder_sweep = bool(encoder_sweep)
        if self.encoder_sweep and not (self.deepsets or self.transformer):
            raise ValueError("PopulationTrainer(encoder_sweep=True) is for a DeepSetsPopulation or a TransformerPopulation: with a "
                             f"{type(population).__name__} the default path already sweeps (pass the sequence of configurations)")
        for net in getattr(population, "nets", ()):
            if self.transformer:
                refuse_dropout(net, "PopulationTrainer")
            else:
                (refuse_transformer if self.deepsets else refuse_deepsets)(net, "PopulationTrainer")
        S = population.num_learners
        if (self.deepsets or self.transformer) and isinstance(cfgs, (list, tuple)) and not self.encoder_sweep:
            if len(cfgs) != S:
                raise ValueError(f"PopulationTrainer: {len(cfgs)} configurations for {S} learners")
            if any(dataclasses.replace(c, seed=cfgs[0].seed) != cfgs[0] for c in cfgs):
                kind = "transformer learners" if self.transformer else "deep-sets learners"
                raise ValueError(f"PopulationTrainer: sweeps of {kind} are not built: a {type(population).__name__} trains under "
                                 "ONE configuration (unless encoder_sweep=True is given: the sweep is opt-in)")
            cfgs = cfgs[0]
        if self.encoder_sweep and not isinstance(cfgs, (list, tuple)):
            cfgs = [cfgs] * S
        self.sweep = isinstance(cfgs, (list, tuple))
        if self.sweep:
            self.cfgs = list(cfgs)
            if len(self.cfgs) != S:
                raise ValueError(f"PopulationTrainer: {len(self.cfgs)} configurations for {S} learners")
            for c in self.cfgs:
                c.check()
            check_structure(self.cfgs, "PopulationTrainer")
        else:
            cfgs.check()
            self.cfgs = [cfgs] * S
        cfg = self.cfgs[0]
        if env.num_envs != S * cfg.num_envs:
            raise ValueError(f"PopulationTrainer: the env has {env.num_envs} envs; {S} learners x cfg.num_envs = {S * cfg.num_envs}")
        self.env, self.population, self.cfg = env, population, cfg
        self.nets, self.device = population.nets, population.device
        self.num_learners, self.envs_per_learner = S, int(cfg.num_envs)
        make_optimizer = TransformerPopulationAdam if self.transformer else PopulationAdam
        self.optimizer = make_optimizer(population, lr=[c.learning_rate for c in self.cfgs], eps=1e-5,
                                        max_grad_norm=[c.max_grad_norm for c in self.cfgs])
        self.generators = []
        for seed in population.seeds:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed))
            self.generators.append(g)
        self.learner_index = torch.arange(S, device=self.device).reshape(S, 1, 1)
        self.update_index = 0
        self.global_step = 0                      # of ONE learner, as RPOTrainer counts
        self.minibatch_steps = [0] * S            # every learner's draw counter of the RPO perturbation
        self.start_time = None
        self.storage = self.advantages = self.returns = None
        self.next_obs = self.next_done = None
        self.stats_rows = self.workspace = None
        self.last_permutations = None             # [S, epochs, B_l]: the learners' own permutations of the last update
        self.evaluator = None
        self.population_evaluator = None          # evaluate()'s: every learner in one set of launches

    def _start(self):
        obs, _ = self.env.reset()
        self.next_obs = obs.clone()
        self.next_done = torch.zeros(self.env.num_envs, dtype=torch.float32, device=self.device)
        self.start_time = time.time()

    def collect(self):
        """Every learner's collection phase (one launch) and advantages (one launch)."""
        if self.next_obs is None:
            self._start()
        if self.start_time is None:
            self.start_time = time.time()
        with torch.no_grad():
            if self.encoder_sweep:
                self.storage = self.env.policy_rollout_sweep(self.population, self.cfg.num_steps, self.next_obs, self.next_done,
                                                             [c.gamma for c in self.cfgs], out=self.storage)
            else:
                kw = {"gammas": [c.gamma for c in self.cfgs]} if self.sweep else {}
                self.storage = self.env.policy_rollout_population(self.population, self.cfg.num_steps, self.next_obs, self.next_done,
                                                                  out=self.storage, **kw)
            out = None if self.advantages is None else (self.advantages, self.returns)
            if self.sweep:
                self.advantages, self.returns = gae(self.storage, [c.gamma for c in self.cfgs], [c.gae_lambda for c in self.cfgs],
                                                    out=out, envs_per_learner=self.envs_per_learner)
            else:
                self.advantages, self.returns = gae(self.storage, self.cfg.gamma, self.cfg.gae_lambda, out=out)
        self.global_step += self.cfg.batch_size
        return self.storage

    def update(self) -> List[dict]:
        cfg, S, E_l = self.cfg, self.num_learners, self.envs_per_learner
        frac = 1.0 - self.update_index / max(1, cfg.num_updates)
        for c, opt in zip(self.cfgs, self.optimizer.learners):        # (every learner anneals its own rate, or does not)
            if c.anneal_lr:
                opt.param_groups[0]["lr"] = frac * c.learning_rate
        storage = self.collect()
        batch = flatten_batch(storage, self.advantages, self.returns)
        B_l, T = cfg.batch_size, cfg.num_steps
        perms = torch.stack([torch.stack([torch.randperm(B_l, device=self.device, generator=g) for _ in range(cfg.update_epochs)])
                             for g in self.generators])
        self.last_permutations = perms
        rows = population_rows(perms, self.learner_index, E_l, S)
        steps = cfg.update_epochs * len(update_steps(B_l, cfg.minibatch_size, cfg.norm_adv))
        if self.stats_rows is None or self.stats_rows.shape[1] != steps:
            self.stats_rows = torch.zeros(S, steps, 8, dtype=torch.float32, device=self.device)
        need = population_workspace_bytes(self.population.obs_dim, min(cfg.minibatch_size, B_l), S, deepsets=self.deepsets,
                                          transformer=self.transformer, sweep=self.encoder_sweep)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.encoder_sweep:
            update = transformer_update_sweep if self.transformer else deepsets_update_sweep
        else:
            update = (transformer_update_population if self.transformer else
                      deepsets_update_population if self.deepsets else rpo_update_population)
        stats, headers = update(self.population, batch, rows, self.cfgs if self.sweep else cfg, self.optimizer,
                                first_draw_counters=self.minibatch_steps, stats=self.stats_rows, workspace=self.workspace)
        self.update_index += 1
        # the logged scalars of every learner, over its own columns (contiguous copies: the arrays RPOTrainer reduces), ONE transfer
        ret, val = self.returns.view(T, S, E_l), storage["values"].view(T, S, E_l)
        evs, var_ys = [], []
        for s in range(S):
            y_true, y_pred = ret[:, s].reshape(-1), val[:, s].reshape(-1)
            var_y = y_true.var(unbiased=False)
            evs.append((1 - (y_true - y_pred).var(unbiased=False) / var_y).reshape(1))
            var_ys.append(var_y.reshape(1))
        host = torch.cat([headers.view(torch.float32).reshape(-1), stats.reshape(-1)] + evs + var_ys).cpu()
        hdr, rows_h = host[:16 * S].reshape(S, 16), host[16 * S:16 * S + S * steps * 8].reshape(S, steps, 8)
        tail = host[16 * S + S * steps * 8:]
        es = storage["episode_stats"]
        done = storage["dones"][1:].bool()
        ended = torch.cat([done, storage["next_done"].bool()[None]], dim=0)
        sps = int(self.global_step / max(time.time() - self.start_time, 1e-9))
        lrs = [g["lr"] for g in self.optimizer.param_groups]
        differs = [{f: getattr(c, f) for f in SWEEP_FIELDS if getattr(c, f) != getattr(cfg, f)} for c in self.cfgs]
        logs = []
        for s in range(S):
            h = decode_header(hdr[s])
            ran = h["steps_run"]
            self.minibatch_steps[s] += ran
            last, clipfrac = rows_h[s, ran - 1].tolist(), float(rows_h[s, :ran, 6].mean())
            cols = slice(s * E_l, (s + 1) * E_l)
            recs = es[:, cols][ended[:, cols]]
            ev, var_y = float(tail[s]), float(tail[S + s])
            logs.append({"update": self.update_index, "global_step": self.global_step, "learning_rate": lrs[s], "value_loss": last[2],
                         "policy_loss": last[1], "entropy": last[3], "old_approx_kl": last[4], "approx_kl": last[5],
                         "clipfrac": clipfrac, "explained_variance": float("nan") if var_y == 0 else ev, "loss": last[0], "SPS": sps,
                         "episodes": {k: recs[:, i] for i, k in enumerate(STATS_FIELDS)}, "learner": s,
                         "seed": self.population.seeds[s], "steps_run": ran, "epochs_run": h["epochs_run"], "config": differs[s]})
        return logs

    def make_evaluator(self, num_envs: Optional[int] = None):
        """One ``PolicyEvaluator`` for all learners: the training env's configs, a handle and a batch of its own (``num_envs``: a
        learner's share of the training batch by default)."""
        from .evaluation import PolicyEvaluator
        base = getattr(self.env, "env", self.env)
        n = self.envs_per_learner if num_envs is None else int(num_envs)
        if self.evaluator is None or self.evaluator.num_envs != n:
            if self.evaluator is not None:
                self.evaluator.close()
            self.evaluator = PolicyEvaluator(base.env_config, base.wrap_config, num_envs=n, seed=base.seed_value, device=base.device)
        return self.evaluator

    def make_population_evaluator(self, num_envs: Optional[int] = None):
        """One ``PopulationEvaluator`` for all learners: the training env's configs and seed, a handle of its own with
        ``num_envs`` envs per learner (a learner's share of the training batch by default)."""
        from .evaluation import PopulationEvaluator
        base = getattr(self.env, "env", self.env)
        n = self.envs_per_learner if num_envs is None else int(num_envs)
        if self.population_evaluator is None or self.population_evaluator.num_envs != n:
            if self.population_evaluator is not None:
                self.population_evaluator.close()
            self.population_evaluator = PopulationEvaluator(base.env_config, base.wrap_config, num_learners=self.num_learners,
                                                            num_envs=n, seed=base.seed_value, device=base.device)
        return self.population_evaluator

    def evaluate(self, n_episodes: int = 1, num_envs: Optional[int] = None, deterministic: bool = True) -> list:
        """``RPOTrainer.evaluate`` for every learner in ONE set of launches on the population evaluator, each with its own rows
        of the training env's observation statistics (frozen copies).  Returns S ``EvaluationResult``s, bit for bit those of
        ``make_evaluator().evaluate(nets[s], ...)`` learner by learner.  A ``DeepSetsPopulation`` likewise
        (``evac_policy_evaluate_population_deepsets``), and a ``TransformerPopulation``
        (``evac_policy_evaluate_population_transformer``)."""
        S, E_l = self.num_learners, self.envs_per_learner
        ev = self.make_population_evaluator(num_envs)
        kw = {}
        if hasattr(self.env, "norm_state"):
            kw = {"norm_state": self.env.norm_state.view(S, E_l, -1).clone(), "obs_clip": self.env.obs_clip,
                  "epsilon": self.env.epsilon}
        with torch.no_grad():
            return ev.evaluate(self.population, n_episodes, deterministic=deterministic, **kw)

    def learn(self, total_timesteps: Optional[int] = None, callback: Optional[Callable[[List[dict]], None]] = None, *,
              eval_every: Optional[int] = None, eval_episodes: int = 1) -> list:
        """``num_updates`` updates (``total_timesteps // batch_size``, per learner); returns the list of ``update()``'s results.
        Every ``eval_every`` updates each learner's ``log["eval"]`` holds the ``summary()`` of its ``evaluate(eval_episodes)``
        (``EvaluationResult.summaries``: one host transfer for all learners)."""
        from .evaluation import EvaluationResult
        n = self.cfg.num_updates if total_timesteps is None else int(total_timesteps) // self.cfg.batch_size
        all_logs = []
        for _ in range(n):
            logs = self.update()
            if eval_every and self.update_index % int(eval_every) == 0:
                for log, summary in zip(logs, EvaluationResult.summaries(self.evaluate(eval_episodes))):
                    log["eval"] = summary
            all_logs.append(logs)
            if callback is not None:
                callback(logs)
        return all_logs
