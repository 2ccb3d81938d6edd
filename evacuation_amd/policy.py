"""The reference trainer's actor-critic for the policy rollout (``BatchedEvacuationEnv.policy_rollout``, ``evac_policy_rollout``).

``LinearActorCritic`` has the structure and attribute names of RPOLinearNetwork
(/root/reference/src/agents/networks/rpo_linear_agent_network.py:19-61): ``actor_mean`` and ``critic``, each
``Sequential(Linear, Tanh, Linear, Tanh, Linear)``, and ``actor_logstd`` [1, 2].  Any module with those names -- the
reference's own network included -- can drive the device rollout; its parameters are read by the kernel in place.

``DeepSetsActorCritic`` is RPODeepSetsEmbedding (/root/reference/src/agents/networks/rpo_deep_sets_agent_network.py:25-90): the
same actor-critic behind a set encoder ``deep_sets`` (``transform_phi``, ``transform_rho``) that reads the Box observation as
``N + 2`` rows.  A module with those names routes to ``evac_policy_rollout_deepsets`` / ``evac_policy_evaluate_deepsets``."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import nn
from torch.distributions.normal import Normal

from . import _lib

HIDDEN = 64           # the only hidden width the kernel takes (RPOLinearNetworkConfig.num_hidden default)
SET_HIDDEN = 24       # ... and the only width of the set encoder (RPODeepSetsEmbeddingConfig.dim_hidden default)
SET_MAX_ELEM_DIM = 6  # positions + one-hot status
MAX_PEDESTRIANS = 64  # one wave per env


def layer_init(layer: nn.Linear, std: float = float(np.sqrt(2)), bias_const: float = 0.0) -> nn.Linear:
    """The reference's initialisation (src/agents/networks/utils.py:4-7)."""
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class LinearActorCritic(nn.Module):
    """RPOLinearNetwork without the env argument: ``LinearActorCritic(obs_dim, hidden=64)``."""

    def __init__(self, obs_dim: int, hidden: int = HIDDEN, action_dim: int = 2):
        super().__init__()
        self.critic = nn.Sequential(layer_init(nn.Linear(obs_dim, hidden)), nn.Tanh(), layer_init(nn.Linear(hidden, hidden)), nn.Tanh(),
                                    layer_init(nn.Linear(hidden, 1), std=1.0))
        self.actor_mean = nn.Sequential(layer_init(nn.Linear(obs_dim, hidden)), nn.Tanh(), layer_init(nn.Linear(hidden, hidden)), nn.Tanh(),
                                        layer_init(nn.Linear(hidden, action_dim), std=0.01))
        self.actor_logstd = nn.Parameter(torch.zeros(1, action_dim))

    def get_value(self, x):
        return self.critic(x)

    def get_action_and_value(self, x, action=None):
        mean = self.actor_mean(x)
        std = torch.exp(self.actor_logstd.expand_as(mean))
        probs = Normal(mean, std)
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action).sum(1), probs.entropy().sum(1), self.critic(x)


class DeepSets(nn.Module):
    """The reference's DeepSets: ``transform_rho(sum_i transform_phi(x_i))`` of x [batch, set_size, set_elem_dim].  torch's
    default ``nn.Linear`` initialisation, as the reference's (not ``layer_init``)."""

    def __init__(self, set_elem_dim: int, output_dim: int, hidden_dim: int):
        super().__init__()
        self.transform_phi = nn.Sequential(nn.Linear(set_elem_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim))
        self.transform_rho = nn.Sequential(nn.Linear(hidden_dim, output_dim))

    def forward(self, x):
        if x.dim() != 3 or x.shape[1] < 2:
            raise ValueError(f"DeepSets: expected [batch, set_size > 1, set_elem_dim], got {tuple(x.shape)}")
        return self.transform_rho(self.transform_phi(x).sum(dim=-2))


class DeepSetsActorCritic(LinearActorCritic):
    """RPODeepSetsEmbedding without the env argument: ``DeepSetsActorCritic(obs_dim, number_of_pedestrians, dim_hidden=24)``.
    One encoder serves actor and critic; ``encode(x)`` is what they read."""

    def __init__(self, obs_dim: int, number_of_pedestrians: int, dim_hidden: int = SET_HIDDEN, hidden: int = HIDDEN, action_dim: int = 2):
        super().__init__(obs_dim, hidden, action_dim)
        elements = int(number_of_pedestrians) + 2
        if int(obs_dim) % elements:
            raise ValueError(f"DeepSetsActorCritic: an observation of {obs_dim} floats is not a whole number of floats for each of "
                             f"the {elements} elements ({number_of_pedestrians} pedestrians, the leader, the exit): a Box observation is needed")
        self.set_element_dim = int(obs_dim) // elements
        self.deep_sets = DeepSets(self.set_element_dim, int(obs_dim), int(dim_hidden))

    def encode(self, x):
        return encode_observation(self, x)

    def get_value(self, x):
        return super().get_value(self.encode(x))

    def get_action_and_value(self, x, action=None):
        return super().get_action_and_value(self.encode(x), action)


def is_deepsets(net) -> bool:
    return hasattr(net, "deep_sets")


def encode_observation(net, x):
    """What ``actor_mean`` / ``critic`` of ``net`` read for the observations x [B, D]: x itself, or -- with a set encoder --
    ``deep_sets`` of x as [B, D / set_elem_dim, set_elem_dim] (rpo_deep_sets_agent_network.py:76-90)."""
    if not is_deepsets(net):
        return x
    ed = net.deep_sets.transform_phi[0].in_features
    return net.deep_sets(x.view(x.shape[0], -1, ed)).view(x.shape)


def deepsets_tensors(net) -> tuple:
    """The 6 parameter tensors of the set encoder of ``net`` in ``evac_deepsets_t`` order."""
    phi, rho = net.deep_sets.transform_phi, net.deep_sets.transform_rho
    return (phi[0].weight, phi[0].bias, phi[2].weight, phi[2].bias, rho[0].weight, rho[0].bias)


def all_tensors(net) -> tuple:
    """Every parameter tensor the device reads: the actor-critic's 13, then the set encoder's 6 if ``net`` has one."""
    return mlp_tensors(net) + (deepsets_tensors(net) if is_deepsets(net) else ())


def refuse_deepsets(net, what: str) -> None:
    """``ValueError`` where only the linear network can go: the linear entries (``rpo_minibatch_grad`` .. ``rpo_update``),
    populations, sweeps, and ``RPOTrainer(optimizer="device")`` with the gradient left at its default, which for such a network
    is autograd's.  (Its own device entries are ``trainer.deepsets_minibatch_grad`` / ``deepsets_minibatch_step`` /
    ``deepsets_update`` and ``DeviceAdam``: ``RPOTrainer(grad_fn=deepsets_kernel_grad, optimizer="device")``.)"""
    if net is not None and is_deepsets(net):
        raise ValueError(f"{what}: the network has a set encoder (`deep_sets`); the gradient and optimiser kernels are the linear "
                         "network's -- train it with RPOTrainer(optimizer=\"torch\"), whose gradient is autograd's")


def mlp_tensors(net) -> tuple:
    """The 13 parameter tensors of ``net`` in ``evac_mlp_policy_t`` order."""
    a, c = net.actor_mean, net.critic
    return (a[0].weight, a[0].bias, a[2].weight, a[2].bias, a[4].weight, a[4].bias, net.actor_logstd,
            c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias)


def _check_structure(net, obs_dim: int, device: torch.device) -> None:
    for name in ("actor_mean", "critic", "actor_logstd"):
        if not hasattr(net, name):
            raise ValueError(f"policy: the network has no `{name}` (expected RPOLinearNetwork's attribute names)")
    for name, out in (("actor_mean", 2), ("critic", 1)):
        seq = getattr(net, name)
        kinds = (nn.Linear, nn.Tanh, nn.Linear, nn.Tanh, nn.Linear)
        if not isinstance(seq, nn.Sequential) or len(seq) != 5 or not all(isinstance(m, k) for m, k in zip(seq, kinds)):
            raise ValueError(f"policy: `{name}` must be Sequential(Linear, Tanh, Linear, Tanh, Linear)")
        hidden = seq[0].out_features
        if hidden != HIDDEN:
            raise ValueError(f"policy: `{name}` has hidden width {hidden}; the device rollout takes {HIDDEN}")
        shapes = ((hidden, obs_dim), (hidden,), (hidden, hidden), (hidden,), (out, hidden), (out,))
        got = (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias)
        for t, s in zip(got, shapes):
            if t is None or tuple(t.shape) != s:
                raise ValueError(f"policy: `{name}` parameter of shape {None if t is None else tuple(t.shape)}, expected {s} "
                                 f"(observation dim {obs_dim})")
    if tuple(net.actor_logstd.shape) != (1, 2):
        raise ValueError(f"policy: actor_logstd of shape {tuple(net.actor_logstd.shape)}, expected (1, 2)")
    for t in mlp_tensors(net):
        if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
            raise ValueError(f"policy: parameters must be contiguous float32 tensors on {device}, got {t.dtype} on {t.device}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")


_ENCODER_NAMES = ("deep_sets.transform_phi[0].weight", "deep_sets.transform_phi[0].bias", "deep_sets.transform_phi[2].weight",
                  "deep_sets.transform_phi[2].bias", "deep_sets.transform_rho[0].weight", "deep_sets.transform_rho[0].bias")


def _check_encoder(net, obs_dim: int, device: torch.device, n_ped: Optional[int] = None) -> int:
    """The set encoder of ``net`` against the observation; returns ``set_elem_dim``."""
    ds = net.deep_sets
    for name, kinds in (("transform_phi", (nn.Linear, nn.ReLU, nn.Linear)), ("transform_rho", (nn.Linear,))):
        seq = getattr(ds, name, None)
        if not isinstance(seq, nn.Sequential) or len(seq) != len(kinds) or not all(isinstance(m, k) for m, k in zip(seq, kinds)):
            raise ValueError(f"policy: `deep_sets.{name}` must be Sequential({', '.join(k.__name__ for k in kinds)})")
    phi, rho = ds.transform_phi, ds.transform_rho
    width = phi[0].out_features
    if width != SET_HIDDEN:
        raise ValueError(f"policy: `deep_sets` has dim_hidden {width}; the device kernels take {SET_HIDDEN}")
    ed = phi[0].in_features
    if ed < 1 or ed > SET_MAX_ELEM_DIM or obs_dim % ed or (n_ped is not None and ed * (n_ped + 2) != obs_dim) or \
            getattr(net, "set_element_dim", ed) != ed:
        rows = "" if n_ped is None else f" of {n_ped} + 2 elements"
        raise ValueError(f"policy: the observation's {obs_dim} floats are not a whole number of rows of `deep_sets`' {ed} floats per "
                         f"element{rows} (a Box observation is needed)")
    shapes = ((width, ed), (width,), (width, width), (width,), (obs_dim, width), (obs_dim,))
    for name, t, shape in zip(_ENCODER_NAMES, deepsets_tensors(net), shapes):
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"policy: `{name}` of shape {None if t is None else tuple(t.shape)}, expected {shape} "
                             f"(observation dim {obs_dim})")
        if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
            raise ValueError(f"policy: `{name}` must be a contiguous float32 tensor on {device}, got {t.dtype} on {t.device}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    if deepsets_tensors(net)[4].data_ptr() % 16:
        raise ValueError(f"policy: `{_ENCODER_NAMES[4]}` must be 16-byte aligned (its rows are read as vectors)")
    return ed


class PolicyBinder:
    """``evac_mlp_policy_t`` of a network, validated once per distinct set of parameter tensors (keyed by the tensor objects and
    their addresses: parameters updated in place keep their entry; new tensors are checked again)."""

    _ENTRIES = 8

    def __init__(self, obs_dim: int, device: torch.device, n_ped: Optional[int] = None):
        self.obs_dim, self.device, self.n_ped = int(obs_dim), device, n_ped
        self._cache = {}
        self._encoders = {}

    def __call__(self, net) -> _lib.EvacMlpPolicy:
        try:
            ts = mlp_tensors(net)
        except (AttributeError, IndexError, TypeError):
            _check_structure(net, self.obs_dim, self.device)
            raise
        key = tuple((id(t), t.data_ptr()) for t in ts)
        ent = self._cache.get(key)
        if ent is not None:
            return ent[0]
        _check_structure(net, self.obs_dim, self.device)
        st = _lib.EvacMlpPolicy(self.obs_dim, HIDDEN, *[t.data_ptr() for t in ts])
        if len(self._cache) >= self._ENTRIES:
            self._cache.pop(next(iter(self._cache)))
        self._cache[key] = (st, ts)      # (the tensors stay referenced: their ids cannot be reused while the entry exists)
        return st

    def encoder(self, net) -> _lib.EvacDeepSets:
        """``evac_deepsets_t`` of the set encoder of ``net`` (``is_deepsets``): cached and validated as the 13 tensors are."""
        try:
            ts = deepsets_tensors(net)
        except (AttributeError, IndexError, TypeError):
            _check_encoder(net, self.obs_dim, self.device, self.n_ped)
            raise
        key = tuple((id(t), t.data_ptr()) for t in ts)
        ent = self._encoders.get(key)
        if ent is not None:
            return ent[0]
        ed = _check_encoder(net, self.obs_dim, self.device, self.n_ped)
        st = _lib.EvacDeepSets(ed, SET_HIDDEN, *[t.data_ptr() for t in ts])
        if len(self._encoders) >= self._ENTRIES:
            self._encoders.pop(next(iter(self._encoders)))
        self._encoders[key] = (st, ts)
        return st
