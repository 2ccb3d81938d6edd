"""The reference trainer's actor-critic for the policy rollout (``BatchedEvacuationEnv.policy_rollout``, ``evac_policy_rollout``).

``LinearActorCritic`` has the structure and attribute names of RPOLinearNetwork
(/root/reference/src/agents/networks/rpo_linear_agent_network.py:19-61): ``actor_mean`` and ``critic``, each
``Sequential(Linear, Tanh, Linear, Tanh, Linear)``, and ``actor_logstd`` [1, 2].  Any module with those names -- the
reference's own network included -- can drive the device rollout; its parameters are read by the kernel in place."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.distributions.normal import Normal

from . import _lib

HIDDEN = 64           # the only hidden width the kernel takes (RPOLinearNetworkConfig.num_hidden default)
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


class PolicyBinder:
    """``evac_mlp_policy_t`` of a network, validated once per distinct set of parameter tensors (keyed by the tensor objects and
    their addresses: parameters updated in place keep their entry; new tensors are checked again)."""

    _ENTRIES = 8

    def __init__(self, obs_dim: int, device: torch.device):
        self.obs_dim, self.device = int(obs_dim), device
        self._cache = {}

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
