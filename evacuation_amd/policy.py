"""The reference trainer's actor-critic for the policy rollout (``BatchedEvacuationEnv.policy_rollout``, ``evac_policy_rollout``).

``LinearActorCritic`` has the structure and attribute names of RPOLinearNetwork
(/root/reference/src/agents/networks/rpo_linear_agent_network.py:19-61): ``actor_mean`` and ``critic``, each
``Sequential(Linear, Tanh, Linear, Tanh, Linear)``, and ``actor_logstd`` [1, 2].  Any module with those names -- the
reference's own network included -- can drive the device rollout; its parameters are read by the kernel in place.

``DeepSetsActorCritic`` is RPODeepSetsEmbedding (/root/reference/src/agents/networks/rpo_deep_sets_agent_network.py:25-90): the
same actor-critic behind a set encoder ``deep_sets`` (``transform_phi``, ``transform_rho``) that reads the Box observation as
``N + 2`` rows.  A module with those names routes to ``evac_policy_rollout_deepsets`` / ``evac_policy_evaluate_deepsets``.

``TransformerActorCritic`` is RPOTransformerEmbedding (src/agents/networks/rpo_transformer_agent_network.py): the same
actor-critic behind ``embedding``, a ``Sequential`` of attention blocks over the ``N + 2`` tokens of the Box observation.  A
module with that attribute routes to ``evac_policy_rollout_transformer`` / ``evac_policy_evaluate_transformer``, which compute
its EVAL-MODE function (dropout the identity): collection and training refuse a dropout probability other than 0."""
from __future__ import annotations

from collections import namedtuple
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
TF_HEADS = 3          # the only head count, feed-forward width and LayerNorm eps of the attention encoder the kernels take
TF_FEEDFORWARD = 96   # (RPOTransformerEmbeddingConfig's defaults, nn.LayerNorm's default)
TF_LN_EPS = 1e-5
TF_MAX_BLOCKS = 2
TF_MAX_PEDESTRIANS = 62   # one wave holds the N + 2 tokens


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


class MultiHeadAttention(nn.Module):
    """The reference's attention over x [batch, tokens, d_model]: ``Wq``, ``Wk``, ``Wv`` map a token to ``num_heads * d_model``
    values, read as [heads, d_model] and permuted to [batch, d_model, tokens, heads] -- so the scores are taken per CHANNEL and
    contracted over the heads, and ``dense`` reads the result flattened as channel * heads + head.  Restated as it is."""

    def __init__(self, d_model: int, num_heads: int = TF_HEADS):
        super().__init__()
        self.d_model, self.num_heads, self.scale = int(d_model), int(num_heads), float(np.sqrt(d_model))
        self.Wq = nn.Linear(self.d_model, self.d_model * self.num_heads)
        self.Wk = nn.Linear(self.d_model, self.d_model * self.num_heads)
        self.Wv = nn.Linear(self.d_model, self.d_model * self.num_heads)
        self.dense = nn.Linear(self.d_model * self.num_heads, self.d_model)

    def _by_channel(self, t):
        return t.view(t.shape[0], -1, self.num_heads, self.d_model).permute(0, 3, 1, 2)      # [batch, d_model, tokens, heads]

    def forward(self, x):
        if x.dim() != 3:
            raise ValueError(f"MultiHeadAttention: expected [batch, tokens, d_model], got {tuple(x.shape)}")
        q, k, v = self._by_channel(self.Wq(x)), self._by_channel(self.Wk(x)), self._by_channel(self.Wv(x))
        weights = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) / self.scale, dim=-1)   # [batch, d_model, tokens, tokens]
        out = torch.matmul(weights, v).transpose(1, 2).contiguous().flatten(-2, -1)           # [batch, tokens, d_model * heads]
        return self.dense(out)


class TransformerBlock(nn.Module):
    """One block of the reference's encoder: attention, ``norm1``, the feed-forward ``ff`` (Linear, Dropout, ReLU, Linear),
    ``norm2``; with ``use_resid`` each norm reads its input plus the sublayer's output, otherwise the output alone.  Takes the
    observation flat [batch, tokens * d_model] or as tokens, and returns the shape it was given."""

    def __init__(self, d_model: int, num_heads: int = TF_HEADS, d_ff: int = TF_FEEDFORWARD, dropout: float = 0.0, use_resid: bool = False):
        super().__init__()
        self.d_model, self.num_heads, self.use_resid = int(d_model), int(num_heads), bool(use_resid)
        self.attention = MultiHeadAttention(self.d_model, self.num_heads)
        self.ff = nn.Sequential(nn.Linear(self.d_model, int(d_ff)), nn.Dropout(dropout), nn.ReLU(), nn.Linear(int(d_ff), self.d_model))
        self.norm1 = nn.LayerNorm(self.d_model)
        self.norm2 = nn.LayerNorm(self.d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        shape = x.shape
        if x.dim() == 2:
            x = x.view(shape[0], -1, self.d_model)
        a = self.dropout(self.attention(x))
        x = self.norm1(x + a if self.use_resid else a)
        f = self.dropout(self.ff(x))
        x = self.norm2(x + f if self.use_resid else f)
        return x.view(shape)


class TransformerActorCritic(LinearActorCritic):
    """RPOTransformerEmbedding without the env argument.  ``dropout`` defaults to 0 (the reference's 0.1 is drawn from torch's
    generator in its collection and its update alike; the device computes the eval-mode function, so collection and training
    take p = 0 only).  One encoder serves actor and critic; ``encode(x)`` is what they read."""

    def __init__(self, obs_dim: int, number_of_pedestrians: int, num_blocks: int = 2, num_heads: int = TF_HEADS,
                 dim_feedforward: int = TF_FEEDFORWARD, dropout: float = 0.0, use_resid: bool = False, hidden: int = HIDDEN,
                 action_dim: int = 2):
        super().__init__(obs_dim, hidden, action_dim)
        tokens = int(number_of_pedestrians) + 2
        if int(obs_dim) % tokens:
            raise ValueError(f"TransformerActorCritic: an observation of {obs_dim} floats is not a whole number of floats for each of "
                             f"the {tokens} tokens ({number_of_pedestrians} pedestrians, the leader, the exit): a Box observation is needed")
        self.token_dim = int(obs_dim) // tokens
        self.embedding = nn.Sequential(*[TransformerBlock(self.token_dim, num_heads, dim_feedforward, dropout, use_resid)
                                         for _ in range(int(num_blocks))])

    def encode(self, x):
        return encode_observation(self, x)

    def get_value(self, x):
        return super().get_value(self.encode(x))

    def get_action_and_value(self, x, action=None):
        return super().get_action_and_value(self.encode(x), action)


def is_deepsets(net) -> bool:
    return hasattr(net, "deep_sets")


def is_transformer(net) -> bool:
    return hasattr(net, "embedding")


def encoder_kind(net):
    """The row of ``ENCODER_KINDS`` (below, with what its rows name) of the encoder in front of ``net``'s actor-critic, or None
    for the linear network.  The table's order is the precedence: a module with both attributes is read by ``embedding``."""
    return next((kind for kind in ENCODER_KINDS if hasattr(net, kind.attr)), None)


def encode_observation(net, x):
    """What ``actor_mean`` / ``critic`` of ``net`` read for the observations x [B, D]: x itself, or -- with a set encoder --
    ``deep_sets`` of x as [B, D / set_elem_dim, set_elem_dim] (rpo_deep_sets_agent_network.py:76-90); with an attention encoder
    ``embedding`` of x (its blocks take the flat observation)."""
    kind = encoder_kind(net)
    if kind is None:
        return x
    if kind is _TRANSFORMER:
        return net.embedding(x)
    ed = net.deep_sets.transform_phi[0].in_features
    return net.deep_sets(x.view(x.shape[0], -1, ed)).view(x.shape)


def deepsets_tensors(net) -> tuple:
    """The 6 parameter tensors of the set encoder of ``net`` in ``evac_deepsets_t`` order."""
    phi, rho = net.deep_sets.transform_phi, net.deep_sets.transform_rho
    return (phi[0].weight, phi[0].bias, phi[2].weight, phi[2].bias, rho[0].weight, rho[0].bias)


_BLOCK_TENSORS = ("attention.Wq.weight", "attention.Wq.bias", "attention.Wk.weight", "attention.Wk.bias", "attention.Wv.weight",
                  "attention.Wv.bias", "attention.dense.weight", "attention.dense.bias", "ff[0].weight", "ff[0].bias", "ff[3].weight",
                  "ff[3].bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def _block_tensors(blk) -> tuple:
    at = blk.attention
    return (at.Wq.weight, at.Wq.bias, at.Wk.weight, at.Wk.bias, at.Wv.weight, at.Wv.bias, at.dense.weight, at.dense.bias,
            blk.ff[0].weight, blk.ff[0].bias, blk.ff[3].weight, blk.ff[3].bias, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight,
            blk.norm2.bias)


def transformer_tensors(net) -> tuple:
    """The parameter tensors of the attention encoder of ``net``: 16 per block in ``evac_transformer_block_t`` order, block by
    block."""
    return tuple(t for blk in net.embedding for t in _block_tensors(blk))


def all_tensors(net) -> tuple:
    """Every parameter tensor the device reads: the actor-critic's 13, then the set encoder's 6 or the attention encoder's 16 per
    block if ``net`` has one."""
    kind = encoder_kind(net)
    return mlp_tensors(net) + (() if kind is None else kind.tensors(net))


def transformer_dropouts(net) -> list:
    """The probabilities of every ``nn.Dropout`` inside ``embedding``."""
    return [float(m.p) for m in net.embedding.modules() if isinstance(m, nn.Dropout)]


def refuse_transformer(net, what: str) -> None:
    """``ValueError`` where a network with an attention encoder cannot go: the gradient and optimiser entries of the linear
    network and of the set encoder, ``DeviceAdam``, sweeps, and populations -- but for ``population.TransformerPopulation``, which
    the entries that run learners on a handle's envs take.  It trains with ``RPOTrainer(optimizer="torch")``,
    whose gradient for such a network is autograd's, or with its own entries (``trainer.transformer_minibatch_grad`` /
    ``transformer_minibatch_step`` / ``transformer_update`` and ``TransformerAdam``:
    ``RPOTrainer(grad_fn=transformer_kernel_grad, optimizer="device_transformer")``)."""
    if net is not None and is_transformer(net):
        raise ValueError(f"{what}: the network has an attention encoder (`embedding`); these gradient and optimiser kernels do not "
                         "know its tensors -- train it with RPOTrainer(optimizer=\"torch\"), whose gradient is autograd's, or with "
                         "RPOTrainer(grad_fn=transformer_kernel_grad, optimizer=\"device_transformer\")")


def refuse_dropout(net, what: str) -> None:
    """``ValueError`` for an attention encoder with a dropout probability other than 0 where the device's eval-mode forward pass
    would disagree with the module's own (collection against the autograd update)."""
    if net is not None and is_transformer(net) and any(p != 0.0 for p in transformer_dropouts(net)):
        raise ValueError(f"{what}: `embedding` has dropout p = {max(transformer_dropouts(net))}; the device computes the eval-mode "
                         "function (no dropout masks), so collection and training take p = 0 only (evaluation takes any p)")


def refuse_deepsets(net, what: str) -> None:
    """``ValueError`` where only the linear network can go: the linear entries (``rpo_minibatch_grad`` .. ``rpo_update``),
    populations, sweeps, and ``RPOTrainer(optimizer="device")`` with the gradient left at its default, which for such a network
    is autograd's.  (Its own device entries are ``trainer.deepsets_minibatch_grad`` / ``deepsets_minibatch_step`` /
    ``deepsets_update`` and ``DeviceAdam``: ``RPOTrainer(grad_fn=deepsets_kernel_grad, optimizer="device")``.)  A network with
    an attention encoder (`embedding`) is refused in all the same places (``refuse_transformer``)."""
    refuse_transformer(net, what)
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


def _check_tensors(names, tensors, shapes, device: torch.device, shape_note: str = "") -> None:
    """``shape_note`` ends the message of a wrong shape (the set encoder's names the observation)."""
    for name, t, shape in zip(names, tensors, shapes):
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"policy: `{name}` of shape {None if t is None else tuple(t.shape)}, expected {shape}{shape_note}")
        if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
            raise ValueError(f"policy: `{name}` must be a contiguous float32 tensor on {device}, got {t.dtype} on {t.device}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")


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
    _check_tensors(_ENCODER_NAMES, deepsets_tensors(net), shapes, device, f" (observation dim {obs_dim})")
    if deepsets_tensors(net)[4].data_ptr() % 16:
        raise ValueError(f"policy: `{_ENCODER_NAMES[4]}` must be 16-byte aligned (its rows are read as vectors)")
    return ed


def _check_transformer(net, obs_dim: int, device: torch.device, n_ped: Optional[int] = None) -> tuple:
    """The attention encoder of ``net`` against the observation and what the kernels take; returns (token width, blocks,
    use_resid)."""
    emb = net.embedding
    if not isinstance(emb, (nn.Sequential, nn.ModuleList)) or len(emb) < 1:
        raise ValueError("policy: `embedding` must be a Sequential of transformer blocks")
    if len(emb) > TF_MAX_BLOCKS:
        raise ValueError(f"policy: `embedding` has num_blocks {len(emb)}; the device kernels take 1 to {TF_MAX_BLOCKS}")
    if n_ped is not None and n_ped > TF_MAX_PEDESTRIANS:
        raise ValueError(f"policy: `embedding` over N = {n_ped} pedestrians: one wave holds the N + 2 tokens, so the device kernels take "
                         f"N <= {TF_MAX_PEDESTRIANS}")
    dm, resid = None, None
    for b, blk in enumerate(emb):
        where = f"embedding[{b}]"
        try:
            ts = _block_tensors(blk)
            at, norms = blk.attention, (blk.norm1, blk.norm2)
        except (AttributeError, IndexError, TypeError):
            raise ValueError(f"policy: `{where}` must have the reference's `attention.Wq/Wk/Wv/dense`, `ff[0]`, `ff[3]`, `norm1`, "
                             "`norm2`") from None
        d = int(at.Wq.in_features)
        heads = int(getattr(at, "num_heads", at.Wq.out_features // max(d, 1)))
        if heads != TF_HEADS or at.Wq.out_features != TF_HEADS * d:
            raise ValueError(f"policy: `{where}.attention` has num_heads {heads}; the device kernels take {TF_HEADS}")
        if blk.ff[0].out_features != TF_FEEDFORWARD:
            raise ValueError(f"policy: `{where}.ff` has dim_feedforward {blk.ff[0].out_features}; the device kernels take {TF_FEEDFORWARD}")
        for name, nm in zip(("norm1", "norm2"), norms):
            if not isinstance(nm, nn.LayerNorm) or not nm.elementwise_affine or nm.weight is None or nm.bias is None:
                raise ValueError(f"policy: `{where}.{name}` must be an affine LayerNorm")
            if np.float32(nm.eps) != np.float32(TF_LN_EPS):
                raise ValueError(f"policy: `{where}.{name}` has eps {nm.eps}; the device kernels take {TF_LN_EPS}")
        if dm is None:
            dm, resid = d, bool(getattr(blk, "use_resid", False))
        if d != dm or bool(getattr(blk, "use_resid", False)) != resid:
            raise ValueError(f"policy: `{where}` has d_model {d}, use_resid {bool(getattr(blk, 'use_resid', False))}; "
                             f"`embedding[0]` has {dm}, {resid}")
        if d < 1 or d > SET_MAX_ELEM_DIM or obs_dim % d or (n_ped is not None and d * (n_ped + 2) != obs_dim):
            rows = "" if n_ped is None else f" of {n_ped} + 2 tokens"
            raise ValueError(f"policy: the observation's {obs_dim} floats are not a whole number of rows of `embedding`'s {d} floats per "
                             f"token{rows} (a Box observation is needed)")
        shapes = ((3 * d, d), (3 * d,)) * 3 + ((d, 3 * d), (d,), (TF_FEEDFORWARD, d), (TF_FEEDFORWARD,), (d, TF_FEEDFORWARD), (d,)) + ((d,),) * 4
        _check_tensors([f"{where}.{name}" for name in _BLOCK_TENSORS], ts, shapes, device)
    return dm, len(emb), resid


def _transformer_struct(found, ts) -> _lib.EvacTransformer:
    dm, blocks, resid = found
    st = _lib.EvacTransformer(dm, blocks, TF_HEADS, TF_FEEDFORWARD, int(resid), TF_LN_EPS)
    for b in range(blocks):
        st.blocks[b] = _lib.EvacTransformerBlock(*[t.data_ptr() for t in ts[16 * b:16 * b + 16]])
    return st


def _transformer_grads(*ptrs) -> _lib.EvacTransformerGrads:
    """``evac_transformer_grads_t`` of 16 addresses per block (the blocks the network does not have stay NULL: they are never
    followed)."""
    st = _lib.EvacTransformerGrads()
    for b in range(len(ptrs) // 16):
        st.blocks[b] = _lib.EvacTransformerBlockGrads(*ptrs[16 * b:16 * b + 16])
    return st


# One kind of encoder in front of the actor-critic: the attribute that marks such a network, the suffix of its C entries
# (evac_policy_rollout + suffix, evac_policy_evaluate + suffix; "evac" + suffix + _workspace_bytes, _minibatch_grad), its
# parameter tensors in its struct's order, check(net, obs_dim, device, n_ped) -> what struct(found, tensors) builds the C struct
# from, what a binder's key holds beside the tensors (None: nothing; `use_resid` is no tensor, so it is read at every call), and
# grads(*addresses of the tensors' .grad) -> the C struct of its gradients.  The kinds in order of precedence.
EncoderKind = namedtuple("EncoderKind", "attr suffix tensors check struct key grads")
ENCODER_KINDS = (
    EncoderKind("embedding", "_transformer", transformer_tensors, _check_transformer, _transformer_struct,
                lambda net: tuple(bool(getattr(b, "use_resid", False)) for b in net.embedding), _transformer_grads),
    EncoderKind("deep_sets", "_deepsets", deepsets_tensors, _check_encoder,
                lambda ed, ts: _lib.EvacDeepSets(ed, SET_HIDDEN, *[t.data_ptr() for t in ts]), None, _lib.EvacDeepSetsGrads))
_TRANSFORMER, _DEEP_SETS = ENCODER_KINDS


class PolicyBinder:
    """``evac_mlp_policy_t`` of a network, validated once per distinct set of parameter tensors (keyed by the tensor objects and
    their addresses: parameters updated in place keep their entry; new tensors are checked again), and its encoder's struct
    likewise: the policies' dictionary, and one for the encoders of every kind (6 pairs, or 16 per block and a tuple of bools)."""

    _ENTRIES = 8

    def __init__(self, obs_dim: int, device: torch.device, n_ped: Optional[int] = None):
        self.obs_dim, self.device, self.n_ped = int(obs_dim), device, n_ped
        self._cache = {}
        self._encoders = {}

    def _bound(self, cache, net, tensors, check, struct, key=None):
        """The cached struct of ``tensors(net)``, or after ``check()`` a new one, in place of the oldest of ``_ENTRIES``."""
        try:
            ts = tensors(net)
        except (AttributeError, IndexError, TypeError):
            check()             # (the check's own message, where it has one)
            raise
        k = tuple((id(t), t.data_ptr()) for t in ts) + (() if key is None else (key(net),))
        ent = cache.get(k)
        if ent is not None:
            return ent[0]
        st = struct(check(), ts)
        if len(cache) >= self._ENTRIES:
            cache.pop(next(iter(cache)))
        cache[k] = (st, ts)      # (the tensors stay referenced: their ids cannot be reused while the entry exists)
        return st

    def __call__(self, net) -> _lib.EvacMlpPolicy:
        return self._bound(self._cache, net, mlp_tensors, lambda: _check_structure(net, self.obs_dim, self.device),
                           lambda _, ts: _lib.EvacMlpPolicy(self.obs_dim, HIDDEN, *[t.data_ptr() for t in ts]))

    def _bind(self, kind: EncoderKind, net):
        return self._bound(self._encoders, net, kind.tensors, lambda: kind.check(net, self.obs_dim, self.device, self.n_ped),
                           kind.struct, kind.key)

    def encoder(self, net) -> _lib.EvacDeepSets:
        """``evac_deepsets_t`` of the set encoder of ``net`` (``is_deepsets``): cached and validated as the 13 tensors are."""
        return self._bind(_DEEP_SETS, net)

    def transformer(self, net) -> _lib.EvacTransformer:
        """``evac_transformer_t`` of the attention encoder of ``net`` (``is_transformer``): cached and validated as the 13
        tensors are (``use_resid`` is read at every call: it is no tensor)."""
        return self._bind(_TRANSFORMER, net)

    def bind_encoder(self, net) -> Optional[tuple]:
        """(the C entries' suffix, the encoder's struct) for ``encoder_kind(net)``, or None for the linear network."""
        kind = encoder_kind(net)
        return None if kind is None else (kind.suffix, self._bind(kind, net))
