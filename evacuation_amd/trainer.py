"""The reference trainer's update on the device: the other half of ``RPOAgent.learn()`` (src/agents/rpo_agent.py:172-299).

``policy_rollout`` fills the trainer's storage in one launch; this module does what the reference does with it afterwards:
``gae`` (rpo_agent.py:205-220, ``evac_gae``: one launch), ``rpo_minibatch_grad`` (rpo_agent.py:239-277 up to and including
``loss.backward()``, ``evac_rpo_minibatch_grad``: at most three launches, deterministic) and ``RPOTrainer``, one iteration of the
reference's loop per ``update()``.  Gradient clipping and Adam are torch's by default (they work on ``.grad`` in place) or the
library's own (``DeviceAdam``, ``evac_adam_step``: one launch), with which a minibatch step is one host call
(``rpo_minibatch_step``) and a whole update's epochs and minibatches are one (``rpo_update``), ``target_kl`` included.  The
deep-sets and the transformer leader have the same three forms for their 19 and 13 + 16 per block tensors (``deepsets_*``;
``transformer_*`` with ``TransformerAdam``)."""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch

from . import _lib
from .policy import (PolicyBinder, all_tensors, encode_observation, encoder_kind, is_deepsets, is_transformer, mlp_tensors,
                     refuse_deepsets, refuse_dropout, refuse_transformer)
from .vector_env import STATS_FIELDS, _ptr

STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_sumsq")
BATCH_KEYS = ("b_obs", "b_actions", "b_logprobs", "b_advantages", "b_returns", "b_values")


@dataclass
class RPOTrainingConfig:
    """RPOAgentTrainingConfig (rpo_agent.py:41-104) and ``rpo_alpha`` of RPOLinearNetworkConfig: same names and defaults."""
    exp_name: str = "rpo-agent"
    seed: int = 1
    torch_deterministic: bool = True
    cuda: bool = True
    total_timesteps: int = 80000000
    learning_rate: float = 3e-4
    num_envs: int = 3
    num_steps: int = 2048
    anneal_lr: bool = True
    gamma: float = 0.99
    gae_lambda: float = 0.95
    num_minibatches: int = 32
    update_epochs: int = 10
    norm_adv: bool = True
    clip_coef: float = 0.2
    clip_vloss: bool = True
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    target_kl: Optional[float] = None
    rpo_alpha: float = 0.5           # RPOLinearNetworkConfig.rpo_alpha (rpo_linear_agent_network.py:14)

    @property
    def batch_size(self) -> int:
        return int(self.num_envs * self.num_steps)

    @property
    def minibatch_size(self) -> int:
        return int(self.batch_size // self.num_minibatches)

    @property
    def num_updates(self) -> int:
        return self.total_timesteps // self.batch_size

    num_iterations = num_updates

    def check(self) -> None:
        """What the device update needs of the settings (the reference checks nothing and fails later)."""
        if self.num_envs < 1 or self.num_steps < 1 or self.num_minibatches < 1 or self.update_epochs < 1:
            raise ValueError("RPOTrainingConfig: num_envs, num_steps, num_minibatches and update_epochs must be >= 1")
        if self.minibatch_size < (2 if self.norm_adv else 1):
            raise ValueError(f"RPOTrainingConfig: minibatch_size = {self.minibatch_size}: norm_adv needs at least 2 samples "
                             "(the unbiased std of one sample does not exist)")
        if self.rpo_alpha < 0 or self.clip_coef < 0:
            raise ValueError("RPOTrainingConfig: rpo_alpha and clip_coef must be >= 0")

    def loss_config(self) -> "_lib.EvacRpoLossConfig":
        return _lib.EvacRpoLossConfig(float(self.clip_coef), float(self.ent_coef), float(self.vf_coef), float(self.rpo_alpha),
                                      int(bool(self.norm_adv)), int(bool(self.clip_vloss)))


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _f32(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a contiguous float32 device tensor of shape {tuple(shape)}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return t


def gae(storage: Dict[str, torch.Tensor], gamma, gae_lambda, out=None, *, envs_per_learner: Optional[int] = None):
    """Advantages and returns [T, E] of the storage ``policy_rollout`` returns (rpo_agent.py:205-220), one launch, bit-equal to
    the reference's loop in float32.  ``out`` = (advantages, returns) to reuse.  For a population's storage ``gamma`` and
    ``gae_lambda`` may be sequences of S with ``envs_per_learner = E / S``: learner s's columns take its own pair
    (``evac_gae_learners``), bit-equal to ``gae`` on those columns alone."""
    rewards = storage["rewards"]
    T, E = rewards.shape
    rewards = _f32(rewards, (T, E), "rewards")
    values, dones = _f32(storage["values"], (T, E), "values"), _f32(storage["dones"], (T, E), "dones")
    next_value, next_done = _f32(storage["next_value"], (E,), "next_value"), _f32(storage["next_done"], (E,), "next_done")
    if out is None:
        out = (torch.empty_like(rewards), torch.empty_like(rewards))
    adv, ret = _f32(out[0], (T, E), "advantages"), _f32(out[1], (T, E), "returns")
    per_learner = isinstance(gamma, (list, tuple)) or isinstance(gae_lambda, (list, tuple))
    if per_learner or envs_per_learner is not None:
        if envs_per_learner is None or int(envs_per_learner) < 1 or E % int(envs_per_learner):
            raise ValueError(f"gae: per-learner gamma / gae_lambda need envs_per_learner, a divisor of the storage's {E} envs")
        S = E // int(envs_per_learner)
        hypers = _lib.learner_hypers(S, gamma=gamma, gae_lambda=gae_lambda)
        rc = _lib.load().evac_gae_learners(T, E, _ptr(rewards), _ptr(values), _ptr(dones), _ptr(next_value), _ptr(next_done),
                                           int(envs_per_learner), S, hypers, _ptr(adv), _ptr(ret), _stream(rewards.device))
    else:
        rc = _lib.load().evac_gae(T, E, _ptr(rewards), _ptr(values), _ptr(dones), _ptr(next_value), _ptr(next_done), float(gamma),
                                  float(gae_lambda), _ptr(adv), _ptr(ret), _stream(rewards.device))
    _lib.check(rc)
    return adv, ret


def flatten_batch(storage: Dict[str, torch.Tensor], advantages: torch.Tensor, returns: torch.Tensor) -> Dict[str, torch.Tensor]:
    """rpo_agent.py:223-228: the flattened views of the storage (no copy)."""
    obs = storage["obs"]
    return {"b_obs": obs.reshape(-1, obs.shape[-1]), "b_actions": storage["actions"].reshape(-1, 2),
            "b_logprobs": storage["logprobs"].reshape(-1), "b_advantages": advantages.reshape(-1), "b_returns": returns.reshape(-1),
            "b_values": storage["values"].reshape(-1)}


def _tensor_struct(cache: list, tensors, struct=_lib.EvacMlpPolicyGrads):
    """The addresses of the tensors as ``struct`` (``evac_mlp_policy_grads_t``: 13; ``evac_deepsets_grads_t``: the encoder's 6),
    rebuilt when one of them changes.  ``cache``: [key, struct]."""
    key = tuple(t.data_ptr() for t in tensors)
    if key != cache[0]:
        cache[:] = key, struct(*key)
    return cache[1]


class _GradState:
    """What ``rpo_minibatch_grad`` keeps per network: the binder, the ``.grad`` tensors' addresses and the workspace."""

    def __init__(self):
        self.binder, self.grads, self.workspace = None, [None, None], None
        self.encoder_grads = [None, None]                                    # the encoder's own entries' (ensure_encoder_grads)


def _grad_state(net) -> _GradState:
    st = getattr(net, "_evac_grad_state", None)
    if st is None:
        st = _GradState()
        object.__setattr__(net, "_evac_grad_state", st)
    return st


def ensure_grads(net) -> "_lib.EvacMlpPolicyGrads":
    """Every parameter gets a contiguous float32 ``.grad`` on its device (allocated once, then reused: torch's optimisers update
    in place); their addresses as ``evac_mlp_policy_grads_t``."""
    ts = mlp_tensors(net)
    for t in all_tensors(net):               # (a set encoder's six as well: autograd_minibatch_grad writes them)
        g = t.grad
        if g is None or g.dtype != torch.float32 or g.device != t.device or not g.is_contiguous() or g.shape != t.shape:
            t.grad = torch.zeros_like(t, memory_format=torch.contiguous_format)
    return _tensor_struct(_grad_state(net).grads, [t.grad for t in ts])


def ensure_encoder_grads(net):
    """``ensure_grads`` for the tensors of the encoder of ``net`` (``encoder_kind``): the addresses of their ``.grad`` as
    ``evac_deepsets_grads_t`` (the set encoder's six) or ``evac_transformer_grads_t`` (the attention encoder's 16 per block; the
    blocks the network does not have stay NULL: they are never followed)."""
    ensure_grads(net)
    kind = encoder_kind(net)
    return _tensor_struct(_grad_state(net).encoder_grads, [t.grad for t in kind.tensors(net)], kind.grads)


def _entry_name(kind, what: str) -> str:
    """``evac_rpo_<what>``, or for a row of ``ENCODER_KINDS`` ``evac_deepsets_<what>`` / ``evac_transformer_<what>``."""
    return f"evac{'_rpo' if kind is None else kind.suffix}_{what}"


def _batch_args(net, batch: Dict[str, torch.Tensor], own_encoder_entry: bool = False):
    """The checks every gradient entry makes of ``batch``; returns (B, D, device, state, evac_mlp_policy_t, grads struct, the
    entries' arguments ``batch_size, b_obs .. b_values``).  ``own_encoder_entry``: the caller is an encoder's own entry (the set
    encoder's, or the attention encoder's), not the linear network's, which refuses a network with either."""
    if not own_encoder_entry:
        refuse_deepsets(net, "the device gradient")
    b_obs = batch["b_obs"]
    B, D = b_obs.shape
    dev = b_obs.device
    _f32(b_obs, (B, D), "b_obs")
    _f32(batch["b_actions"], (B, 2), "b_actions")
    for k in BATCH_KEYS[2:]:
        _f32(batch[k], (B,), k)
    st = _grad_state(net)
    if st.binder is None or st.binder.obs_dim != D or st.binder.device != dev:
        st.binder = PolicyBinder(D, dev)
    pol = st.binder(net)
    grads = ensure_grads(net)
    return B, D, dev, st, pol, grads, [B] + [_ptr(batch[k]) for k in BATCH_KEYS]


def _call_buffers(st: _GradState, D: int, M: int, dev, rpo_noise, stats, steps: Optional[int] = None,
                  sizer: str = "evac_rpo_workspace_bytes"):
    """``rpo_noise`` and ``stats`` checked against the call's shape ([M, 2] and [8]; [steps, M, 2] and [steps, 8] for a whole
    update), ``stats`` made if None, the workspace grown if too small for ``sizer``'s figure; returns (stats, the workspace)."""
    lead = () if steps is None else (steps,)
    if rpo_noise is not None:
        _f32(rpo_noise, lead + (M, 2), "rpo_noise")
    need = int(getattr(_lib.load(), sizer)(D, M))
    if need < 0:
        raise _lib.EvacError(need, f"{sizer}({D}, {M})")
    if st.workspace is None or st.workspace.numel() < need or st.workspace.device != dev:
        st.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if stats is None:
        stats = (torch.empty if steps is None else torch.zeros)(lead + (8,), dtype=torch.float32, device=dev)
    else:
        _f32(stats, lead + (8,), "stats")
    return stats, st.workspace


def _loss_config(cfg) -> "_lib.EvacRpoLossConfig":
    return cfg.loss_config() if hasattr(cfg, "loss_config") else RPOTrainingConfig.loss_config(cfg)


def _u64(x: int) -> int:
    return int(x) & (2 ** 64 - 1)


def _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, opt: Optional["DeviceAdam"], kind=None) -> torch.Tensor:
    """``evac_rpo_minibatch_grad``, or with ``opt`` ``evac_rpo_minibatch_step``: the same arguments and the optimiser's three;
    or with ``kind`` (the network's own row of ``ENCODER_KINDS``) ``evac_deepsets_minibatch_grad`` /
    ``evac_transformer_minibatch_grad``: the same arguments, the encoder after the policy and its gradients after the policy's,
    and a workspace of its own size -- and with ``opt`` ``evac_deepsets_minibatch_step`` / ``evac_transformer_minibatch_step``: the
    optimiser's three, the encoder's parameters after the policy's."""
    B, D, dev, st, pol, grads, b_args = _batch_args(net, batch, kind is not None)
    if kind is not None:
        enc, enc_grads = st.binder.bind_encoder(net)[1], ensure_encoder_grads(net)
    if mb_inds.dtype != torch.int64 or mb_inds.device != dev or not mb_inds.is_contiguous() or mb_inds.dim() != 1:
        raise ValueError("mb_inds: expected a contiguous int64 device vector")
    M = int(mb_inds.shape[0])
    stats, ws = _call_buffers(st, D, M, dev, rpo_noise, stats, sizer=_entry_name(kind, "workspace_bytes"))
    lc = _loss_config(cfg)
    args = [C.byref(pol), C.byref(lc), *b_args, M, _ptr(mb_inds), _ptr(rpo_noise), _u64(seed), _u64(draw_counter), C.byref(grads),
            _ptr(stats), _ptr(ws), _stream(dev)]
    if kind is not None:
        args = [args[0], C.byref(enc), *args[1:-3], C.byref(enc_grads), *args[-3:]]
    if opt is not None:
        oc = opt.config()
        args += [C.byref(opt.params_struct()), *([] if kind is None else [C.byref(opt.encoder_params_struct())]),
                 C.byref(opt.state_struct()), C.byref(oc)]
    _lib.check(getattr(_lib.load(), _entry_name(kind, "minibatch_grad" if opt is None else "minibatch_step"))(*args))
    return stats


def rpo_minibatch_grad(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, *, rpo_noise: Optional[torch.Tensor] = None,
                       seed: int = 0, draw_counter: int = 0, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of the RPO loss of the minibatch ``mb_inds`` of ``batch`` (``flatten_batch``) into the parameters' ``.grad``
    (written, not accumulated), by ``evac_rpo_minibatch_grad``; returns the 8 statistics (``STAT_NAMES``) as a device tensor.
    ``cfg``: an ``RPOTrainingConfig`` (or anything with its loss fields).  ``rpo_noise`` [M, 2] injects the RPO perturbation;
    None draws it on the device from (``seed``, ``draw_counter``).  No host synchronisation; capturable into a graph."""
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, None)


def deepsets_minibatch_grad(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, *, rpo_noise: Optional[torch.Tensor] = None,
                            seed: int = 0, draw_counter: int = 0, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rpo_minibatch_grad`` for a network with the reference's set encoder (``policy.DeepSetsActorCritic``): the gradient of the
    RPO loss of the minibatch into the ``.grad`` of all 19 tensors (written, not accumulated) by ``evac_deepsets_minibatch_grad``
    -- the encoder forwards, the linear network's three gradient launches on the encoded observations, the encoder backwards.
    Same arguments, same 8 statistics (``stats[7]``: the sum of squares over the 19 tensors), deterministic, no host
    synchronisation, capturable.  The optimiser stays torch's (``RPOTrainer(grad_fn=deepsets_kernel_grad)``)."""
    refuse_transformer(net, "deepsets_minibatch_grad")
    if not is_deepsets(net):
        raise ValueError("deepsets_minibatch_grad: the network has no set encoder (`deep_sets`); its gradient is rpo_minibatch_grad's")
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, None, encoder_kind(net))


def transformer_minibatch_grad(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, *,
                               rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, draw_counter: int = 0,
                               stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rpo_minibatch_grad`` for a network with the reference's attention encoder (``policy.TransformerActorCritic``): the
    gradient of the RPO loss of the minibatch into the ``.grad`` of all 13 + 16 per block tensors (written, not accumulated) by
    ``evac_transformer_minibatch_grad`` -- the encoder forwards, the linear network's three gradient launches on the encoded
    observations, one launch per block backwards.  Same arguments, same 8 statistics (``stats[7]``: the sum of squares over all
    the tensors), deterministic, no host synchronisation, capturable.  The encoder is the eval-mode function: a dropout
    probability other than 0 is refused.  The optimiser is torch's (``RPOTrainer(grad_fn=transformer_kernel_grad)``) or, in the
    same call, the device's (``transformer_minibatch_step``)."""
    if not is_transformer(net):
        raise ValueError("transformer_minibatch_grad: the network has no attention encoder (`embedding`); its gradient is "
                         "rpo_minibatch_grad's or deepsets_minibatch_grad's")
    refuse_dropout(net, "transformer_minibatch_grad")
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, None, encoder_kind(net))


HEADER_FIELDS = ("t", "P1", "P2", "stop", "steps_run", "epochs_run")


def decode_header(header: torch.Tensor) -> dict:
    """The optimiser's 64-byte header (``evac_adam_state_t.header``) as a dict of ``HEADER_FIELDS``: one host transfer for a
    device tensor, none for a host copy."""
    h = header.detach().cpu().contiguous().view(torch.int64).numpy()
    t = int(h[0])
    P1, P2 = (float(x) for x in h[1:3].view("float64"))
    stop, steps_run, epochs_run = (int(x) for x in h[3:5].view("int32")[:3])
    return {"t": t, "P1": P1 if t else 1.0, "P2": P2 if t else 1.0, "stop": stop, "steps_run": steps_run, "epochs_run": epochs_run}


# evac_deepsets_adam_state_t / evac_transformer_adam_state_t by the suffix of the encoder's entries
_ENCODER_ADAM_STATES = {"_deepsets": _lib.EvacDeepSetsAdamState, "_transformer": _lib.EvacTransformerAdamState}


class DeviceAdam:
    """``clip_grad_norm_(max_grad_norm)`` and ``torch.optim.Adam(lr, betas, eps)`` (no weight decay, no amsgrad) for the 13
    tensors of ``net`` in one launch (``evac_adam_step``; the arithmetic is specified in include/evac.h) -- or, for a network
    with a set encoder, for all 19 in ``all_tensors`` order (``evac_deepsets_adam_step``: one launch, one clip coefficient, one
    step count).  The step count and the bias corrections' running products live on the device, so a captured step counts when
    it is replayed.  ``param_groups[0]`` is read at every call: ``opt.param_groups[0]["lr"] = lrnow`` works as with torch."""

    def __init__(self, net, lr: float = 3e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5,
                 *, storage=None):
        """``storage`` = (header, exp_avg, exp_avg_sq): the state lives in the caller's tensors (``PopulationAdam``'s rows: 13
        tensors, or all 19 for a network with a set encoder -- 13 for such a network is a ``ValueError``)."""
        refuse_transformer(net, "DeviceAdam")                                   # (its own optimiser is TransformerAdam)
        self._setup(net, lr, betas, eps, max_grad_norm, storage)

    def _setup(self, net, lr, betas, eps, max_grad_norm, storage=None) -> None:
        """The constructor's body for the network's own kind (``encoder_kind``): the 13 tensors' state, then the encoder's."""
        self.kind = encoder_kind(net)
        self.deepsets = is_deepsets(net) and not is_transformer(net)
        if self.deepsets and storage is not None and (len(storage[1]) != 19 or len(storage[2]) != 19):
            raise ValueError("DeviceAdam: `storage` holds the 13 tensors of a linear population's row; a network with a set encoder "
                             "(`deep_sets`) has 19 (a DeepSetsPopulation's row)")
        group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "max_grad_norm": float(max_grad_norm)}
        self._check_group(group)
        self.net = net
        self.params = list(all_tensors(net))        # (13, or 19 with a set encoder)
        self.device = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise ValueError("DeviceAdam: the parameters must be contiguous float32 device tensors")
        self.obs_dim = int(self.params[0].shape[1])
        self.set_elem_dim = int(self.params[13].shape[1]) if self.deepsets else None
        self.elem_dim = int(self.params[13].shape[1]) if self.kind is not None else None     # (phi_w1 [24][ed]; wq [3 dm][dm])
        self.param_groups = [group]
        if storage is None:
            self.header = torch.zeros(8, dtype=torch.int64, device=self.device)
            self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
            self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        else:
            self.header, self.exp_avg, self.exp_avg_sq = storage[0], list(storage[1]), list(storage[2])
        self._state = _lib.EvacAdamState(self.header.data_ptr(), _lib.EvacMlpPolicyGrads(*(t.data_ptr() for t in self.exp_avg[:13])),
                                         _lib.EvacMlpPolicyGrads(*(t.data_ptr() for t in self.exp_avg_sq[:13])))
        if self.kind is not None:                                               # (the encoder's moments after the 13 tensors')
            self._state = _ENCODER_ADAM_STATES[self.kind.suffix](self._state.header, self._state.exp_avg, self._state.exp_avg_sq,
                                                                 self.kind.grads(*(t.data_ptr() for t in self.exp_avg[13:])),
                                                                 self.kind.grads(*(t.data_ptr() for t in self.exp_avg_sq[13:])))
        self._params, self._encoder_params = [None, None], [None, None]
        ensure_grads(net)

    @staticmethod
    def _check_group(g: dict) -> None:
        b1, b2 = g["betas"]
        if not math.isfinite(g["lr"]):
            raise ValueError(f"DeviceAdam: lr = {g['lr']} is not finite")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"DeviceAdam: betas = {g['betas']} outside [0, 1)")
        if not g["eps"] > 0.0:
            raise ValueError(f"DeviceAdam: eps = {g['eps']} must be > 0")
        if not g["max_grad_norm"] > 0.0:
            raise ValueError(f"DeviceAdam: max_grad_norm = {g['max_grad_norm']} must be > 0")

    def config(self) -> "_lib.EvacAdamConfig":
        g = self.param_groups[0]
        return _lib.EvacAdamConfig(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["max_grad_norm"]))

    def params_struct(self) -> "_lib.EvacMlpPolicyGrads":
        return _tensor_struct(self._params, self.params[:13])

    def encoder_params_struct(self):
        """The encoder's parameter tensors as its gradients' struct (a network with an encoder only): the set encoder's six, or
        ``TransformerAdam``'s 16 per block."""
        return _tensor_struct(self._encoder_params, self.params[13:], self.kind.grads)

    def state_struct(self):
        """``evac_adam_state_t``, or ``evac_deepsets_adam_state_t`` for a network with a set encoder
        (``evac_transformer_adam_state_t``: ``TransformerAdam``)."""
        return self._state

    def step(self, grad_sumsq: torch.Tensor) -> None:
        """Clip the parameters' ``.grad`` by ``grad_sumsq`` (a float32 device scalar: the sum of squares of all gradient entries,
        ``stats[7]`` of ``rpo_minibatch_grad``) and take one Adam step.  One launch, no host synchronisation."""
        if not isinstance(grad_sumsq, torch.Tensor) or grad_sumsq.dtype != torch.float32 or grad_sumsq.device != self.device or grad_sumsq.numel() != 1:
            raise ValueError("DeviceAdam.step: grad_sumsq must be a float32 scalar on the parameters' device")
        grads = ensure_grads(self.net)
        cfg = self.config()
        if self.kind is not None:                                               # (evac_deepsets_adam_step / evac_transformer_adam_step)
            rc = getattr(_lib.load(), _entry_name(self.kind, "adam_step"))(
                C.byref(self.params_struct()), C.byref(self.encoder_params_struct()), C.byref(grads),
                C.byref(ensure_encoder_grads(self.net)), C.byref(self._state), C.byref(cfg), self.obs_dim, *self._encoder_sizes(),
                _ptr(grad_sumsq), _stream(self.device))
        else:
            rc = _lib.load().evac_adam_step(C.byref(self.params_struct()), C.byref(grads), C.byref(self._state), C.byref(cfg),
                                            self.obs_dim, _ptr(grad_sumsq), _stream(self.device))
        _lib.check(rc)

    def _encoder_sizes(self) -> tuple:
        """What the encoder's ``adam_step`` entry takes between ``obs_dim`` and ``grad_sumsq``: ``set_elem_dim``."""
        return (self.set_elem_dim,)

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Nothing to do: the gradient kernels write ``.grad``, they do not accumulate (kept for torch's interface)."""

    def read_header(self) -> dict:
        return decode_header(self.header)

    @property
    def step_count(self) -> int:
        return int(self.header[0].item())

    def state_dict(self) -> dict:
        """``torch.optim.Adam``'s format (``state[i]`` in ``all_tensors`` order: 13 entries, 19 with a set encoder), plus ``P1``, ``P2`` (the running products) and
        ``max_grad_norm`` in the param group: torch's ``load_state_dict`` takes the dict once those three keys are dropped."""
        h = self.read_header()
        g = self.param_groups[0]
        state = {i: {"step": torch.tensor(float(h["t"])), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
                 for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq))}
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
                 "max_grad_norm": g["max_grad_norm"], "P1": h["P1"], "P2": h["P2"], "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict) -> None:
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"DeviceAdam.load_state_dict: expected one param group of {len(self.params)} tensors")
        sg = groups[0]
        if sg.get("weight_decay", 0) or sg.get("amsgrad", False):
            raise ValueError("DeviceAdam.load_state_dict: weight decay and amsgrad are not supported")
        g = dict(self.param_groups[0])
        g.update({"lr": float(sg["lr"]), "betas": (float(sg["betas"][0]), float(sg["betas"][1])), "eps": float(sg["eps"])})
        if "max_grad_norm" in sg:
            g["max_grad_norm"] = float(sg["max_grad_norm"])
        self._check_group(g)
        state = sd["state"]
        steps = {int(float(state[i]["step"])) for i in sg["params"]} if state else {0}
        if len(steps) != 1:
            raise ValueError("DeviceAdam.load_state_dict: the tensors' step counts differ")
        t = steps.pop()
        with torch.no_grad():
            for k, i in enumerate(sg["params"]):
                if state:
                    self.exp_avg[k].copy_(state[i]["exp_avg"])
                    self.exp_avg_sq[k].copy_(state[i]["exp_avg_sq"])
                else:
                    self.exp_avg[k].zero_()
                    self.exp_avg_sq[k].zero_()
        P1 = float(sg["P1"]) if "P1" in sg else g["betas"][0] ** t
        P2 = float(sg["P2"]) if "P2" in sg else g["betas"][1] ** t
        host = torch.zeros(8, dtype=torch.int64)
        host[0] = t
        host[1:3] = torch.tensor([P1, P2], dtype=torch.float64).view(torch.int64)
        self.header.copy_(host)
        self.param_groups[0] = g


def _check_opt(opt, net) -> None:
    refuse_transformer(net, "the device optimiser step")      # (no DeviceAdam exists for such a network: say why, not "no DeviceAdam")
    if not isinstance(opt, DeviceAdam):
        raise TypeError(f"expected a DeviceAdam, got {type(opt).__name__}")
    if opt.net is not net:
        raise ValueError("the DeviceAdam was made for another network")


class TransformerAdam(DeviceAdam):
    """``DeviceAdam`` for a network with the reference's attention encoder (``policy.TransformerActorCritic``): clip + Adam over
    all 13 + 16 per block tensors in ``all_tensors`` order (29 with one block, 45 with two) in one launch
    (``evac_transformer_adam_step``: one clip coefficient, one step count, one header).  The same interface: ``step``,
    ``param_groups``, ``config``, the structs, ``read_header``, ``step_count``, ``state_dict`` / ``load_state_dict`` in torch's
    format.  A class of its own because ``DeviceAdam(net)`` stays a ``ValueError`` for such a network."""

    def __init__(self, net, lr: float = 3e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5,
                 *, storage=None):
        """``storage`` = (header, exp_avg, exp_avg_sq), as ``DeviceAdam`` takes it: the state lives in the caller's tensors
        (``TransformerPopulationAdam``'s rows), as many moments of each kind as the network has tensors (29 or 45) -- any other
        count is a ``ValueError``."""
        if not is_transformer(net):
            raise ValueError("TransformerAdam: the network has no attention encoder (`embedding`); its optimiser is DeviceAdam")
        refuse_dropout(net, "TransformerAdam")
        count = len(all_tensors(net))
        if storage is not None and (len(storage) != 3 or len(storage[1]) != count or len(storage[2]) != count):
            raise ValueError(f"TransformerAdam: `storage` is (header, {count} exp_avg, {count} exp_avg_sq) for this network's 13 + 16 per "
                             "block tensors (a TransformerPopulation's row)")
        self._setup(net, lr, betas, eps, max_grad_norm, storage)
        self.num_blocks = (len(self.params) - 13) // 16

    def _encoder_sizes(self) -> tuple:
        return (self.elem_dim, self.num_blocks)


def _check_transformer_opt(opt, net, what: str) -> None:
    """``_check_opt`` for the attention encoder's own entries (``_check_opt`` refuses such a network for every other)."""
    if not is_transformer(net):
        raise ValueError(f"{what}: the network has no attention encoder (`embedding`); its entries are rpo_* or deepsets_*")
    refuse_dropout(net, what)
    if not isinstance(opt, TransformerAdam):
        raise TypeError(f"expected a TransformerAdam, got {type(opt).__name__}")
    if opt.net is not net:
        raise ValueError("the TransformerAdam was made for another network")


def rpo_minibatch_step(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, opt: DeviceAdam, *,
                       rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, draw_counter: int = 0,
                       stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rpo_minibatch_grad`` with the same arguments, then ``opt.step(stats[7])``, in one host call
    (``evac_rpo_minibatch_step``: one launch more than the gradient).  ``.grad`` is left clipped; ``stats`` are those of the
    gradient at the parameters before the step.  No host synchronisation; capturable (``lr`` and ``draw_counter`` are frozen by
    a capture, the step count is not)."""
    _check_opt(opt, net)
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, opt)


def update_steps(batch_size: int, minibatch_size: int, norm_adv: bool) -> list:
    """The sizes of the minibatches of one epoch, in order: ``range(0, B, M)`` with a tail of fewer than 2 samples (1 without
    ``norm_adv``) left out, as the trainer's loop skips it."""
    B, M, least = int(batch_size), int(minibatch_size), 2 if norm_adv else 1
    return [min(M, B - s) for s in range(0, B, M) if min(M, B - s) >= least]


def _update_call(net, batch, perms, cfg, opt, rpo_noise, seed, first_draw_counter, stats, minibatch_size, kind=None, checked=False):
    """``evac_rpo_update``, or with ``kind`` (the network's own row of ``ENCODER_KINDS``) ``evac_deepsets_update`` /
    ``evac_transformer_update``: the same arguments with the encoder after the policy, its parameters after the policy's and its
    gradients after the policy's, and a workspace of its own size.  ``checked``: the caller has checked ``opt`` itself
    (``transformer_update``: ``_check_opt`` refuses its network)."""
    if not checked:
        _check_opt(opt, net)
    B, D, dev, st, pol, grads, b_args = _batch_args(net, batch, kind is not None)
    name = _entry_name(kind, "update")
    if not isinstance(perms, torch.Tensor) or perms.dtype != torch.int64 or perms.device != dev or not perms.is_contiguous() or \
            perms.dim() != 2 or perms.shape[1] != B or perms.shape[0] < 1:
        raise ValueError(f"perms: expected a contiguous int64 device tensor of shape [epochs, {B}]")
    M = int(cfg.minibatch_size if minibatch_size is None else minibatch_size)
    norm_adv = bool(getattr(cfg, "norm_adv", True))
    if M < (2 if norm_adv else 1):
        raise ValueError(f"{name[len('evac_'):]}: minibatch_size = {M}")
    M = min(M, B)
    n_epochs = int(perms.shape[0])
    steps = n_epochs * len(update_steps(B, M, norm_adv))
    stats, ws = _call_buffers(st, D, M, dev, rpo_noise, stats, steps, sizer=_entry_name(kind, "workspace_bytes"))
    target_kl = getattr(cfg, "target_kl", None)
    lc, oc = _loss_config(cfg), opt.config()
    front = [C.byref(pol), C.byref(opt.params_struct()), C.byref(grads)]
    if kind is not None:                                                      # ... each followed by the encoder's
        enc, enc_grads = st.binder.bind_encoder(net)[1], ensure_encoder_grads(net)
        front = [x for pair in zip(front, map(C.byref, (enc, opt.encoder_params_struct(), enc_grads))) for x in pair]
    rc = getattr(_lib.load(), name)(*front, C.byref(lc), C.byref(oc), C.byref(opt.state_struct()), *b_args, M, n_epochs,
                                    _ptr(perms), _ptr(rpo_noise), _u64(seed), _u64(first_draw_counter), int(target_kl is not None),
                                    float(target_kl or 0.0), _ptr(stats), _ptr(ws), _stream(dev))
    _lib.check(rc)
    return stats, opt.header


def rpo_update(net, batch: Dict[str, torch.Tensor], perms: torch.Tensor, cfg, opt: DeviceAdam, *,
               rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, first_draw_counter: int = 0,
               stats: Optional[torch.Tensor] = None, minibatch_size: Optional[int] = None):
    """rpo_agent.py:233-283 in one host call (``evac_rpo_update``): for every row of ``perms`` (int64 [epochs, B], device) and
    every ``start`` in ``range(0, B, M)`` one minibatch step on ``perms[epoch, start:start + M]``, ``M = minibatch_size``
    (default ``cfg.minibatch_size``).  Step k of the call draws its perturbation at ``first_draw_counter + k`` or reads
    ``rpo_noise[k]`` ([steps, M, 2]).  With ``cfg.target_kl`` set, the early exit is taken on the device.  Returns
    (``stats`` [steps, 8], the optimiser's header: ``decode_header``); rows beyond ``steps_run`` keep what they held."""
    return _update_call(net, batch, perms, cfg, opt, rpo_noise, seed, first_draw_counter, stats, minibatch_size)


def deepsets_minibatch_step(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, opt: DeviceAdam, *,
                            rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, draw_counter: int = 0,
                            stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rpo_minibatch_step`` for a network with a set encoder: ``deepsets_minibatch_grad`` with the same arguments, then
    ``opt.step(stats[7])`` over all 19 tensors, in one host call (``evac_deepsets_minibatch_step``: one launch more than the
    gradient).  ``.grad`` is left clipped; ``stats`` are those of the gradient at the parameters before the step.  No host
    synchronisation; capturable (``lr`` and ``draw_counter`` are frozen by a capture, the step count is not)."""
    refuse_transformer(net, "deepsets_minibatch_step")
    if not is_deepsets(net):
        raise ValueError("deepsets_minibatch_step: the network has no set encoder (`deep_sets`); its step is rpo_minibatch_step's")
    _check_opt(opt, net)
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, opt, encoder_kind(net))


def deepsets_update(net, batch: Dict[str, torch.Tensor], perms: torch.Tensor, cfg, opt: DeviceAdam, *,
                    rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, first_draw_counter: int = 0,
                    stats: Optional[torch.Tensor] = None, minibatch_size: Optional[int] = None):
    """``rpo_update`` for a network with a set encoder (``evac_deepsets_update``): the same arguments, the same returns
    (``stats`` [steps, 8], the optimiser's header), the ``target_kl`` exit taken on the device; bit for bit the host loop of
    ``deepsets_minibatch_step``."""
    refuse_transformer(net, "deepsets_update")
    if not is_deepsets(net):
        raise ValueError("deepsets_update: the network has no set encoder (`deep_sets`); its update is rpo_update's")
    return _update_call(net, batch, perms, cfg, opt, rpo_noise, seed, first_draw_counter, stats, minibatch_size, encoder_kind(net))


def transformer_minibatch_step(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, opt: "TransformerAdam", *,
                               rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, draw_counter: int = 0,
                               stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rpo_minibatch_step`` for a network with an attention encoder: ``transformer_minibatch_grad`` with the same arguments,
    then ``opt.step(stats[7])`` over all 13 + 16 per block tensors, in one host call (``evac_transformer_minibatch_step``: one
    launch more than the gradient).  ``.grad`` is left clipped; ``stats`` are those of the gradient at the parameters before the
    step.  No host synchronisation; capturable (``lr`` and ``draw_counter`` are frozen by a capture, the step count is not)."""
    _check_transformer_opt(opt, net, "transformer_minibatch_step")
    return _minibatch_call(net, batch, mb_inds, cfg, rpo_noise, seed, draw_counter, stats, opt, encoder_kind(net))


def transformer_update(net, batch: Dict[str, torch.Tensor], perms: torch.Tensor, cfg, opt: "TransformerAdam", *,
                       rpo_noise: Optional[torch.Tensor] = None, seed: int = 0, first_draw_counter: int = 0,
                       stats: Optional[torch.Tensor] = None, minibatch_size: Optional[int] = None):
    """``rpo_update`` for a network with an attention encoder (``evac_transformer_update``): the same arguments, the same
    returns (``stats`` [steps, 8], the optimiser's header), the ``target_kl`` exit taken on the device; bit for bit the host loop
    of ``transformer_minibatch_step``."""
    _check_transformer_opt(opt, net, "transformer_update")
    return _update_call(net, batch, perms, cfg, opt, rpo_noise, seed, first_draw_counter, stats, minibatch_size, encoder_kind(net),
                        checked=True)


def _kernel_grad(trainer: "RPOTrainer", batch, mb_inds, rpo_noise, draw_counter: int, stats: torch.Tensor) -> torch.Tensor:
    return rpo_minibatch_grad(trainer.net, batch, mb_inds, trainer.cfg, rpo_noise=rpo_noise, seed=trainer.cfg.seed,
                              draw_counter=draw_counter, stats=stats)


def deepsets_kernel_grad(trainer: "RPOTrainer", batch, mb_inds, rpo_noise, draw_counter: int, stats: torch.Tensor) -> torch.Tensor:
    """A ``grad_fn`` of ``RPOTrainer`` for a network with a set encoder: ``deepsets_minibatch_grad`` (collection and gradient on
    the device, torch's clip and Adam).  Opt-in: the default for such a network stays ``autograd_minibatch_grad``."""
    return deepsets_minibatch_grad(trainer.net, batch, mb_inds, trainer.cfg, rpo_noise=rpo_noise, seed=trainer.cfg.seed,
                                   draw_counter=draw_counter, stats=stats)


def transformer_kernel_grad(trainer: "RPOTrainer", batch, mb_inds, rpo_noise, draw_counter: int, stats: torch.Tensor) -> torch.Tensor:
    """A ``grad_fn`` of ``RPOTrainer`` for a network with an attention encoder: ``transformer_minibatch_grad`` (collection and
    gradient on the device; torch's clip and Adam, or with ``optimizer="device_transformer"`` ``TransformerAdam``: the whole
    update one ``transformer_update``).  Opt-in: the default for such a network stays ``autograd_minibatch_grad``, and
    ``optimizer="device"`` stays refused with any ``grad_fn``."""
    return transformer_minibatch_grad(trainer.net, batch, mb_inds, trainer.cfg, rpo_noise=rpo_noise, seed=trainer.cfg.seed,
                                      draw_counter=draw_counter, stats=stats)


# The gradient functions whose step and whole update exist as one host call (RPOTrainer with optimizer="device")
_STEP_OF = ((_kernel_grad, rpo_minibatch_step), (deepsets_kernel_grad, deepsets_minibatch_step))
_UPDATE_OF = ((_kernel_grad, rpo_update), (deepsets_kernel_grad, deepsets_update))
# ... per optimiser kind of RPOTrainer: (the step's table, the update's); "device_transformer" (TransformerAdam) has its own pair
_ONE_CALL_TABLES = {"device": (_STEP_OF, _UPDATE_OF),
                    "device_transformer": (((transformer_kernel_grad, transformer_minibatch_step),),
                                           ((transformer_kernel_grad, transformer_update),))}


def _one_call_form(grad_fn, table):
    """The entry of ``table`` for ``grad_fn`` (compared by identity), or None."""
    return next((form for fn, form in table if grad_fn is fn), None)


def _draw_seed(seed: int, draw_counter: int) -> int:
    return ((int(seed) & 0xffffffff) << 31) ^ (int(draw_counter) & 0x7fffffff)


def autograd_minibatch_grad(trainer, batch, mb_inds, rpo_noise, draw_counter: int, stats: torch.Tensor) -> torch.Tensor:
    """A ``grad_fn`` of ``RPOTrainer`` for ANY network it takes: the reference's minibatch loss (rpo_agent.py:239-274 with
    get_action_and_value of rpo_linear_agent_network.py:48-61 / rpo_deep_sets_agent_network.py:83-90) through torch autograd on
    the module itself -- the gradient of a network with a set encoder, whose 19 tensors the linear gradient kernels do not know,
    and of one with an attention encoder (rpo_transformer_agent_network.py), whose 45 ``transformer_kernel_grad`` does on opt-in.
    Writes the parameters' ``.grad`` (not accumulated) and the 8 statistics (``STAT_NAMES``; ``stats[7]`` the gradient's sum of
    squares, in double).  ``rpo_noise`` [M, 2]: the perturbation of the mean; None draws U(-rpo_alpha, rpo_alpha) from a torch
    generator seeded with (``cfg.seed``, ``draw_counter``).  ``trainer``: anything with ``net`` and ``cfg``."""
    net, cfg = trainer.net, trainer.cfg
    params = list(all_tensors(net))
    dev = params[0].device
    M = int(mb_inds.shape[0])
    if rpo_noise is None:
        gen = getattr(trainer, "_autograd_generator", None)
        if gen is None or gen.device != dev:
            gen = trainer._autograd_generator = torch.Generator(device=dev)
        gen.manual_seed(_draw_seed(cfg.seed, draw_counter))
        alpha = float(cfg.rpo_alpha)
        rpo_noise = (torch.rand(M, 2, device=dev, dtype=torch.float32, generator=gen) * 2.0 - 1.0) * alpha
    with torch.enable_grad():
        y = encode_observation(net, batch["b_obs"][mb_inds])
        mean = net.actor_mean(y) + rpo_noise
        probs = torch.distributions.normal.Normal(mean, torch.exp(net.actor_logstd.expand_as(mean)))
        newlogprob, entropy = probs.log_prob(batch["b_actions"][mb_inds]).sum(1), probs.entropy().sum(1)
        newvalue = net.critic(y).view(-1)
        logratio = newlogprob - batch["b_logprobs"][mb_inds]
        ratio = logratio.exp()
        with torch.no_grad():
            old_approx_kl = (-logratio).mean()
            approx_kl = ((ratio - 1) - logratio).mean()
            clipfrac = ((ratio - 1.0).abs() > cfg.clip_coef).float().mean()
        adv = batch["b_advantages"][mb_inds]
        if cfg.norm_adv:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)).mean()
        ret, old_v = batch["b_returns"][mb_inds], batch["b_values"][mb_inds]
        if cfg.clip_vloss:
            v_clipped = old_v + torch.clamp(newvalue - old_v, -cfg.clip_coef, cfg.clip_coef)
            v_loss = 0.5 * torch.max((newvalue - ret) ** 2, (v_clipped - ret) ** 2).mean()
        else:
            v_loss = 0.5 * ((newvalue - ret) ** 2).mean()
        ent = entropy.mean()
        loss = pg_loss - cfg.ent_coef * ent + v_loss * cfg.vf_coef
        grads = torch.autograd.grad(loss, params)
    with torch.no_grad():
        for p, g in zip(params, grads):
            if p.grad is None or p.grad.shape != g.shape:
                p.grad = g.contiguous().clone()
            else:
                p.grad.copy_(g)
        sumsq = torch.stack([(g.double() ** 2).sum() for g in grads]).sum().float()
        stats.copy_(torch.stack([loss.detach(), pg_loss.detach(), v_loss.detach(), ent.detach(), old_approx_kl, approx_kl, clipfrac,
                                 sumsq]))
    return stats


class RPOTrainer:
    """One iteration of the reference's training loop (rpo_agent.py:172-299) per ``update()``: learning-rate annealing, the
    collection phase (``policy_rollout``), ``gae``, ``update_epochs`` x ``num_minibatches`` steps of gradient (kernel),
    ``clip_grad_norm_`` (from the kernel's sum of squares) and ``Adam(eps=1e-5)``, the ``target_kl`` early exit.

    ``net``: the linear network, or one with the reference's set encoder (``policy.DeepSetsActorCritic``): its collection and
    evaluation run on the device too, its gradient is ``autograd_minibatch_grad`` (the default ``grad_fn`` then) or, with
    ``grad_fn=deepsets_kernel_grad``, the device's (``evac_deepsets_minibatch_grad``).  Its optimiser is torch's by default;
    ``optimizer="device"`` takes an explicit ``grad_fn`` (``DeviceAdam`` over all 19 tensors: with ``deepsets_kernel_grad`` the
    whole update is one ``deepsets_update``, or one ``deepsets_minibatch_step`` per minibatch with ``one_call=False``; any other
    ``grad_fn`` is followed by ``self.optimizer.step(stats[7])``) and stays a ``ValueError`` with ``grad_fn`` left at its
    default, which for such a network is autograd's.  Or one with the reference's attention encoder
    (``policy.TransformerActorCritic``): collection and evaluation on the device, the gradient of its 13 + 16 per block tensors
    by ``autograd_minibatch_grad`` or, with ``grad_fn=transformer_kernel_grad``, the device's
    (``evac_transformer_minibatch_grad``), and torch's Adam -- or, with ``optimizer="device_transformer"`` and an explicit
    ``grad_fn``, ``TransformerAdam`` over all its tensors: with ``transformer_kernel_grad`` the whole update is one
    ``transformer_update``, or one ``transformer_minibatch_step`` per minibatch with ``one_call=False``; any other ``grad_fn`` is
    followed by ``self.optimizer.step(stats[7])``.  ``optimizer="device"`` (with any ``grad_fn``) and a dropout probability other
    than 0 (the device collects with the eval-mode function) are ``ValueError``s, as is ``optimizer="device_transformer"`` for a
    network without an attention encoder or with ``grad_fn`` left at its default.

    ``env``: a ``NormalizedVectorEnv`` (the trainer's wrapper chain) or a ``BatchedEvacuationEnv`` with ``cfg.num_envs`` envs.
    The permutation of every epoch is drawn on the device from a generator seeded with ``cfg.seed`` (the reference shuffles on
    the host).  ``grad_fn(trainer, batch, mb_inds, rpo_noise, draw_counter, stats)`` computes the gradient of one minibatch into
    the parameters' ``.grad`` and returns the 8 statistics: the kernel by default.  ``rpo_noise_fn(M)`` -> [M, 2] injects the
    RPO perturbation (default: drawn inside the kernel).

    ``optimizer="torch"`` (default): ``torch.optim.Adam`` and a ``foreach`` clip.  ``optimizer="device"``: ``DeviceAdam``.  The
    permutations of all epochs are then drawn before the loop, so with ``target_kl`` the generator advances by
    ``update_epochs`` draws per update whether or not the loop stops early.  With the default ``grad_fn`` and ``one_call=True``
    the whole update is one ``rpo_update`` (the early exit on the device; an ``rpo_noise_fn`` is called once per step in step
    order before the call and the results stacked, so both forms see the same perturbations -- for every epoch, stopped early
    or not); ``one_call=False`` makes one ``rpo_minibatch_step`` per minibatch and reads ``approx_kl`` on the host after every
    epoch; a custom ``grad_fn`` is followed by ``self.optimizer.step(stats[7])``."""

    def __init__(self, env, net, cfg: RPOTrainingConfig, *, grad_fn: Optional[Callable] = None,
                 rpo_noise_fn: Optional[Callable[[int], torch.Tensor]] = None, optimizer: str = "torch", one_call: bool = True):
        cfg.check()
        if optimizer not in ("torch", "device", "device_transformer"):
            raise ValueError(f"RPOTrainer: optimizer = {optimizer!r}: expected \"torch\", \"device\" or \"device_transformer\"")
        self.optimizer_kind, self.one_call = optimizer, bool(one_call)
        self.device_optimizer = optimizer != "torch"                            # (DeviceAdam or TransformerAdam)
        if env.num_envs != cfg.num_envs:
            raise ValueError(f"RPOTrainer: the env has {env.num_envs} envs, cfg.num_envs = {cfg.num_envs}")
        self.env, self.net, self.cfg = env, net, cfg
        if optimizer == "device":                                               # (no optimiser kernel knows an attention encoder's tensors)
            refuse_transformer(net, "RPOTrainer(optimizer=\"device\")")
        if optimizer == "device_transformer":
            if not is_transformer(net):
                raise ValueError("RPOTrainer(optimizer=\"device_transformer\"): the network has no attention encoder (`embedding`); "
                                 "its device optimiser is optimizer=\"device\"")
            if grad_fn is None:                                                 # (the default gradient of such a net is autograd's)
                raise ValueError("RPOTrainer(optimizer=\"device_transformer\") takes an explicit grad_fn "
                                 "(transformer_kernel_grad: the whole update on the device); the default gradient of a network with "
                                 "an attention encoder is autograd's")
        refuse_dropout(net, "RPOTrainer")                                       # (collection is the eval-mode function)
        if is_deepsets(net) and optimizer == "device" and grad_fn is None:     # (the default gradient of such a net is autograd's)
            refuse_deepsets(net, "RPOTrainer(optimizer=\"device\")")
        # (an encoder: collection and evaluation on the device, the gradient of all 19 / 13 + 16 per block tensors by autograd)
        self.grad_fn = grad_fn or (autograd_minibatch_grad if encoder_kind(net) is not None else _kernel_grad)
        self.rpo_noise_fn = rpo_noise_fn
        self.params = list(all_tensors(net))
        self.device = self.params[0].device
        ensure_grads(net)
        if self.device_optimizer:
            make = TransformerAdam if optimizer == "device_transformer" else DeviceAdam
            self.optimizer = make(net, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm)
        else:
            self.optimizer = torch.optim.Adam(self.params, lr=cfg.learning_rate, eps=1e-5)
        self.stats_rows = None
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(cfg.seed))
        self.update_index = 0            # updates done
        self.global_step = 0
        self.minibatch_steps = 0         # the draw counter of the RPO perturbation
        self.start_time = None
        self.storage = None
        self.advantages = self.returns = None
        self.stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.next_obs = self.next_done = None
        self.last_permutations = []
        self.evaluator = None            # evaluate(): built on first use

    def _start(self):
        obs, _ = self.env.reset(seed=self.cfg.seed)
        self.next_obs = obs.clone()
        self.next_done = torch.zeros(self.cfg.num_envs, dtype=torch.float32, device=self.device)
        self.start_time = time.time()

    def collect(self):
        """rpo_agent.py:180-196 (one launch) and :205-220 (one launch)."""
        if self.next_obs is None:
            self._start()
        with torch.no_grad():
            self.storage = self.env.policy_rollout(self.net, self.cfg.num_steps, self.next_obs, self.next_done, out=self.storage)
            out = None if self.advantages is None else (self.advantages, self.returns)
            self.advantages, self.returns = gae(self.storage, self.cfg.gamma, self.cfg.gae_lambda, out=out)
        self.global_step += self.cfg.batch_size
        return self.storage

    def apply_gradient(self, stats: torch.Tensor):
        """``clip_grad_norm_`` (rpo_agent.py:279) from the sum of squares the gradient step left in ``stats[7]``, then Adam."""
        if self.device_optimizer:
            return self.optimizer.step(stats[7])
        coef = torch.clamp(self.cfg.max_grad_norm / (stats[7].sqrt() + 1e-6), max=1.0)
        torch._foreach_mul_([p.grad for p in self.params], coef)
        self.optimizer.step()

    def _randperm(self) -> torch.Tensor:
        return torch.randperm(self.cfg.batch_size, device=self.device, generator=self.generator)

    def _epochs_by_minibatch(self, batch, perms) -> list:
        """One host call (or ``grad_fn`` and ``apply_gradient``) per minibatch, one read of ``approx_kl`` per epoch with
        ``target_kl``; ``perms`` None: every epoch draws its permutation as it starts.  Returns what the log needs, on the device:
        the last step's statistics and the mean ``clipfrac``."""
        cfg = self.cfg
        one_step = _one_call_form(self.grad_fn, _ONE_CALL_TABLES[self.optimizer_kind][0]) if self.device_optimizer else None
        sizes = update_steps(cfg.batch_size, cfg.minibatch_size, cfg.norm_adv)
        clipfracs = []
        for e in range(cfg.update_epochs):
            if perms is None:
                perm = self._randperm()
                self.last_permutations.append(perm)
            else:
                perm = perms[e]
            start = 0
            for m in sizes:
                mb_inds = perm[start:start + m]
                start += cfg.minibatch_size
                noise = self.rpo_noise_fn(m) if self.rpo_noise_fn is not None else None
                if one_step is not None:
                    stats = one_step(self.net, batch, mb_inds, cfg, self.optimizer, rpo_noise=noise, seed=cfg.seed,
                                     draw_counter=self.minibatch_steps, stats=self.stats)
                else:
                    stats = self.grad_fn(self, batch, mb_inds, noise, self.minibatch_steps, self.stats)
                    self.apply_gradient(stats)
                self.minibatch_steps += 1
                clipfracs.append(stats[6].clone())
            if cfg.target_kl is not None and float(stats[5]) > cfg.target_kl:   # rpo_agent.py:282-284 (the one host read)
                break
        return [stats, torch.stack(clipfracs).mean().reshape(1)]

    def _epochs_one_call(self, batch, perms) -> list:
        """The whole update as one ``rpo_update`` (``deepsets_update`` for ``deepsets_kernel_grad``, ``transformer_update`` for
        ``transformer_kernel_grad`` with ``optimizer="device_transformer"``).  Returns what the log needs, on the device: the optimiser's header (16 words)
        and every step's statistics."""
        cfg = self.cfg
        sizes = update_steps(cfg.batch_size, cfg.minibatch_size, cfg.norm_adv)
        steps = cfg.update_epochs * len(sizes)
        noise = None
        if self.rpo_noise_fn is not None:
            noise = torch.zeros(steps, cfg.minibatch_size, 2, dtype=torch.float32, device=self.device)
            for k in range(steps):
                m = sizes[k % len(sizes)]
                noise[k, :m] = self.rpo_noise_fn(m)
        if self.stats_rows is None or self.stats_rows.shape[0] != steps:
            self.stats_rows = torch.zeros(steps, 8, dtype=torch.float32, device=self.device)
        update = _one_call_form(self.grad_fn, _ONE_CALL_TABLES[self.optimizer_kind][1])
        rows, header = update(self.net, batch, perms, cfg, self.optimizer, rpo_noise=noise, seed=cfg.seed,
                              first_draw_counter=self.minibatch_steps, stats=self.stats_rows)
        return [header.view(torch.float32), rows.reshape(-1)]

    def update(self) -> dict:
        cfg = self.cfg
        if cfg.anneal_lr:                                                     # rpo_agent.py:174-177
            frac = 1.0 - self.update_index / max(1, cfg.num_updates)
            self.optimizer.param_groups[0]["lr"] = frac * cfg.learning_rate
        storage = self.collect()
        batch = flatten_batch(storage, self.advantages, self.returns)
        device = self.device_optimizer
        one_call = device and self.one_call and _one_call_form(self.grad_fn, _ONE_CALL_TABLES[self.optimizer_kind][1]) is not None
        perms = torch.stack([self._randperm() for _ in range(cfg.update_epochs)]) if device else None
        self.last_permutations = list(perms) if device else []
        sent = self._epochs_one_call(batch, perms) if one_call else self._epochs_by_minibatch(batch, perms)
        self.update_index += 1
        # rpo_agent.py:286-299: the logged scalars (one transfer) and the finished episodes of this collection phase
        y_pred, y_true = batch["b_values"], batch["b_returns"]
        var_y = y_true.var(unbiased=False)
        ev = 1 - (y_true - y_pred).var(unbiased=False) / var_y
        host = torch.cat(sent + [ev.reshape(1), var_y.reshape(1)]).cpu()
        if one_call:
            ran = decode_header(host[:16])["steps_run"]
            rows = host[16:-2].reshape(-1, 8)
            self.minibatch_steps += ran
            last, clipfrac = rows[ran - 1].tolist(), float(rows[:ran, 6].mean())
        else:
            last, clipfrac = host[:8].tolist(), float(host[8])
        es = storage["episode_stats"]
        done = storage["dones"][1:].bool()                                    # (an episode that ended at step t shows in dones[t + 1])
        ended = torch.cat([done, storage["next_done"].bool()[None]], dim=0)
        recs = es[ended]
        sps = int(self.global_step / max(time.time() - self.start_time, 1e-9))
        return {"update": self.update_index, "global_step": self.global_step, "learning_rate": self.optimizer.param_groups[0]["lr"],
                "value_loss": last[2], "policy_loss": last[1], "entropy": last[3], "old_approx_kl": last[4], "approx_kl": last[5],
                "clipfrac": clipfrac, "explained_variance": float("nan") if float(host[-1]) == 0 else float(host[-2]), "loss": last[0],
                "SPS": sps, "episodes": {k: recs[:, i] for i, k in enumerate(STATS_FIELDS)}}

    def make_evaluator(self, num_envs: Optional[int] = None):
        """The ``PolicyEvaluator`` of ``evaluate``: the training env's configs, a handle and a batch of its own (``num_envs``:
        the training batch's size by default).  Kept until a different ``num_envs`` is asked for."""
        from .evaluation import PolicyEvaluator
        base = getattr(self.env, "env", self.env)
        n = base.num_envs if num_envs is None else int(num_envs)
        if self.evaluator is None or self.evaluator.num_envs != n:
            if self.evaluator is not None:
                self.evaluator.close()
            self.evaluator = PolicyEvaluator(base.env_config, base.wrap_config, num_envs=n, seed=base.seed_value, device=base.device)
        return self.evaluator

    def evaluate(self, n_episodes: int = 1, num_envs: Optional[int] = None, deterministic: bool = True, capture_envs: int = 0):
        """``n_episodes`` whole episodes per env of the current network on an evaluation batch of its own: the mean action
        (``deterministic``), the training env's observation statistics frozen at a copy of what they are now (when the
        training env normalises).  Nothing of the training env is touched.  Returns an ``EvaluationResult``; with
        ``capture_envs = K > 0`` it holds the frames of the batch's envs ``0..K-1`` (``EvaluationResult.episode_memory``)."""
        ev = self.make_evaluator(num_envs)
        kw = {}
        if hasattr(self.env, "norm_state"):
            kw = {"norm_state": self.env.norm_state.clone(), "obs_clip": self.env.obs_clip, "epsilon": self.env.epsilon}
        with torch.no_grad():
            return ev.evaluate(self.net, n_episodes, deterministic=deterministic, capture_envs=capture_envs, **kw)

    def learn(self, total_timesteps: Optional[int] = None, callback: Optional[Callable[[dict], None]] = None, *,
              eval_every: Optional[int] = None, eval_episodes: int = 1) -> list:
        """``num_updates`` updates (``total_timesteps // batch_size``); returns the list of their logged scalars.  Every
        ``eval_every`` updates ``log["eval"]`` holds the ``summary()`` of ``evaluate(eval_episodes)``."""
        n = self.cfg.num_updates if total_timesteps is None else int(total_timesteps) // self.cfg.batch_size
        logs = []
        for _ in range(n):
            log = self.update()
            if eval_every and self.update_index % int(eval_every) == 0:
                log["eval"] = self.evaluate(eval_episodes).summary()
            logs.append(log)
            if callback is not None:
                callback(log)
        return logs
