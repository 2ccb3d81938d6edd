"""The reference trainer's update on the device: the other half of ``RPOAgent.learn()`` (src/agents/rpo_agent.py:172-299).

``policy_rollout`` fills the trainer's storage in one launch; this module does what the reference does with it afterwards:
``gae`` (rpo_agent.py:205-220, ``evac_gae``: one launch), ``rpo_minibatch_grad`` (rpo_agent.py:239-277 up to and including
``loss.backward()``, ``evac_rpo_minibatch_grad``: at most three launches, deterministic) and ``RPOTrainer``, one iteration of the
reference's loop per ``update()``.  Gradient clipping and Adam stay torch (they work on ``.grad`` in place)."""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch

from . import _lib
from .policy import PolicyBinder, mlp_tensors
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


def gae(storage: Dict[str, torch.Tensor], gamma: float, gae_lambda: float, out=None):
    """Advantages and returns [T, E] of the storage ``policy_rollout`` returns (rpo_agent.py:205-220), one launch, bit-equal to
    the reference's loop in float32.  ``out`` = (advantages, returns) to reuse."""
    rewards = storage["rewards"]
    T, E = rewards.shape
    rewards = _f32(rewards, (T, E), "rewards")
    values, dones = _f32(storage["values"], (T, E), "values"), _f32(storage["dones"], (T, E), "dones")
    next_value, next_done = _f32(storage["next_value"], (E,), "next_value"), _f32(storage["next_done"], (E,), "next_done")
    if out is None:
        out = (torch.empty_like(rewards), torch.empty_like(rewards))
    adv, ret = _f32(out[0], (T, E), "advantages"), _f32(out[1], (T, E), "returns")
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


class _GradState:
    """What ``rpo_minibatch_grad`` keeps per network: the binder, the ``.grad`` tensors' addresses and the workspace."""

    def __init__(self):
        self.binder = None
        self.grads_key = None
        self.grads_struct = None
        self.workspace = None


def _grad_state(net) -> _GradState:
    st = getattr(net, "_evac_grad_state", None)
    if st is None:
        st = _GradState()
        object.__setattr__(net, "_evac_grad_state", st)
    return st


def ensure_grads(net) -> "_lib.EvacMlpPolicyGrads":
    """Every parameter gets a contiguous float32 ``.grad`` on its device (allocated once, then reused: torch's optimisers update
    in place); their addresses as ``evac_mlp_policy_grads_t``."""
    st = _grad_state(net)
    ts = mlp_tensors(net)
    for t in ts:
        g = t.grad
        if g is None or g.dtype != torch.float32 or g.device != t.device or not g.is_contiguous() or g.shape != t.shape:
            t.grad = torch.zeros_like(t, memory_format=torch.contiguous_format)
    key = tuple(t.grad.data_ptr() for t in ts)
    if key != st.grads_key:
        st.grads_struct, st.grads_key = _lib.EvacMlpPolicyGrads(*key), key
    return st.grads_struct


def rpo_minibatch_grad(net, batch: Dict[str, torch.Tensor], mb_inds: torch.Tensor, cfg, *, rpo_noise: Optional[torch.Tensor] = None,
                       seed: int = 0, draw_counter: int = 0, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of the RPO loss of the minibatch ``mb_inds`` of ``batch`` (``flatten_batch``) into the parameters' ``.grad``
    (written, not accumulated), by ``evac_rpo_minibatch_grad``; returns the 8 statistics (``STAT_NAMES``) as a device tensor.
    ``cfg``: an ``RPOTrainingConfig`` (or anything with its loss fields).  ``rpo_noise`` [M, 2] injects the RPO perturbation;
    None draws it on the device from (``seed``, ``draw_counter``).  No host synchronisation; capturable into a graph."""
    b_obs = batch["b_obs"]
    B, D = b_obs.shape
    dev = b_obs.device
    _f32(b_obs, (B, D), "b_obs")
    _f32(batch["b_actions"], (B, 2), "b_actions")
    for k in BATCH_KEYS[2:]:
        _f32(batch[k], (B,), k)
    if mb_inds.dtype != torch.int64 or mb_inds.device != dev or not mb_inds.is_contiguous() or mb_inds.dim() != 1:
        raise ValueError("mb_inds: expected a contiguous int64 device vector")
    M = int(mb_inds.shape[0])
    if rpo_noise is not None:
        _f32(rpo_noise, (M, 2), "rpo_noise")
    st = _grad_state(net)
    if st.binder is None or st.binder.obs_dim != D or st.binder.device != dev:
        st.binder = PolicyBinder(D, dev)
    pol = st.binder(net)
    grads = ensure_grads(net)
    lib = _lib.load()
    need = int(lib.evac_rpo_workspace_bytes(D, M))
    if need < 0:
        raise _lib.EvacError(need, f"evac_rpo_workspace_bytes({D}, {M})")
    if st.workspace is None or st.workspace.numel() < need or st.workspace.device != dev:
        st.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=dev)
    else:
        _f32(stats, (8,), "stats")
    lc = cfg.loss_config() if hasattr(cfg, "loss_config") else RPOTrainingConfig.loss_config(cfg)
    rc = lib.evac_rpo_minibatch_grad(C.byref(pol), C.byref(lc), B, _ptr(b_obs), _ptr(batch["b_actions"]), _ptr(batch["b_logprobs"]),
                                     _ptr(batch["b_advantages"]), _ptr(batch["b_returns"]), _ptr(batch["b_values"]), M,
                                     _ptr(mb_inds), _ptr(rpo_noise), int(seed) & (2 ** 64 - 1), int(draw_counter) & (2 ** 64 - 1),
                                     C.byref(grads), _ptr(stats), _ptr(st.workspace), _stream(dev))
    _lib.check(rc)
    return stats


def _kernel_grad(trainer: "RPOTrainer", batch, mb_inds, rpo_noise, draw_counter: int, stats: torch.Tensor) -> torch.Tensor:
    return rpo_minibatch_grad(trainer.net, batch, mb_inds, trainer.cfg, rpo_noise=rpo_noise, seed=trainer.cfg.seed,
                              draw_counter=draw_counter, stats=stats)


class RPOTrainer:
    """One iteration of the reference's training loop (rpo_agent.py:172-299) per ``update()``: learning-rate annealing, the
    collection phase (``policy_rollout``), ``gae``, ``update_epochs`` x ``num_minibatches`` steps of gradient (kernel),
    ``clip_grad_norm_`` (from the kernel's sum of squares) and ``Adam(eps=1e-5)``, the ``target_kl`` early exit.

    ``env``: a ``NormalizedVectorEnv`` (the trainer's wrapper chain) or a ``BatchedEvacuationEnv`` with ``cfg.num_envs`` envs.
    The permutation of every epoch is drawn on the device from a generator seeded with ``cfg.seed`` (the reference shuffles on
    the host).  ``grad_fn(trainer, batch, mb_inds, rpo_noise, draw_counter, stats)`` computes the gradient of one minibatch into
    the parameters' ``.grad`` and returns the 8 statistics: the kernel by default.  ``rpo_noise_fn(M)`` -> [M, 2] injects the
    RPO perturbation (default: drawn inside the kernel)."""

    def __init__(self, env, net, cfg: RPOTrainingConfig, *, grad_fn: Optional[Callable] = None,
                 rpo_noise_fn: Optional[Callable[[int], torch.Tensor]] = None):
        cfg.check()
        if env.num_envs != cfg.num_envs:
            raise ValueError(f"RPOTrainer: the env has {env.num_envs} envs, cfg.num_envs = {cfg.num_envs}")
        self.env, self.net, self.cfg = env, net, cfg
        self.grad_fn = grad_fn or _kernel_grad
        self.rpo_noise_fn = rpo_noise_fn
        self.params = list(mlp_tensors(net))
        self.device = self.params[0].device
        ensure_grads(net)
        self.optimizer = torch.optim.Adam(self.params, lr=cfg.learning_rate, eps=1e-5)
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
        coef = torch.clamp(self.cfg.max_grad_norm / (stats[7].sqrt() + 1e-6), max=1.0)
        torch._foreach_mul_([p.grad for p in self.params], coef)
        self.optimizer.step()

    def update(self) -> dict:
        cfg = self.cfg
        if cfg.anneal_lr:                                                     # rpo_agent.py:174-177
            frac = 1.0 - self.update_index / max(1, cfg.num_updates)
            self.optimizer.param_groups[0]["lr"] = frac * cfg.learning_rate
        storage = self.collect()
        batch = flatten_batch(storage, self.advantages, self.returns)
        B, M = cfg.batch_size, cfg.minibatch_size
        clipfracs = []
        self.last_permutations = []
        for _ in range(cfg.update_epochs):
            perm = torch.randperm(B, device=self.device, generator=self.generator)
            self.last_permutations.append(perm)
            for start in range(0, B, M):
                mb_inds = perm[start:start + M]
                if mb_inds.shape[0] < (2 if cfg.norm_adv else 1):
                    continue
                noise = self.rpo_noise_fn(int(mb_inds.shape[0])) if self.rpo_noise_fn is not None else None
                stats = self.grad_fn(self, batch, mb_inds, noise, self.minibatch_steps, self.stats)
                self.minibatch_steps += 1
                self.apply_gradient(stats)
                clipfracs.append(stats[6].clone())
            if cfg.target_kl is not None and float(stats[5]) > cfg.target_kl:   # rpo_agent.py:282-284 (the one host read)
                break
        self.update_index += 1
        # rpo_agent.py:286-299: the logged scalars (one transfer) and the finished episodes of this collection phase
        y_pred, y_true = batch["b_values"], batch["b_returns"]
        var_y = y_true.var(unbiased=False)
        ev = 1 - (y_true - y_pred).var(unbiased=False) / var_y
        host = torch.cat([stats, torch.stack(clipfracs).mean().reshape(1), ev.reshape(1), var_y.reshape(1)]).tolist()
        es = storage["episode_stats"]
        done = storage["dones"][1:].bool()                                    # (an episode that ended at step t shows in dones[t + 1])
        ended = torch.cat([done, storage["next_done"].bool()[None]], dim=0)
        recs = es[ended]
        sps = int(self.global_step / max(time.time() - self.start_time, 1e-9))
        return {"update": self.update_index, "global_step": self.global_step, "learning_rate": self.optimizer.param_groups[0]["lr"],
                "value_loss": host[2], "policy_loss": host[1], "entropy": host[3], "old_approx_kl": host[4], "approx_kl": host[5],
                "clipfrac": host[8], "explained_variance": float("nan") if host[10] == 0 else host[9], "loss": host[0], "SPS": sps,
                "episodes": {k: recs[:, i] for i, k in enumerate(STATS_FIELDS)}}

    def learn(self, total_timesteps: Optional[int] = None, callback: Optional[Callable[[dict], None]] = None) -> list:
        """``num_updates`` updates (``total_timesteps // batch_size``); returns the list of their logged scalars."""
        n = self.cfg.num_updates if total_timesteps is None else int(total_timesteps) // self.cfg.batch_size
        logs = []
        for _ in range(n):
            log = self.update()
            logs.append(log)
            if callback is not None:
                callback(log)
        return logs
