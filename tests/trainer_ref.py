"""The yardstick of the trainer's update (evacuation_amd/trainer.py, csrc/evac_train.h): the reference's advantage estimation and
RPO loss (src/agents/rpo_agent.py:205-274, src/agents/networks/rpo_linear_agent_network.py:48-61) restated as functions of
tensors in torch -- dtype-generic, so the same lines run in float32 (the reference's precision) and in float64 (the truth the
kernels' errors are measured against) -- and differentiated by torch autograd.  tests/test_trainer_cpu.py pins it to the
reference's own network on the CPU."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from evacuation_amd.policy import mlp_tensors

NAMES = ("actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "actor_logstd",
         "critic_w1", "critic_b1", "critic_w2", "critic_b2", "critic_w3", "critic_b3")
STATS = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_sumsq")


def gae(rewards, values, dones, next_value, next_done, gamma: float, gae_lambda: float):
    """rpo_agent.py:205-220: advantages and returns [T, E] of storage rows [T, E] and the bootstrap [E].  ``gamma`` and
    ``gae_lambda`` stay Python floats, as the reference's: their product is formed in double."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = 0
    for t in range(T - 1, -1, -1):
        not_done = 1.0 - (next_done if t == T - 1 else dones[t + 1])
        v_next = next_value if t == T - 1 else values[t + 1]
        delta = rewards[t] + gamma * v_next * not_done - values[t]
        last = delta + gamma * gae_lambda * not_done * last
        adv[t] = last
    return adv, adv + values


def params_of(net, dtype=None, device=None):
    """The 13 tensors (``NAMES`` order) as fresh leaves that require grad."""
    return [t.detach().to(dtype=dtype or t.dtype, device=device or t.device).clone().requires_grad_(True) for t in mlp_tensors(net)]


def _mlp(x, w1, b1, w2, b2, w3, b3):
    h = torch.tanh(x @ w1.T + b1)
    h = torch.tanh(h @ w2.T + b2)
    return h @ w3.T + b3


def logprob_entropy_value(P, x, action, z):
    """get_action_and_value(x, action) (rpo_linear_agent_network.py:48-61) with the RPO perturbation ``z`` of the mean given
    (a constant): log-probability [M], entropy [M], value [M, 1]."""
    mean = _mlp(x, *P[0:6]) + z
    std = torch.exp(P[6].expand_as(mean))
    log_std = std.log()             # (torch's Normal takes the logarithm of its scale again)
    logprob = (-((action - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))).sum(1)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum(1)
    return logprob, entropy, _mlp(x, *P[7:13])


def loss_terms(P, batch, mb_inds, cfg, z):
    """rpo_agent.py:239-274 for one minibatch.  ``batch``: dict of b_obs, b_actions, b_logprobs, b_advantages, b_returns,
    b_values; ``cfg``: clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss.  Returns a namespace with the loss, its parts, the
    logged scalars and the per-sample quantities the tests place relative to the branch points."""
    x, act = batch["b_obs"][mb_inds], batch["b_actions"][mb_inds]
    logprob, entropy, value = logprob_entropy_value(P, x, act, z)
    logratio = logprob - batch["b_logprobs"][mb_inds]
    ratio = logratio.exp()
    with torch.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > cfg.clip_coef).to(ratio.dtype).mean()
    adv = batch["b_advantages"][mb_inds]
    if cfg.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg1 = -adv * ratio
    pg2 = -adv * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
    pg_loss = torch.max(pg1, pg2).mean()
    value = value.view(-1)
    ret, old_v = batch["b_returns"][mb_inds], batch["b_values"][mb_inds]
    if cfg.clip_vloss:
        unclipped = (value - ret) ** 2
        clipped = (old_v + torch.clamp(value - old_v, -cfg.clip_coef, cfg.clip_coef) - ret) ** 2
        v_loss = 0.5 * torch.max(unclipped, clipped).mean()
    else:
        unclipped = clipped = (value - ret) ** 2
        v_loss = 0.5 * unclipped.mean()
    ent = entropy.mean()
    loss = pg_loss - cfg.ent_coef * ent + v_loss * cfg.vf_coef
    return SimpleNamespace(loss=loss, pg_loss=pg_loss, v_loss=v_loss, entropy=ent, old_approx_kl=old_approx_kl, approx_kl=approx_kl,
                           clipfrac=clipfrac, ratio=ratio.detach(), adv=adv.detach(), dv=(value - old_v).detach(),
                           pg1=pg1.detach(), pg2=pg2.detach(), v_unclipped=unclipped.detach(), v_clipped=clipped.detach())


def minibatch_grad(net, batch, mb_inds, cfg, z, dtype=torch.float32):
    """Gradients of the 13 tensors (list, ``NAMES`` order) and the 8 statistics (``STATS`` order) of one minibatch, everything
    cast to ``dtype`` first, by autograd."""
    P = params_of(net, dtype)
    b = {k: v.to(dtype) for k, v in batch.items()}
    t = loss_terms(P, b, mb_inds, cfg, z.to(dtype))
    grads = torch.autograd.grad(t.loss, P)
    sumsq = sum((g.double() ** 2).sum() for g in grads).to(dtype)
    stats = torch.stack([t.loss.detach(), t.pg_loss.detach(), t.v_loss.detach(), t.entropy.detach(), t.old_approx_kl, t.approx_kl,
                         t.clipfrac, sumsq])
    return list(grads), stats, t
