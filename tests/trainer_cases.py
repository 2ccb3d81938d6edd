"""What the GPU tests of the trainer (tests/test_gpu_trainer.py) and of the optimiser step (tests/test_gpu_optimizer.py) both
build: networks, loss settings, the branch-covering minibatch case, trainers on twin envs, the yardstick-driven ``grad_fn`` and
the comparison of words as integers."""
from tests import trainer_ref as R

DEV = "cuda:0"


def make_net(D, seed=0, dtype=None):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    torch.manual_seed(seed)
    net = LinearActorCritic(D)
    with torch.no_grad():           # visible means and values: a larger actor head, non-zero biases, two different sigmas
        net.actor_mean[4].weight.mul_(40.0)
        net.actor_logstd.copy_(torch.tensor([[-0.4, 0.2]]))
        for seq in (net.actor_mean, net.critic):
            for i in (0, 2, 4):
                seq[i].bias.uniform_(-0.2, 0.2)
    return net.to(DEV)


def make_initial_net(D, net_seed=0):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    torch.manual_seed(net_seed)
    return LinearActorCritic(D).to(DEV)


def loss_cfg(norm_adv=True, clip_vloss=True, ent_coef=0.0, rpo_alpha=0.5, clip_coef=0.2, vf_coef=0.5):
    from evacuation_amd.trainer import RPOTrainingConfig
    return RPOTrainingConfig(norm_adv=bool(norm_adv), clip_vloss=bool(clip_vloss), ent_coef=ent_coef, rpo_alpha=rpo_alpha,
                             clip_coef=clip_coef, vf_coef=vf_coef)


def build_case(D, M, mode, cfg, seed):
    """A batch whose minibatch takes every branch of the loss by a known share of its samples: the old log-probabilities and
    values are set FROM the float64 forward pass so that the ratio lies inside the clip range for half of the batch rows, above
    it for a quarter and below it for a quarter (advantages of both signs everywhere), and the value difference likewise around
    +-clip_coef -- each with a margin, so no sample is within 1e-6 of a branch point of max / clamp (checked, regenerated from
    another seed otherwise).  ``mode``: 'repeat' (indices drawn with repetition from a batch of M rows) or 'strided' (every second
    row of a batch of 2 M + 3)."""
    import torch
    c = cfg.clip_coef
    for attempt in range(8):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        net = make_net(D, seed=seed)
        B = max(M, 4) if mode == "repeat" else 2 * M + 3
        inds = torch.randint(0, B, (M,), generator=g) if mode == "repeat" else torch.arange(M) * 2 + 1
        obs = (0.6 * torch.randn(B, D, generator=g)).clamp(-1, 1)
        act = torch.randn(B, 2, generator=g)
        z = (torch.rand(M, 2, generator=g) * 2 - 1) * cfg.rpo_alpha
        # the float64 forward pass of every batch row, with the perturbation of the LAST minibatch position that reads the row
        zrow = torch.zeros(B, 2)
        zrow[inds] = z
        P = [p.detach().cpu().double() for p in R.mlp_tensors(net)]
        lp, _, val = R.logprob_entropy_value(P, obs.double(), act.double(), zrow.double())
        u = torch.rand(B, generator=g)
        mag = 0.25 + 0.35 * torch.rand(B, generator=g)                                    # |log ratio| in [0.25, 0.6]: ratio <= 0.78 or >= 1.28
        inside = (0.05 * torch.randn(B, generator=g)).clamp(-0.12, 0.12)
        target = torch.where(u < 0.5, inside, torch.where(u < 0.75, mag, -mag))
        logprobs = (lp - target.double()).float()
        u2 = torch.rand(B, generator=g)
        mag2 = c * (1.25 + torch.rand(B, generator=g))
        inside2 = c * (0.3 * torch.randn(B, generator=g)).clamp(-0.8, 0.8)
        dv = torch.where(u2 < 0.5, inside2, torch.where(u2 < 0.75, mag2, -mag2))
        values = (val.view(-1) - dv.double()).float()
        returns = (val.view(-1) + 0.7 * torch.randn(B, generator=g).double()).float()
        adv = torch.randn(B, generator=g) + 0.3
        batch = {"b_obs": obs, "b_actions": act, "b_logprobs": logprobs, "b_advantages": adv, "b_returns": returns, "b_values": values}
        batch = {k: v.to(DEV).contiguous() for k, v in batch.items()}
        inds, z = inds.to(DEV), z.to(DEV).contiguous()
        g64, s64, t = R.minibatch_grad(net, batch, inds, cfg, z, torch.float64)
        near = ((t.ratio - (1 - c)).abs() < 1e-6) | ((t.ratio - (1 + c)).abs() < 1e-6) | (t.adv.abs() < 1e-6)
        near |= ((t.dv.abs() - c).abs() < 1e-6)
        if cfg.clip_vloss:
            near |= ((t.dv.abs() > c) & ((t.v_unclipped - t.v_clipped).abs() < 1e-6))
        if not bool(near.any()):
            return net, batch, inds, z, g64, s64, t
    raise AssertionError("could not build a case without samples at a branch point")


def make_trainer(ea, n_ped, E, T, seed=1, net_seed=0, **kw):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig
    hooks = {k: kw.pop(k) for k in ("grad_fn", "rpo_noise_fn", "optimizer", "one_call") if k in kw}
    env_kw = {k: kw.pop(k) for k in ("max_timesteps",) if k in kw}
    cfg = RPOTrainingConfig(seed=seed, num_envs=E, num_steps=T, **kw)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=n_ped, **env_kw), ea.EnvWrappersConfig(positions="grav"), num_envs=E,
                                      gamma=cfg.gamma, seed=seed)
    torch.manual_seed(net_seed)
    net = LinearActorCritic(env.obs_dim).to(DEV)
    return RPOTrainer(env, net, cfg, **hooks)


def _yardstick_grad_fn(dtype, master=None):
    """``grad_fn`` of RPOTrainer with the yardstick + autograd in ``dtype``.  float32: the gradients go to ``.grad`` and the
    trainer clips and steps as ever.  float64: the loop is driven in float64 -- storage cast up, float64 master parameters with
    their own clipping and Adam(eps=1e-5), cast back into the network after each step; ``.grad`` is left zero, which makes the
    trainer's own step a no-op."""
    import torch

    def fn(trainer, batch, mb_inds, rpo_noise, draw_counter, stats):
        params = list(R.mlp_tensors(trainer.net))
        if dtype == torch.float32:
            grads, s, _ = R.minibatch_grad(trainer.net, batch, mb_inds, trainer.cfg, rpo_noise)
            for p, g in zip(params, grads):
                p.grad.copy_(g)
            stats.copy_(s)
            return stats
        if not master:
            master["p"] = [p.detach().double().clone().requires_grad_(True) for p in params]
            master["opt"] = torch.optim.Adam(master["p"], lr=trainer.cfg.learning_rate, eps=1e-5)
        master["opt"].param_groups[0]["lr"] = trainer.optimizer.param_groups[0]["lr"]
        b = {k: v.double() for k, v in batch.items()}
        t = R.loss_terms(master["p"], b, mb_inds, trainer.cfg, rpo_noise.double())
        master["opt"].zero_grad()
        t.loss.backward()
        torch.nn.utils.clip_grad_norm_(master["p"], trainer.cfg.max_grad_norm)
        master["opt"].step()
        with torch.no_grad():
            for p, m in zip(params, master["p"]):
                p.copy_(m)
                p.grad.zero_()
        stats.zero_()
        stats[6] = t.clipfrac
        return stats
    return fn


def bits(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def same_bits(a, b):
    import torch
    return torch.equal(bits(a), bits(b))
