"""What the GPU tests of the trainer (tests/test_gpu_trainer.py) and of the optimiser step (tests/test_gpu_optimizer.py) both
build: networks, loss settings, the branch-covering minibatch case, trainers on twin envs, the yardstick-driven ``grad_fn`` and
the comparison of words as integers."""
from tests import encoder_grad_cases as G
from tests import trainer_ref as R

DEV = "cuda:0"


def make_net(D, seed=0, dtype=None, device=DEV):
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
    return net.to(device)


def make_initial_net(D, net_seed=0):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    torch.manual_seed(net_seed)
    return LinearActorCritic(D).to(DEV)


def loss_cfg(norm_adv=True, clip_vloss=True, ent_coef=0.0, rpo_alpha=0.5, clip_coef=0.2, vf_coef=0.5):
    from evacuation_amd.trainer import RPOTrainingConfig
    return RPOTrainingConfig(norm_adv=bool(norm_adv), clip_vloss=bool(clip_vloss), ent_coef=ent_coef, rpo_alpha=rpo_alpha,
                             clip_coef=clip_coef, vf_coef=vf_coef)


def build_case(D, M, mode, cfg, seed, device=DEV):
    """A batch whose minibatch takes every branch of the loss by a known share of its samples: the old log-probabilities and
    values are set FROM the float64 forward pass so that the ratio lies inside the clip range for half of the batch rows, above
    it for a quarter and below it for a quarter (advantages of both signs everywhere), and the value difference likewise around
    +-clip_coef -- each with a margin, so no sample is within 1e-6 of a branch point of max / clamp (checked, regenerated from
    another seed otherwise).  ``mode``: 'repeat' (indices drawn with repetition from a batch of M rows) or 'strided' (every second
    row of a batch of 2 M + 3)."""
    def encode64(net, obs, g):                       # (no encoder: nothing to redraw, the actor-critic reads the observation)
        return [p.detach().cpu().double() for p in R.mlp_tensors(net)], obs.double(), None
    return G.build_case(D, M, mode, cfg, seed, device, lambda: make_net(D, seed=seed, device=device), encode64, R.minibatch_grad)


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
