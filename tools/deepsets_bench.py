#!/usr/bin/env python3
"""Measure the deep-sets leader's collection phase (evac_policy_rollout_deepsets) against what it stands beside and what it
replaces, its minibatch gradient on the device (evac_deepsets_minibatch_grad) against autograd's, and one whole update's epochs
with torch's optimiser against the device's (evac_deepsets_minibatch_step, evac_deepsets_update).

    python tools/deepsets_bench.py --part a|b|c|c-eager|grad-autograd|grad-device|step-device|update-torch|update-step|update-one-call
                                   [--envs 4096] [--steps 128] [--minibatch 16384] [--epochs 10] [--reps 7]
    python tools/deepsets_bench.py --part update-sweep|collect-sweep --learners S --envs 3 --steps 2048 --minibatch 192
                                   (a configuration per learner against the one-configuration population: tools/encoder_sweep_bench.py)
    python tools/deepsets_bench.py --part update-population --learners S [--envs 3] [--steps 2048] [--minibatch 192] [--epochs 10]

N = 60, the rel + ohe Box observation (D = 372), the trainer's normalisation chain, E envs, T steps per call; hipEvent times of
whole calls after two warm-up calls, median and range of ``--reps`` calls, one JSON line:
  a        ``policy_rollout`` of the linear network (``LinearActorCritic``): one launch
  b        ``policy_rollout`` of ``DeepSetsActorCritic``: one launch
  c        what b replaces: per step the module's torch forward (``get_action_and_value``, written out) and ``step(out_*=)`` into the
           trainer's storage, the T steps captured into a graph once and replayed (as examples/rollout_with_policy.py)
  c-eager  the same loop launched step by step
  grad-autograd  one minibatch gradient of ``DeepSetsActorCritic`` by ``trainer.autograd_minibatch_grad`` at the trainer's shape: a
           batch of E x T rows, a minibatch of ``--minibatch`` (16 384) of them from a permutation, injected noise
  grad-device    the same by ``trainer.deepsets_minibatch_grad`` (six launches)
  step-device    the same followed by clip + Adam over the 19 tensors, one call (``trainer.deepsets_minibatch_step``: seven launches);
           minus grad-device it is the Adam stage alone
  update-torch   one whole update's epochs (``--epochs`` x B / minibatch steps over the E x T batch, the perturbation drawn on the
           device): per minibatch ``deepsets_minibatch_grad``, the ``foreach`` clip and ``torch.optim.Adam.step()``, as
           ``RPOTrainer(grad_fn=deepsets_kernel_grad)`` does; events around the whole loop after one warm-up update
  update-step    the same with one ``deepsets_minibatch_step`` per minibatch (``DeviceAdam``)
  update-one-call  the same as one ``deepsets_update``
  update-population  one whole ``update()`` -- collection, advantages, permutations, every epoch's minibatch steps -- of
           ``PopulationTrainer(env, DeepSetsPopulation(S learners), cfg)`` (``--envs`` envs PER LEARNER) against the loop of S lone
           ``RPOTrainer(grad_fn=deepsets_kernel_grad, optimizer="device", one_call=True)`` updates on twin handles: wall-clock
           times of whole updates between synchronisations (an update ends with its own host transfer) after two warm-up updates
           of each form, the two forms alternated inside every repetition, median and range of ``--reps`` repetitions
One part per process, so that a job script can give each its own time limit."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evacuation_amd as ea  # noqa: E402
from evacuation_amd.policy import DeepSetsActorCritic, LinearActorCritic  # noqa: E402

DEV = torch.device("cuda:0")
N_PED = 60
LOG_SQRT_2PI = 0.9189385332046727


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_batch(args):
    """The network, the configuration and a random batch of E x T rows at the trainer's shape."""
    from evacuation_amd import trainer
    E, T = args.envs, args.steps
    D, B = (N_PED + 2) * 6, E * T
    torch.manual_seed(0)
    net = DeepSetsActorCritic(D, N_PED).to(DEV)
    cfg = trainer.RPOTrainingConfig(num_envs=E, num_steps=T)
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    batch = {"b_obs": rnd(B, D).clamp(-5, 5), "b_actions": rnd(B, 2), "b_logprobs": -2.0 + 0.1 * rnd(B), "b_advantages": rnd(B),
             "b_returns": rnd(B), "b_values": rnd(B)}
    return net, cfg, batch, g


def update_part(args):
    """One whole update's epochs, three ways: whole updates between two events after one warm-up update."""
    from evacuation_amd import trainer
    net, cfg, batch, g = make_batch(args)
    B, M = args.envs * args.steps, args.minibatch
    perms = torch.stack([torch.randperm(B, device=DEV, generator=g) for _ in range(args.epochs)]).contiguous()
    sizes = trainer.update_steps(B, M, cfg.norm_adv)
    steps = args.epochs * len(sizes)
    params = list(trainer.all_tensors(net))
    trainer.ensure_grads(net)
    stats, rows = torch.zeros(8, device=DEV), torch.zeros(steps, 8, device=DEV)
    if args.part == "update-torch":
        opt = torch.optim.Adam(params, lr=cfg.learning_rate, eps=1e-5)

        def step(inds, k):
            trainer.deepsets_minibatch_grad(net, batch, inds, cfg, seed=1, draw_counter=k, stats=stats)
            coef = torch.clamp(cfg.max_grad_norm / (stats[7].sqrt() + 1e-6), max=1.0)       # RPOTrainer.apply_gradient
            torch._foreach_mul_([p.grad for p in params], coef)
            opt.step()
    else:
        opt = trainer.DeviceAdam(net, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm)

        def step(inds, k):
            trainer.deepsets_minibatch_step(net, batch, inds, cfg, opt, seed=1, draw_counter=k, stats=stats)

    def run():
        if args.part == "update-one-call":
            trainer.deepsets_update(net, batch, perms, cfg, opt, seed=1, first_draw_counter=0, stats=rows, minibatch_size=M)
            return
        k = 0
        for e in range(args.epochs):
            start = 0
            for m in sizes:
                step(perms[e, start:start + m], k)
                start += M
                k += 1
    run()
    torch.cuda.synchronize()
    ms = [event_ms(run) for _ in range(max(3, args.reps))]
    med = statistics.median(ms)
    print(json.dumps({"part": args.part, "envs": args.envs, "steps": args.steps, "batch": B, "minibatch": M, "epochs": args.epochs,
                      "minibatch_steps": steps, "ms_per_update_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "us_per_minibatch_step": round(med / steps * 1e3, 2), "updates": len(ms),
                      "finite": bool(all(torch.isfinite(p).all() for p in params))}))


def population_part(args):
    """One population update against the per-learner loop, collection included; see the module's docstring."""
    import dataclasses
    import time

    from evacuation_amd.population import DeepSetsPopulation, PopulationTrainer
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig, deepsets_kernel_grad, update_steps
    S, E_l, T = args.learners, args.envs, args.steps
    cfg = RPOTrainingConfig(num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 1000, num_minibatches=max(1, E_l * T // args.minibatch),
                            update_epochs=args.epochs)
    env_cfg = ea.EnvConfig(number_of_pedestrians=N_PED)
    wrap = ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box")
    seeds = list(range(1, S + 1))
    env = ea.NormalizedVectorEnv.make(env_cfg, wrap, num_envs=S * E_l, gamma=cfg.gamma, seed=1)
    ptr = PopulationTrainer(env, DeepSetsPopulation(env.obs_dim, N_PED, seeds, DEV), cfg)
    lone = []
    for s, seed in enumerate(seeds):
        e = ea.NormalizedVectorEnv.make(env_cfg, wrap, num_envs=E_l, gamma=cfg.gamma, seed=1, env_id_offset=s * E_l)
        torch.manual_seed(seed)
        lone.append(RPOTrainer(e, DeepSetsActorCritic(e.obs_dim, N_PED).to(DEV), dataclasses.replace(cfg, seed=seed),
                               grad_fn=deepsets_kernel_grad, optimizer="device", one_call=True))

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def loop():
        for tr in lone:
            tr.update()
    for _ in range(2):
        ptr.update()
        loop()
    pop_ms, loop_ms = [], []
    for _ in range(max(3, args.reps)):
        pop_ms.append(wall_ms(ptr.update))
        loop_ms.append(wall_ms(loop))
    pm, lm = statistics.median(pop_ms), statistics.median(loop_ms)
    steps = cfg.update_epochs * len(update_steps(cfg.batch_size, cfg.minibatch_size, cfg.norm_adv))
    finite = all(bool(torch.isfinite(t).all()) for t in ptr.population.tensors)
    print(json.dumps({"part": args.part, "learners": S, "envs_per_learner": E_l, "steps": T, "minibatch": cfg.minibatch_size,
                      "epochs": cfg.update_epochs, "minibatch_steps": steps, "obs_dim": env.obs_dim,
                      "population_ms_median": round(pm, 3), "population_ms_min": round(min(pop_ms), 3), "population_ms_max": round(max(pop_ms), 3),
                      "loop_ms_median": round(lm, 3), "loop_ms_min": round(min(loop_ms), 3), "loop_ms_max": round(max(loop_ms), 3),
                      "loop_over_population": round(lm / pm, 3), "updates": len(pop_ms), "finite": finite}))
    for tr in lone:
        tr.env.close()
    env.close()


def grad_part(args):
    """One minibatch gradient of all 19 tensors (step-device: and the optimiser's step): whole calls between two events after two
    warm-up calls."""
    from types import SimpleNamespace

    from evacuation_amd import trainer
    E, T, M = args.envs, args.steps, args.minibatch
    D, B = (N_PED + 2) * 6, E * T
    net, cfg, batch, g = make_batch(args)
    inds = torch.randperm(B, device=DEV, generator=g)[:M].contiguous()
    z = ((torch.rand(M, 2, device=DEV, generator=g) * 2 - 1) * cfg.rpo_alpha).contiguous()
    stats = torch.zeros(8, device=DEV)
    holder = SimpleNamespace(net=net, cfg=cfg)
    trainer.ensure_grads(net)
    if args.part == "grad-device":
        def run():
            trainer.deepsets_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
    elif args.part == "step-device":
        opt = trainer.DeviceAdam(net, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm)

        def run():
            trainer.deepsets_minibatch_step(net, batch, inds, cfg, opt, rpo_noise=z, stats=stats)
    else:
        def run():
            trainer.autograd_minibatch_grad(holder, batch, inds, z, 0, stats)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = [event_ms(run) for _ in range(max(5, args.reps))]
    med = statistics.median(ms)
    print(json.dumps({"part": args.part, "envs": E, "steps": T, "batch": B, "minibatch": M, "obs_dim": D, "ms_per_call_median": round(med, 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "grad_sumsq": float(stats[7]), "calls": len(ms)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["a", "b", "c", "c-eager", "grad-autograd", "grad-device", "step-device", "update-torch",
                                                     "update-step", "update-one-call", "update-population", "update-sweep",
                                                     "collect-sweep"])
    ap.add_argument("--learners", type=int, default=4, help="update-population: the learners of the population")
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=10, help="update-*: the epochs of one update")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.part in ("update-sweep", "collect-sweep"):               # (tools/encoder_sweep_bench.py: shared with transformer_bench.py)
        import encoder_sweep_bench
        part = encoder_sweep_bench.collect_sweep_part if args.part == "collect-sweep" else encoder_sweep_bench.update_sweep_part
        return part(args, "deepsets")
    if args.part == "update-population":
        return population_part(args)
    if args.part.startswith("update-"):
        return update_part(args)
    if args.part.startswith("grad-") or args.part == "step-device":
        return grad_part(args)
    E, T = args.envs, args.steps
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=N_PED), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                      num_envs=E, gamma=0.99, seed=1)
    D = env.obs_dim
    torch.manual_seed(0)
    net = (LinearActorCritic(D) if args.part == "a" else DeepSetsActorCritic(D, N_PED)).to(DEV)
    first, _ = env.reset()
    if args.part in ("a", "b"):
        next_obs, next_done = first.clone(), torch.zeros(E, dtype=torch.float32, device=DEV)
        with torch.no_grad():
            out = env.policy_rollout(net, T, next_obs, next_done)

        def run():
            env.policy_rollout(net, T, next_obs, next_done, out=out)
    else:
        obs = torch.zeros((T + 1, E, D), device=DEV)
        actions, logprobs = torch.zeros((T, E, 2), device=DEV), torch.zeros((T, E), device=DEV)
        values, rewards = torch.zeros((T, E), device=DEV), torch.zeros((T, E), device=DEV)
        terminated, truncated = torch.zeros((T, E), dtype=torch.uint8, device=DEV), torch.zeros((T, E), dtype=torch.uint8, device=DEV)
        obs[0].copy_(first)

        with torch.no_grad():
            std = torch.exp(net.actor_logstd)

        def loop():
            with torch.no_grad():
                for t in range(T):
                    # get_action_and_value(obs[t]) written out (torch's Normal checks its arguments on the host, which a
                    # capture does not allow): the encoder, both heads, the sample and its log-probability
                    y = net.encode(obs[t])
                    mean = net.actor_mean(y)
                    torch.addcmul(mean, std, torch.randn_like(mean), out=actions[t])
                    torch.sum(-((actions[t] - mean) ** 2) / (2 * std * std) - net.actor_logstd - LOG_SQRT_2PI, dim=1, out=logprobs[t])
                    values[t].copy_(net.critic(y).view(-1))
                    env.step(actions[t], out_obs=obs[t + 1], out_reward=rewards[t], out_terminated=terminated[t], out_truncated=truncated[t])
                obs[0].copy_(obs[T])
        loop()
        torch.cuda.synchronize()
        run = loop
        if args.part == "c":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    loop()
            torch.cuda.current_stream().wait_stream(side)
            run = g.replay
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = [event_ms(run) for _ in range(max(5, args.reps))]
    med = statistics.median(ms)
    print(json.dumps({"part": args.part, "envs": E, "steps": T, "obs_dim": D, "ms_per_call_median": round(med, 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "us_per_vector_step": round(med / T * 1e3, 3),
                      "env_steps_per_s": round(E * T / (med * 1e-3), 1), "calls": len(ms)}))
    env.close()


if __name__ == "__main__":
    main()
