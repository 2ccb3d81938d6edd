#!/usr/bin/env python3
"""Measure the transformer leader's collection phase (evac_policy_rollout_transformer) against what it stands beside and what it
replaces.

    python tools/transformer_bench.py --part a|b|c|c-eager [--envs 4096] [--steps 128] [--blocks 2] [--use-resid] [--reps 7]
    python tools/transformer_bench.py --part grad-autograd|grad-device [--minibatch 16384] [--blocks 2] [--use-resid] [--reps 7]
    python tools/transformer_bench.py --part update-torch|update-step|update-one-call [--envs 4096] [--steps 128] [--epochs 10]
    python tools/transformer_bench.py --part collect-population --learners S [--learner-envs 3] [--steps 2048] [--pairs 9]
    python tools/transformer_bench.py --part update-sweep|collect-sweep --learners S [--learner-envs 3] [--steps 2048] [--minibatch 192]
                                   (a configuration per learner against the one-configuration population: tools/encoder_sweep_bench.py)
    python tools/transformer_bench.py --part update-population --learners S [--learner-envs 3] [--steps 2048] [--minibatch 192]
                                      [--epochs 10] [--pairs 9]

N = 60, the rel + ohe Box observation (D = 372, 62 tokens of 6), the trainer's normalisation chain, E envs, T steps per call;
hipEvent times of whole calls after two warm-up calls, median and range of ``--reps`` calls, one JSON line:
  a        ``policy_rollout`` of the linear network (``LinearActorCritic``): one launch
  b        ``policy_rollout`` of ``TransformerActorCritic``: one launch
  c        what b replaces: per step the module's torch forward (``get_action_and_value``, written out) and ``step(out_*=)`` into the
           trainer's storage, the T steps captured into a graph once and replayed (as examples/rollout_with_policy.py)
  c-eager  the same loop launched step by step
  grad-autograd  one minibatch gradient of the 13 + 16 per block tensors by ``trainer.autograd_minibatch_grad`` (torch autograd on
           the module): M = ``--minibatch`` samples of a batch of 2 M observations drawn as 0.6 randn clamped to +-1, no env
  grad-device    the same gradient by ``trainer.transformer_minibatch_grad`` (``evac_transformer_minibatch_grad``: 5 + blocks +
           norm_adv launches)
  update-torch   one whole update's epochs (``--epochs`` x B / minibatch steps over a random batch of E x T rows, the perturbation
           drawn on the device): per minibatch ``transformer_minibatch_grad``, the ``foreach`` clip and
           ``torch.optim.Adam.step()``, as ``RPOTrainer(grad_fn=transformer_kernel_grad)`` does; events around the whole loop
           after one warm-up update
  update-step    the same with one ``transformer_minibatch_step`` per minibatch (``TransformerAdam``)
  update-one-call  the same as one ``transformer_update``
  collect-population  the collection phase of S learners (``--learners``) of ``--learner-envs`` envs and ``--steps`` steps each (the
           reference's 3 x 2048 by default): ONE ``policy_rollout_population`` of a ``TransformerPopulation`` on a handle of S E_l
           envs (``evac_policy_rollout_population_transformer``) against the loop of S ``policy_rollout(nets[s])`` on handles of E_l
           envs at the learners' ids (``evac_policy_rollout_transformer``), the same nets; one warm-up of each, the first calls'
           storage compared bit for bit, then ``--pairs`` interleaved pairs whose order alternates: hipEvent and host wall time
  update-population  one whole update of S learners (``--learners``) of ``--learner-envs`` x ``--steps`` rows each (the reference's
           3 x 2048 by default) in minibatches of ``--minibatch`` (192 by default here) over ``--epochs`` epochs: ONE
           ``transformer_update_population`` of a ``TransformerPopulation`` (``evac_transformer_update_population``) against the
           loop of S ``transformer_update`` calls (``evac_transformer_update``), one per learner on a batch of its own that holds
           its rows of the common random batch, with the same permutations, seeds and draw counters; both forms start from the same tensors and
           the first updates' parameters are compared bit for bit, then ``--pairs`` interleaved pairs whose order alternates:
           hipEvent and host wall time
One part per process, so that a job script can give each its own time limit."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evacuation_amd as ea  # noqa: E402
from evacuation_amd.policy import LinearActorCritic, TransformerActorCritic  # noqa: E402

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


def grad_part(args):
    """One minibatch gradient at N = 60, rel + ohe Box (D = 372): hipEvent median and range after warm-up, one JSON line."""
    from types import SimpleNamespace
    from evacuation_amd import trainer
    D, M = (N_PED + 2) * 6, args.minibatch
    B = 2 * M
    torch.manual_seed(0)
    net = TransformerActorCritic(D, N_PED, num_blocks=args.blocks, use_resid=args.use_resid).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    rand = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    batch = {"b_obs": (0.6 * rand(B, D)).clamp(-1, 1), "b_actions": rand(B, 2), "b_logprobs": -2.0 + 0.3 * rand(B),
             "b_advantages": rand(B), "b_returns": rand(B), "b_values": rand(B)}
    inds = torch.randperm(B, device=DEV, generator=g)[:M].contiguous()
    z = (torch.rand(M, 2, device=DEV, generator=g) * 2 - 1) * 0.5
    cfg = trainer.RPOTrainingConfig()
    stats = torch.zeros(8, device=DEV)
    if args.part == "grad-device":
        def run():
            trainer.transformer_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
        launches = 5 + args.blocks + int(cfg.norm_adv)
    else:
        fake = SimpleNamespace(net=net, cfg=cfg)

        def run():
            trainer.autograd_minibatch_grad(fake, batch, inds, z, 0, stats)
        launches = None
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = [event_ms(run) for _ in range(max(5, args.reps))]
    med = statistics.median(ms)
    print(json.dumps({"part": args.part, "minibatch": M, "obs_dim": D, "blocks": args.blocks, "use_resid": bool(args.use_resid),
                      "ms_per_call_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "launches": launches, "loss": round(float(stats[0]), 6), "grad_sumsq": float(stats[7]), "calls": len(ms)}))


def collect_population_part(args):
    """S learners' collection in one launch against the per-learner loop of the lone entry, interleaved; one JSON line."""
    import time
    from evacuation_amd.population import TransformerPopulation
    S, E_l, T = args.learners, args.learner_envs, args.steps or 2048
    cfg, wrap = ea.EnvConfig(number_of_pedestrians=N_PED), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box")
    make = lambda E, offset: ea.NormalizedVectorEnv.make(cfg, wrap, num_envs=E, gamma=0.99, seed=1, env_id_offset=offset)
    every, lone = make(S * E_l, 0), [make(E_l, s * E_l) for s in range(S)]
    D = every.obs_dim
    pop = TransformerPopulation(D, N_PED, list(range(1, S + 1)), DEV, num_blocks=args.blocks, use_resid=args.use_resid)
    with torch.no_grad():                        # learners that are told apart (tests/test_gpu_transformer_population.py: visible)
        for s, net in enumerate(pop.nets):
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
    zeros = lambda E: torch.zeros(E, dtype=torch.float32, device=DEV)
    obs, done = every.reset()[0].clone(), zeros(S * E_l)
    obs_l, done_l = [e.reset()[0].clone() for e in lone], [zeros(E_l) for _ in lone]
    with torch.no_grad():
        out = every.policy_rollout_population(pop, T, obs, done)
        out_l = [e.policy_rollout(pop.nets[s], T, obs_l[s], done_l[s]) for s, e in enumerate(lone)]
        torch.cuda.synchronize()
        for s in range(S):                       # the two forms give the same storage
            for k in ("obs", "actions", "logprobs", "values", "rewards", "dones"):
                assert out[k][:, s * E_l:(s + 1) * E_l].contiguous().view(torch.int32).equal(out_l[s][k].contiguous().view(torch.int32)), (s, k)

        def together():
            every.policy_rollout_population(pop, T, obs, done, out=out)

        def loop():
            for s, e in enumerate(lone):
                e.policy_rollout(pop.nets[s], T, obs_l[s], done_l[s], out=out_l[s])

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms = event_ms(fn)
            return ms, (time.perf_counter() - t0) * 1e3
        ev, wall = {"loop": [], "population": []}, {"loop": [], "population": []}
        for pair in range(args.pairs):
            for form in (("loop", "population") if pair % 2 == 0 else ("population", "loop")):
                e_ms, w_ms = timed(loop if form == "loop" else together)
                ev[form].append(e_ms)
                wall[form].append(w_ms)
    med = {f: statistics.median(ev[f]) for f in ev}
    row = {"part": args.part, "learners": S, "learner_envs": E_l, "steps": T, "obs_dim": D, "blocks": args.blocks,
           "use_resid": bool(args.use_resid), "pairs": args.pairs}
    for f in ("loop", "population"):
        row[f] = {"ms_median": round(med[f], 3), "ms_min": round(min(ev[f]), 3), "ms_max": round(max(ev[f]), 3),
                  "host_ms_median": round(statistics.median(wall[f]), 3)}
    row["loop_over_population"] = round(med["loop"] / med["population"], 3)
    row["population_range_below_loop"] = max(ev["population"]) < min(ev["loop"])
    print(json.dumps(row))
    for e in [every] + lone:
        e.close()


def update_population_part(args):
    """S learners' whole update in one set of launches against the per-learner loop of the lone entry, interleaved; one JSON line."""
    import time
    from evacuation_amd import trainer
    from evacuation_amd.population import TransformerPopulation, TransformerPopulationAdam, population_rows, transformer_update_population
    S, E_l, T = args.learners, args.learner_envs, args.steps or 2048
    M = 192 if args.minibatch == 16384 else args.minibatch       # (the reference's minibatch unless one is named)
    D, B_l = (N_PED + 2) * 6, E_l * T
    B = S * B_l
    cfg = trainer.RPOTrainingConfig(num_envs=E_l, num_steps=T)
    seeds = list(range(1, S + 1))
    pop = TransformerPopulation(D, N_PED, seeds, DEV, num_blocks=args.blocks, use_resid=args.use_resid)
    opt = TransformerPopulationAdam(pop, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm)
    lone = []                                                    # the loop's learners: tensors of their own, the same values
    for net in pop.nets:
        twin = TransformerActorCritic(D, N_PED, num_blocks=args.blocks, use_resid=args.use_resid).to(DEV)
        with torch.no_grad():
            for p, q in zip(trainer.all_tensors(twin), trainer.all_tensors(net)):
                p.copy_(q)
        lone.append(twin)
    lone_opt = [trainer.TransformerAdam(net, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm) for net in lone]
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    batch = {"b_obs": (0.6 * rnd(B, D)).clamp(-1, 1), "b_actions": rnd(B, 2), "b_logprobs": -2.0 + 0.1 * rnd(B), "b_advantages": rnd(B),
             "b_returns": rnd(B), "b_values": rnd(B)}
    # learner s's own batch [T x E_l]: its columns of the common one [T x S E_l]
    own = [{k: v.reshape(T, S, E_l, *v.shape[1:])[:, s].reshape(B_l, *v.shape[1:]).contiguous() for k, v in batch.items()}
           for s in range(S)]
    perms = torch.stack([torch.stack([torch.randperm(B_l, device=DEV, generator=g) for _ in range(args.epochs)]) for _ in range(S)])
    rows = population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S).contiguous()
    steps = args.epochs * len(trainer.update_steps(B_l, M, cfg.norm_adv))
    stats, stats_l = torch.zeros(S, steps, 8, device=DEV), [torch.zeros(steps, 8, device=DEV) for _ in range(S)]
    need = ea.population.population_workspace_bytes(D, min(M, B_l), S, transformer=True)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def together():
        transformer_update_population(pop, batch, rows, cfg, opt, minibatch_size=M, first_draw_counters=[0] * S, stats=stats, workspace=ws)

    def loop():
        for s in range(S):
            trainer.transformer_update(lone[s], own[s], perms[s], cfg, lone_opt[s], seed=seeds[s], first_draw_counter=0, stats=stats_l[s],
                                       minibatch_size=M)
    together()
    loop()
    torch.cuda.synchronize()
    same = all(a.detach().view(torch.int32).equal(b.detach().view(torch.int32))
               for s in range(S) for a, b in zip(trainer.all_tensors(pop.nets[s]), trainer.all_tensors(lone[s])))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = event_ms(fn)
        return ms, (time.perf_counter() - t0) * 1e3
    ev, wall = {"loop": [], "population": []}, {"loop": [], "population": []}
    for pair in range(args.pairs):
        for form in (("loop", "population") if pair % 2 == 0 else ("population", "loop")):
            e_ms, w_ms = timed(loop if form == "loop" else together)
            ev[form].append(e_ms)
            wall[form].append(w_ms)
    med = {f: statistics.median(ev[f]) for f in ev}
    row = {"part": args.part, "learners": S, "learner_rows": B_l, "minibatch": M, "epochs": args.epochs, "minibatch_steps": steps,
           "launches_per_step": 6 + args.blocks + int(cfg.norm_adv), "obs_dim": D, "blocks": args.blocks, "use_resid": bool(args.use_resid),
           "pairs": args.pairs, "first_update_same_bits": bool(same)}
    for f in ("loop", "population"):
        row[f] = {"ms_median": round(med[f], 3), "ms_min": round(min(ev[f]), 3), "ms_max": round(max(ev[f]), 3),
                  "host_ms_median": round(statistics.median(wall[f]), 3)}
    row["loop_over_population"] = round(med["loop"] / med["population"], 3)
    row["population_range_below_loop"] = max(ev["population"]) < min(ev["loop"])
    print(json.dumps(row))


def update_part(args):
    """One whole update's epochs at N = 60, rel + ohe Box (D = 372), three ways: whole updates between two events after one
    warm-up update (tools/deepsets_bench.py's update parts with this network's entries)."""
    from evacuation_amd import trainer
    E, T, M = args.envs, args.steps, args.minibatch
    D, B = (N_PED + 2) * 6, E * T
    torch.manual_seed(0)
    net = TransformerActorCritic(D, N_PED, num_blocks=args.blocks, use_resid=args.use_resid).to(DEV)
    cfg = trainer.RPOTrainingConfig(num_envs=E, num_steps=T)
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    batch = {"b_obs": (0.6 * rnd(B, D)).clamp(-1, 1), "b_actions": rnd(B, 2), "b_logprobs": -2.0 + 0.1 * rnd(B), "b_advantages": rnd(B),
             "b_returns": rnd(B), "b_values": rnd(B)}
    perms = torch.stack([torch.randperm(B, device=DEV, generator=g) for _ in range(args.epochs)]).contiguous()
    sizes = trainer.update_steps(B, M, cfg.norm_adv)
    steps = args.epochs * len(sizes)
    params = list(trainer.all_tensors(net))
    trainer.ensure_grads(net)
    stats, rows = torch.zeros(8, device=DEV), torch.zeros(steps, 8, device=DEV)
    if args.part == "update-torch":
        opt = torch.optim.Adam(params, lr=cfg.learning_rate, eps=1e-5)

        def step(inds, k):
            trainer.transformer_minibatch_grad(net, batch, inds, cfg, seed=1, draw_counter=k, stats=stats)
            coef = torch.clamp(cfg.max_grad_norm / (stats[7].sqrt() + 1e-6), max=1.0)       # RPOTrainer.apply_gradient
            torch._foreach_mul_([p.grad for p in params], coef)
            opt.step()
    else:
        opt = trainer.TransformerAdam(net, lr=cfg.learning_rate, eps=1e-5, max_grad_norm=cfg.max_grad_norm)

        def step(inds, k):
            trainer.transformer_minibatch_step(net, batch, inds, cfg, opt, seed=1, draw_counter=k, stats=stats)

    def run():
        if args.part == "update-one-call":
            trainer.transformer_update(net, batch, perms, cfg, opt, seed=1, first_draw_counter=0, stats=rows, minibatch_size=M)
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
    print(json.dumps({"part": args.part, "envs": E, "steps": T, "batch": B, "minibatch": M, "epochs": args.epochs, "blocks": args.blocks,
                      "use_resid": bool(args.use_resid), "minibatch_steps": steps, "launches_per_step": 6 + args.blocks + int(cfg.norm_adv),
                      "ms_per_update_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "us_per_minibatch_step": round(med / steps * 1e3, 2), "updates": len(ms),
                      "finite": bool(all(torch.isfinite(p).all() for p in params))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["a", "b", "c", "c-eager", "grad-autograd", "grad-device", "update-torch", "update-step",
                                                     "update-one-call", "collect-population", "update-population", "collect-sweep",
                                                     "update-sweep"])
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=None, help="default 128; collect-population: 2048")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--use-resid", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="update-*: the epochs of one update")
    ap.add_argument("--learners", type=int, default=4, help="collect-population, update-population: the learners")
    ap.add_argument("--learner-envs", type=int, default=3, help="collect-population, update-population: a learner's envs")
    ap.add_argument("--pairs", type=int, default=9, help="collect-population, update-population: interleaved pairs")
    args = ap.parse_args()
    if args.part in ("collect-sweep", "update-sweep"):               # (tools/encoder_sweep_bench.py: shared with deepsets_bench.py)
        import encoder_sweep_bench
        args.envs, args.steps = args.learner_envs, args.steps or 2048
        args.minibatch = 192 if args.minibatch == 16384 else args.minibatch
        part = encoder_sweep_bench.collect_sweep_part if args.part == "collect-sweep" else encoder_sweep_bench.update_sweep_part
        return part(args, "transformer")
    if args.part == "collect-population":
        return collect_population_part(args)
    if args.part == "update-population":
        return update_population_part(args)
    args.steps = args.steps or 128
    if args.part.startswith("update-"):
        return update_part(args)
    if args.part.startswith("grad-"):
        return grad_part(args)
    E, T = args.envs, args.steps
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=N_PED), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                      num_envs=E, gamma=0.99, seed=1)
    D = env.obs_dim
    torch.manual_seed(0)
    net = (LinearActorCritic(D) if args.part == "a" else
           TransformerActorCritic(D, N_PED, num_blocks=args.blocks, use_resid=args.use_resid)).to(DEV)
    first, _ = env.reset()
    if args.part in ("a", "b"):
        next_obs, next_done = first.clone(), torch.zeros(E, dtype=torch.float32, device=DEV)
        with torch.no_grad():
            out = env.policy_rollout(net, T, next_obs, next_done)

        def run():
            env.policy_rollout(net, T, next_obs, next_done, out=out)
    else:
        net.eval()
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
    print(json.dumps({"part": args.part, "envs": E, "steps": T, "obs_dim": D, "blocks": args.blocks, "use_resid": bool(args.use_resid),
                      "ms_per_call_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "us_per_vector_step": round(med / T * 1e3, 3), "env_steps_per_s": round(E * T / (med * 1e-3), 1), "calls": len(ms)}))
    env.close()


if __name__ == "__main__":
    main()
