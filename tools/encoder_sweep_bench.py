"""The parts of tools/deepsets_bench.py and tools/transformer_bench.py that measure a SWEEP of an encoder population (DESIGN.md
4.22, 8.1), written once for both encoders (``kind``: "deepsets" or "transformer"):

  update-sweep   one whole update's epochs of S learners at the reference's shape (``--envs`` 3 x ``--steps`` 2048 rows per
                 learner, minibatches of ``--minibatch`` 192, ``--epochs`` 10, N = 60, D = 372, two blocks), three ways on the same
                 common batch: ``*_update_sweep`` with a configuration per learner, ``*_update_population`` under one configuration,
                 and the loop of S lone ``*_update`` calls; hipEvent times of whole calls after two warm-up calls of each form, the
                 three forms alternated inside every repetition, median and range of ``--reps`` repetitions
  collect-sweep  ``policy_rollout_sweep`` with a gamma per learner against ``policy_rollout_population`` on the same wrapped env,
                 likewise alternated
One JSON line.  One part per process."""
import dataclasses
import json
import statistics

import torch

import evacuation_amd as ea
from evacuation_amd import population, trainer

DEV = torch.device("cuda:0")
N_PED = 60


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def make_population(kind, D, seeds, blocks=2):
    if kind == "transformer":
        return population.TransformerPopulation(D, N_PED, seeds, DEV, num_blocks=blocks)
    return population.DeepSetsPopulation(D, N_PED, seeds, DEV)


def update_sweep_part(args, kind):
    tf = kind == "transformer"
    S, E_l, T, M, epochs = args.learners, args.envs, args.steps, args.minibatch, args.epochs
    D, B_l = (N_PED + 2) * 6, E_l * T
    cfg = trainer.RPOTrainingConfig(num_envs=E_l, num_steps=T, learning_rate=1e-5)
    cfgs = [dataclasses.replace(cfg, learning_rate=1e-5 * (1 + s), ent_coef=0.01 * (s % 3), clip_coef=0.2 + 0.01 * s) for s in range(S)]
    seeds = list(range(1, S + 1))
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    B = S * B_l
    common = {"b_obs": rnd(B, D).clamp(-5, 5), "b_actions": rnd(B, 2), "b_logprobs": -2.0 + 0.1 * rnd(B), "b_advantages": rnd(B),
              "b_returns": rnd(B), "b_values": rnd(B)}
    perms = torch.stack([torch.stack([torch.randperm(B_l, device=DEV, generator=g) for _ in range(epochs)]) for _ in range(S)])
    index = torch.arange(S, device=DEV).reshape(S, 1, 1)
    rows = population.population_rows(perms, index, E_l, S).contiguous()
    own = population.population_rows(torch.arange(B_l, device=DEV).expand(S, 1, B_l), index, E_l, S).reshape(S, B_l)
    batches = [{k: v[own[s]].contiguous() for k, v in common.items()} for s in range(S)]        # a learner's own rows, for the loop
    steps = epochs * len(trainer.update_steps(B_l, M, cfg.norm_adv))
    make_adam = population.TransformerPopulationAdam if tf else population.PopulationAdam
    lone_adam = trainer.TransformerAdam if tf else trainer.DeviceAdam
    lone_update = trainer.transformer_update if tf else trainer.deepsets_update
    sweep_update = population.transformer_update_sweep if tf else population.deepsets_update_sweep
    pop_update = population.transformer_update_population if tf else population.deepsets_update_population
    pa, pb, pc = (make_population(kind, D, seeds) for _ in range(3))
    oa = make_adam(pa, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
    ob = make_adam(pb, lr=cfg.learning_rate)
    oc = [lone_adam(net, lr=c.learning_rate, max_grad_norm=c.max_grad_norm) for net, c in zip(pc.nets, cfgs)]
    stats = [torch.zeros(S, steps, 8, device=DEV) for _ in range(3)]
    ws = {sweep: torch.empty(population.population_workspace_bytes(D, M, S, sweep=sweep, **{kind: True}), dtype=torch.uint8, device=DEV)
          for sweep in (True, False)}
    counters = [0] * S

    def sweep():
        sweep_update(pa, common, rows, cfgs, oa, minibatch_size=M, first_draw_counters=counters, stats=stats[0], workspace=ws[True])

    def one_configuration():
        pop_update(pb, common, rows, cfg, ob, minibatch_size=M, first_draw_counters=counters, stats=stats[1], workspace=ws[False])

    def loop():
        for s in range(S):
            lone_update(pc.nets[s], batches[s], perms[s], cfgs[s], oc[s], seed=seeds[s], first_draw_counter=0, stats=stats[2][s],
                        minibatch_size=M)
    forms = {"sweep": sweep, "population": one_configuration, "loop": loop}
    for _ in range(2):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(max(3, args.reps)):
        for name, fn in forms.items():
            ms[name].append(event_ms(fn))
    med = {name: statistics.median(v) for name, v in ms.items()}
    finite = all(bool(torch.isfinite(t).all()) for p in (pa, pb, pc) for t in p.tensors)
    print(json.dumps({"part": args.part, "network": kind, "learners": S, "rows_per_learner": B_l, "minibatch": M, "epochs": epochs,
                      "minibatch_steps": steps, "obs_dim": D, **{f"{name}_ms": spread(v) for name, v in ms.items()},
                      "sweep_over_population": round(med["sweep"] / med["population"], 4),
                      "loop_over_sweep": round(med["loop"] / med["sweep"], 3), "updates": len(ms["sweep"]), "finite": finite}))


def collect_sweep_part(args, kind):
    S, E_l, T = args.learners, args.envs, args.steps
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=N_PED), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                      num_envs=S * E_l, gamma=0.99, seed=1)
    pop = make_population(kind, env.obs_dim, list(range(1, S + 1)))
    gammas = [0.99 - 0.01 * (s % 5) for s in range(S)]
    first, _ = env.reset()
    next_obs, next_done = first.clone(), torch.zeros(S * E_l, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        out = env.policy_rollout_population(pop, T, next_obs, next_done)
    forms = {"sweep": lambda: env.policy_rollout_sweep(pop, T, next_obs, next_done, gammas, out=out),
             "population": lambda: env.policy_rollout_population(pop, T, next_obs, next_done, out=out)}
    for _ in range(2):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(max(5, args.reps)):
        for name, fn in forms.items():
            ms[name].append(event_ms(fn))
    med = {name: statistics.median(v) for name, v in ms.items()}
    print(json.dumps({"part": args.part, "network": kind, "learners": S, "envs_per_learner": E_l, "steps": T, "obs_dim": env.obs_dim,
                      **{f"{name}_ms": spread(v) for name, v in ms.items()},
                      "sweep_over_population": round(med["sweep"] / med["population"], 4), "calls": len(ms["sweep"])}))
    env.close()
