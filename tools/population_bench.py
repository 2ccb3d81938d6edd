#!/usr/bin/env python3
"""Time S learners' updates, as a population or one after another ("population").

    python tools/population_bench.py --tree . --form population --shapes 3:2048:1,3:2048:4,3:2048:10
    python tools/population_bench.py --tree ../parent-checkout --form standalone --shapes 3:2048:10

`--tree`: the checkout whose package and libevac.so are timed (a built checkout of another commit for an A/B run; the two
builds run as separate processes, alternated by the caller inside every repetition).  `--form standalone`: S
``RPOTrainer(optimizer="device")`` on handles of E_l envs, updated one after another; `--form population`: one
``PopulationTrainer`` of S learners; `--form sweep_equal` / `sweep_differ`: the same population given S configurations (the
per-learner path), all equal or differing in learning rate, annealing, gamma, lambda, the loss
coefficients, max_grad_norm and target_kl (none of them reached, so every form runs the same steps).  The reference's 32 minibatches x 10 epochs, N = 60, gravity observation.  hipEvent times
after two warm-up windows; one JSON line per shape: the milliseconds of each window of S learner-updates."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True)
ap.add_argument("--form", required=True, choices=("standalone", "population", "sweep_equal", "sweep_differ"))
ap.add_argument("--shapes", required=True, help="E_l:T:S,E_l:T:S,...")
ap.add_argument("--windows", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch
import evacuation_amd as ea
from evacuation_amd.policy import LinearActorCritic
from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig
assert os.path.abspath(ea.__file__).startswith(os.path.abspath(args.tree)), ea.__file__
DEV = torch.device("cuda:0")


def cfg_of(E_l, T, seed):
    return RPOTrainingConfig(num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 1000, num_minibatches=32, update_epochs=10, seed=seed)


def env_of(E, cfg, offset=0):
    return ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=60, is_new_exiting_reward=True),
                                       ea.EnvWrappersConfig(positions="grav", alpha=3), num_envs=E, gamma=cfg.gamma, seed=1, env_id_offset=offset)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


for shape in args.shapes.split(","):
    E_l, T, S = (int(x) for x in shape.split(":"))
    seeds = list(range(1, S + 1))
    if args.form == "standalone":
        trs = []
        for s in range(S):
            cfg = cfg_of(E_l, T, seeds[s])
            env = env_of(E_l, cfg, s * E_l)
            torch.manual_seed(seeds[s])
            trs.append(RPOTrainer(env, LinearActorCritic(env.obs_dim).to(DEV), cfg, optimizer="device", one_call=True))
        def window():
            for tr in trs:
                tr.update()
        close = lambda: [tr.env.close() for tr in trs]
    else:
        from evacuation_amd.population import PolicyPopulation, PopulationTrainer
        import dataclasses
        cfg = cfg_of(E_l, T, 0)
        env = env_of(S * E_l, cfg)
        cfgs = cfg
        if args.form == "sweep_equal":
            cfgs = [dataclasses.replace(cfg) for _ in range(S)]
        elif args.form == "sweep_differ":
            cfgs = [dataclasses.replace(cfg, learning_rate=3e-4 * (1 + s), anneal_lr=bool(s % 2), gamma=0.99 - 0.01 * s,
                                        gae_lambda=0.95 - 0.02 * s, clip_coef=0.2 + 0.01 * s, ent_coef=0.001 * s, vf_coef=0.5 + 0.05 * s,
                                        rpo_alpha=0.5 - 0.03 * s, max_grad_norm=0.5 + 0.1 * s, target_kl=None if s % 3 == 0 else 1e9)
                    for s in range(S)]
        ptr = PopulationTrainer(env, PolicyPopulation(env.obs_dim, seeds, DEV), cfgs)
        window = ptr.update
        close = env.close
    window(); window()
    torch.cuda.synchronize()
    ms = [timed(window) for _ in range(args.windows)]
    print(json.dumps({"tree": os.path.basename(os.path.abspath(args.tree)), "form": args.form, "E_l": E_l, "T": T, "S": S, "ms": ms}), flush=True)
    close()
