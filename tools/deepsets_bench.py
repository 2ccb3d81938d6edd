#!/usr/bin/env python3
"""Measure the deep-sets leader's collection phase (evac_policy_rollout_deepsets) against what it stands beside and what it
replaces, and its minibatch gradient on the device (evac_deepsets_minibatch_grad) against autograd's.

    python tools/deepsets_bench.py --part a|b|c|c-eager|grad-autograd|grad-device [--envs 4096] [--steps 128] [--reps 7]

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


def grad_part(args):
    """One minibatch gradient of all 19 tensors: whole calls between two events after two warm-up calls."""
    from types import SimpleNamespace

    from evacuation_amd import trainer
    E, T, M = args.envs, args.steps, args.minibatch
    D, B = (N_PED + 2) * 6, E * T
    torch.manual_seed(0)
    net = DeepSetsActorCritic(D, N_PED).to(DEV)
    cfg = trainer.RPOTrainingConfig(num_envs=E, num_steps=T)
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    batch = {"b_obs": rnd(B, D).clamp(-5, 5), "b_actions": rnd(B, 2), "b_logprobs": -2.0 + 0.1 * rnd(B), "b_advantages": rnd(B),
             "b_returns": rnd(B), "b_values": rnd(B)}
    inds = torch.randperm(B, device=DEV, generator=g)[:M].contiguous()
    z = ((torch.rand(M, 2, device=DEV, generator=g) * 2 - 1) * cfg.rpo_alpha).contiguous()
    stats = torch.zeros(8, device=DEV)
    holder = SimpleNamespace(net=net, cfg=cfg)
    trainer.ensure_grads(net)
    if args.part == "grad-device":
        def run():
            trainer.deepsets_minibatch_grad(net, batch, inds, cfg, rpo_noise=z, stats=stats)
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
    ap.add_argument("--part", required=True, choices=["a", "b", "c", "c-eager", "grad-autograd", "grad-device"])
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.part.startswith("grad-"):
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
