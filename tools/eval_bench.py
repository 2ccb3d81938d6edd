#!/usr/bin/env python3
"""Measure the policy evaluation kernel (evac_policy_evaluate) against the policy rollout.

    python tools/eval_bench.py [--envs 4096] [--steps 128] [--reps 9] [--shape grav|wide|both] [--evaluate-only]
    python tools/eval_bench.py --learners S [--learner-envs 256] [--pairs 9] [--network linear|deep_sets|transformer]
    python tools/eval_bench.py --capture K [--envs 4096] [--steps 128] [--reps 9]

Per shape -- N = 60 with the gravity observation (D = 6), and with the rel + ohe Box observation (D = 372), both with the frozen
normaliser -- the time per env-step of ``policy_evaluate(mean, max_steps = T)`` and of ``policy_rollout(T)`` from the same start
state: hipEvent times after warm-up, the two forms alternated inside every repetition, median and range.  Then one
``PolicyEvaluator.evaluate(n_episodes = 1)`` at the default ``max_timesteps`` (host wall time and launches) and one launch of
4096 steps, which is what the ``max_steps_per_launch`` default rests on.  ``--evaluate-only`` runs just the evaluate() part
(for a kernel trace: ``rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --evaluate-only``).

``--learners S`` measures the population evaluation instead: S learners of ``--learner-envs`` envs each, N = 60 with the gravity
observation and the frozen normaliser, one episode per env at the default ``max_timesteps`` -- a loop of S
``PolicyEvaluator.evaluate`` calls (one learner after another) against ONE ``PopulationEvaluator.evaluate``, the same nets and
statistics, one warm-up of each, then interleaved pairs whose order alternates: hipEvent time and host wall time, median and
range, and the S ``summary()`` reads against one ``EvaluationResult.summaries``.  ``--network deep_sets``: the same for a
``DeepSetsPopulation`` on the rel + ohe Box observation (D = 372), its learners made visible as the tests make them -- the loop is
what ``PopulationTrainer.evaluate()`` ran for such a population before ``evac_policy_evaluate_population_deepsets``.  ``--network transformer``:
the same for a ``TransformerPopulation`` (two blocks) on that observation, against the loop of the lone entry
(``evac_policy_evaluate_transformer``); a report, whatever the ratio.  The exit
code says whether the population call's whole host-wall range lies below the loop's.

``--capture K`` measures what recording costs (``policy_evaluate(capture=...)``, the ``k_evaluate_capture*`` kernels): N = 60, the
gravity observation, the frozen normaliser -- ``policy_evaluate(mean, max_steps = T)`` without and with the frames of envs
``0..K-1`` from the same start state, alternated inside every repetition, and one ``PolicyEvaluator.evaluate(n_episodes = 1)`` at
the default ``max_timesteps`` without and with ``capture_envs = K`` (host wall time, the buffers' allocation included).  A
report, not a threshold: recording is a diagnostic face."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evacuation_amd as ea  # noqa: E402
from evacuation_amd.policy import LinearActorCritic  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"grav": dict(positions="grav", alpha=3), "wide": dict(positions="rel", statuses="ohe", type="Box")}
STATE = ("ped", "status", "agent", "clock", "acc")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def show(v, scale=1.0, unit="ms"):
    return f"{statistics.median(v) * scale:10.3f} {unit}  [{min(v) * scale:.3f} .. {max(v) * scale:.3f}]"


def kernel_against_rollout(shape, args):
    E, T = args.envs, args.steps
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=60, is_new_exiting_reward=True), ea.EnvWrappersConfig(**SHAPES[shape]),
                                      num_envs=E, seed=1)
    b = env.env
    torch.manual_seed(0)
    net = LinearActorCritic(env.obs_dim).to(DEV)
    obs, _ = env.reset()
    next_obs, next_done = obs.clone(), torch.zeros(E, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        storage = env.policy_rollout(net, T, next_obs, next_done)             # the statistics move; allocates the storage
        storage = env.policy_rollout(net, T, next_obs, next_done, out=storage)
        keep = {k: getattr(b, k).clone() for k in STATE}
        keep_ns, keep_obs, keep_done = env.norm_state.clone(), next_obs.clone(), next_done.clone()
        progress, out = env.policy_evaluate(net, T, T)

        def rewind():
            for k in STATE:
                getattr(b, k).copy_(keep[k])
            env.norm_state.copy_(keep_ns)
            next_obs.copy_(keep_obs)
            next_done.copy_(keep_done)
            progress.zero_()

        def rollout():
            env.policy_rollout(net, T, next_obs, next_done, out=storage)

        def evaluate():
            env.policy_evaluate(net, T, T, progress, out)
        for _ in range(2):                                                     # warm-up of both forms from the start state
            rewind(); rollout(); rewind(); evaluate()
        torch.cuda.synchronize()
        t_ro, t_ev = [], []
        for rep in range(args.reps):                                           # alternated inside every repetition
            for form in (("ro", "ev") if rep % 2 == 0 else ("ev", "ro")):
                rewind()
                torch.cuda.synchronize()
                (t_ro if form == "ro" else t_ev).append(event_ms(rollout if form == "ro" else evaluate))
    per = 1e6 / (E * T)                                                        # ms per launch -> ns per env-step
    print(f"[{shape}] N = 60, D = {env.obs_dim}, {E} envs x {T} steps, frozen normaliser; median [min .. max] of {args.reps} repetitions")
    print(f"    policy_rollout({T})              {show(t_ro)}   {show(t_ro, per, 'ns / env-step')}")
    print(f"    policy_evaluate(mean, {T})       {show(t_ev)}   {show(t_ev, per, 'ns / env-step')}")
    ok = statistics.median(t_ev) <= max(t_ro)
    print(f"    evaluation median / rollout median = {statistics.median(t_ev) / statistics.median(t_ro):.3f}; "
          f"evaluation median {'within or below' if ok else 'ABOVE'} the rollout's range")
    env.close()
    return ok


def capture_against_plain(args):
    E, T, K = args.envs, args.steps, args.capture
    cfg = ea.EnvConfig(number_of_pedestrians=60, is_new_exiting_reward=True, clip_action=True)
    ev = ea.PolicyEvaluator(cfg, ea.EnvWrappersConfig(**SHAPES["grav"]), num_envs=E, seed=1)
    env = ev.env
    torch.manual_seed(0)
    net = LinearActorCritic(6).to(DEV)
    ns = torch.zeros((E, 22), dtype=torch.float64, device=DEV)
    ns[:, 6:12] = 1.0
    norm = (ns, 1.0, 1e-8)
    cap = {"frames": torch.zeros((T, K, 61, 3), dtype=torch.float32, device=DEV), "starts": torch.zeros((T, K, 61, 3), dtype=torch.float32, device=DEV)}
    with torch.no_grad():
        progress, out = env.policy_evaluate(net, T, T, _norm=norm)
        forms = {"plain": lambda: env.policy_evaluate(net, T, T, progress, out, _norm=norm),
                 "capture": lambda: env.policy_evaluate(net, T, T, progress, out, _norm=norm, capture=cap)}

        def rewind():
            ev.restore()
            progress.zero_()
        for _ in range(2):
            for fn in forms.values():
                rewind(); fn()
        torch.cuda.synchronize()
        t = {"plain": [], "capture": []}
        for rep in range(args.reps):                                           # alternated inside every repetition
            for form in (("plain", "capture") if rep % 2 == 0 else ("capture", "plain")):
                rewind()
                torch.cuda.synchronize()
                t[form].append(event_ms(forms[form]))
        per = 1e6 / (E * T)
        print(f"[capture] N = 60, D = 6, {E} envs x {T} steps, frozen normaliser, K = {K} recorded envs; median [min .. max] of {args.reps} repetitions")
        print(f"    policy_evaluate(mean, {T})                {show(t['plain'])}   {show(t['plain'], per, 'ns / env-step')}")
        print(f"    policy_evaluate(mean, {T}, capture)       {show(t['capture'])}   {show(t['capture'], per, 'ns / env-step')}")
        print(f"    capture median / plain median = {statistics.median(t['capture']) / statistics.median(t['plain']):.3f}")
        for name, kw in (("without capture", {}), (f"capture_envs = {K}", dict(capture_envs=K))):
            ev.evaluate(net, 1, norm_state=ns, **kw)                           # warm-up
            torch.cuda.synchronize()
            wall = []
            for _ in range(args.eval_reps):
                t0 = time.perf_counter()
                res = ev.evaluate(net, 1, norm_state=ns, **kw)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            print(f"evaluate(n_episodes=1), {E} envs, max_timesteps = {cfg.max_timesteps}, {name}: {show(wall)} host wall time, "
                  f"{ev.launches} launch(es), {int(res.steps.sum())} env-steps")
    ev.close()


def whole_evaluation(args):
    E = args.envs
    cfg = ea.EnvConfig(number_of_pedestrians=60, is_new_exiting_reward=True, clip_action=True)
    ev = ea.PolicyEvaluator(cfg, ea.EnvWrappersConfig(**SHAPES["grav"]), num_envs=E, seed=1)
    torch.manual_seed(0)
    net = LinearActorCritic(6).to(DEV)
    ns = torch.zeros((E, 22), dtype=torch.float64, device=DEV)
    ns[:, 6:12] = 1.0
    with torch.no_grad():
        for name, agent, kw in (("policy (mean), frozen normaliser", net, dict(norm_state=ns)), ("vacuum_cleaner", "vacuum_cleaner", {})):
            ev.evaluate(agent, 1, **kw)                                        # warm-up
            torch.cuda.synchronize()
            wall = []
            for _ in range(args.eval_reps):
                t0 = time.perf_counter()
                res = ev.evaluate(agent, 1, **kw)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            s = res.summary()
            steps = int(res.steps.sum())
            print(f"evaluate(n_episodes=1), {E} envs, max_timesteps = {cfg.max_timesteps}, {name}: {show(wall)} host wall time, "
                  f"{ev.launches} launch(es), {steps} env-steps ({statistics.median(wall) * 1e6 / steps:.2f} ns / env-step), "
                  f"episodic_return {s['episode_reward_mean']:.2f}, length {s['episode_length_mean']:.1f}, escaped {s['escaped_fraction_mean']:.3f}")
        if not args.evaluate_only:
            # one launch of max_steps_per_launch = 4096 steps that no env finishes early (n_episodes = 8 at max_timesteps = 2000)
            progress, out = ev.env.policy_evaluate(net, 8, 4096, _norm=(ns, 1.0, 1e-8))
            torch.cuda.synchronize()
            t = []
            for _ in range(args.eval_reps):
                ev.restore()
                progress.zero_()
                torch.cuda.synchronize()
                t.append(event_ms(lambda: ev.env.policy_evaluate(net, 8, 4096, progress, out, _norm=(ns, 1.0, 1e-8))))
            assert int(progress[:, 1].min()) == 4096
            print(f"one launch of 4096 steps, {E} envs (policy, frozen normaliser): {show(t)}   {show(t, 1e6 / (E * 4096), 'ns / env-step')}")
    ev.close()


def visible_deepsets_population(D, N, S):
    """Freshly seeded deep-sets learners whose actions are told apart, each in its own way (tests/test_gpu_deepsets_population.py: visible)."""
    from evacuation_amd.population import DeepSetsPopulation
    pop = DeepSetsPopulation(D, N, list(range(1, S + 1)), DEV)
    with torch.no_grad():
        for s, net in enumerate(pop.nets):
            g = torch.Generator().manual_seed(1000 + s)
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
            net.deep_sets.transform_rho[0].weight.mul_(3.0 / (N + 2))
    return pop


def visible_transformer_population(D, N, S):
    """Freshly seeded transformer learners (two blocks) whose actions are told apart (tests/test_gpu_transformer_population.py: visible)."""
    from evacuation_amd.population import TransformerPopulation
    pop = TransformerPopulation(D, N, list(range(1, S + 1)), DEV)
    with torch.no_grad():
        for s, net in enumerate(pop.nets):
            g = torch.Generator().manual_seed(1000 + s)
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
    return pop


def population_against_loop(args):
    from evacuation_amd.evaluation import EvaluationResult, PopulationEvaluator
    S, E_l = args.learners, args.learner_envs
    deep_sets, transformer = args.network == "deep_sets", args.network == "transformer"
    cfg = ea.EnvConfig(number_of_pedestrians=60, is_new_exiting_reward=True, clip_action=True)
    wrap = ea.EnvWrappersConfig(**SHAPES["wide" if deep_sets or transformer else "grav"])
    one = ea.PolicyEvaluator(cfg, wrap, num_envs=E_l, seed=1)
    every = PopulationEvaluator(cfg, wrap, num_learners=S, num_envs=E_l, seed=1)
    D = every.env.obs_dim
    if transformer:
        pop = visible_transformer_population(D, 60, S)
    else:
        pop = visible_deepsets_population(D, 60, S) if deep_sets else ea.PolicyPopulation(6, list(range(1, S + 1)), DEV)
    g = torch.Generator().manual_seed(0)
    ns = torch.zeros((S, E_l, 3 * D + 4), dtype=torch.float64)               # frozen rows that differ per learner and env
    ns[..., :D] = torch.randn((S, E_l, D), generator=g, dtype=torch.float64) * 0.1
    ns[..., D:2 * D] = torch.rand((S, E_l, D), generator=g, dtype=torch.float64) + 0.5
    ns = ns.to(DEV)
    launches = {}

    def loop():
        launches["loop"] = 0
        res = []
        for s in range(S):
            res.append(one.evaluate(pop.nets[s], 1, norm_state=ns[s]))
            launches["loop"] += one.launches
        return res

    def together():
        res = every.evaluate(pop, 1, norm_state=ns)
        launches["population"] = every.launches
        return res

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        return res, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    with torch.no_grad():
        r_loop, r_pop = loop(), together()                                     # one warm-up of each
        for s in range(S):                                                     # the two paths give the same records
            for k in r_loop[s].episodes:
                assert r_loop[s].episodes[k].contiguous().view(torch.int32).equal(r_pop[s].episodes[k].contiguous().view(torch.int32)), (s, k)
        ev = {"loop": [], "population": []}
        wall = {"loop": [], "population": []}
        summ = {"loop": [], "population": []}
        for pair in range(args.pairs):
            for form in (("loop", "population") if pair % 2 == 0 else ("population", "loop")):
                res, e_ms, w_ms = timed(loop if form == "loop" else together)
                ev[form].append(e_ms)
                wall[form].append(w_ms)
                if form == "loop":
                    summ[form].append(host_ms(lambda: [r.summary() for r in res]))
                else:
                    summ[form].append(host_ms(lambda: EvaluationResult.summaries(res)))
    steps = int(sum(int(r.steps.sum()) for r in r_pop))
    print(f"[population, {args.network}] S = {S} learners x {E_l} envs, N = 60, D = {D}, frozen normaliser, 1 episode per env, max_timesteps = "
          f"{cfg.max_timesteps}, {steps} env-steps; median [min .. max] of {args.pairs} interleaved pairs")
    for form, name in (("loop", f"{S} x PolicyEvaluator.evaluate     "), ("population", "1 x PopulationEvaluator.evaluate")):
        print(f"    {name}  events {show(ev[form])}   host {show(wall[form])}   {launches[form]} launch(es)   summaries {show(summ[form])}")
    r_ev = statistics.median(ev["loop"]) / statistics.median(ev["population"])
    r_wall = statistics.median(wall["loop"]) / statistics.median(wall["population"])
    r_all = (statistics.median(wall["loop"]) + statistics.median(summ["loop"])) / \
        (statistics.median(wall["population"]) + statistics.median(summ["population"]))
    print(f"    loop / population: events {r_ev:.2f} x, host {r_wall:.2f} x, host with the summaries {r_all:.2f} x")
    below = max(wall["population"]) < min(wall["loop"])
    print(f"    the population call's whole host-wall range lies {'below' if below else 'NOT below'} the loop's")
    one.close()
    every.close()
    return True if transformer else (below if deep_sets else r_wall >= 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--eval-reps", type=int, default=3)
    ap.add_argument("--shape", choices=("grav", "wide", "both"), default="both")
    ap.add_argument("--evaluate-only", action="store_true")
    ap.add_argument("--learners", type=int, default=0, help="measure the population evaluation with this many learners instead")
    ap.add_argument("--learner-envs", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--network", choices=("linear", "deep_sets", "transformer"), default="linear", help="with --learners: the learners' network")
    ap.add_argument("--capture", type=int, default=0, metavar="K", help="measure an evaluation without and with the frames of K envs instead")
    args = ap.parse_args()
    if args.capture:
        capture_against_plain(args)
        return 0
    if args.learners:
        return 0 if population_against_loop(args) else 1
    ok = True
    if not args.evaluate_only:
        for shape in (("grav", "wide") if args.shape == "both" else (args.shape,)):
            ok = kernel_against_rollout(shape, args) and ok
    whole_evaluation(args)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
